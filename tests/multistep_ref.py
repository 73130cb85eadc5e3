"""Reference loops for the multistep solvers, shared by test_multistep_cpu.py (which checks THIS file on the CPU: against the
oracle's DDIM loop at order 1, against a closed-form probability-flow ODE, and against the host classes' coefficient rows) and
test_gpu_multistep.py (which checks the device sampler against it).  No new oracle code: as the ``oracle.sampler`` loops, these take
the UNet / ControlNet as callables; guidance is ``guidance_ref.GuidedUNet`` around them.

The formulas are written out term by term (nothing is folded), in float64:

    alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log(alpha / sigma), abar clamped to 2^-24
    m_i = (x_i - sigma_i eps_i) / alpha_i,  h = lambda_next - lambda_cur

DPM-Solver++ 2M (Lu et al. 2022), midpoint:
    x' = (sigma'/sigma) x - alpha' (e^-h - 1) m_i - 1/2 alpha' (e^-h - 1) (m_i - m_{i-1}) / r0,   r0 = (lambda_i - lambda_{i-1}) / h
UniPC bh2 (Zhao et al. 2023), data prediction, B(h) = phi_1 = expm1(-h):
    predictor  x' = (sigma'/sigma_i) x_i^c - alpha' phi_1 m_i - alpha' B sum_k rho_k (m_{i-k} - m_i) / r_k
    corrector  x_i^c = (sigma_i/sigma_{i-1}) x_{i-1}^c - alpha_i phi_1 m_{i-1}
                       - alpha_i B (sum_k rho_k (m_{i-1-k} - m_{i-1}) / r_k + rho_last (m_i - m_{i-1}))
With ``lr_latents`` the solver runs on z = x - LR (the model still sees x)."""
import math

import numpy as np
import torch

ABAR_MIN = 2.0 ** -24


def grid(timesteps, alphas_cumprod, final_sigmas_type):
    ts = [int(t) for t in timesteps]
    ac = alphas_cumprod.to(torch.float32).double().numpy()
    abar = np.maximum(np.array([ac[t] for t in ts] + [ac[0]]), ABAR_MIN)
    al, sg = np.sqrt(abar), np.sqrt(1.0 - abar)
    lam = np.log(al / sg)
    if final_sigmas_type == "zero":
        al[-1], sg[-1], lam[-1] = 1.0, 0.0, math.inf
    else:
        assert final_sigmas_type == "sigma_min"
    return ts, al, sg, lam


def unipc_rhos(rks, h, k):
    """rho: the leading k x k block of R rho = b (rows of R: rks^(j-1); b_j = phi_{j+1}-recurrence value * j! / B(h))."""
    hh = -h
    Bh = math.expm1(hh)
    phik, fact = math.expm1(hh) / hh - 1.0, 1.0
    R, b = [], []
    for j in range(1, len(rks) + 1):
        R.append([r ** (j - 1) for r in rks])
        b.append(phik * fact / Bh)
        fact *= j + 1
        phik = phik / hh - 1.0 / fact
    return np.linalg.solve(np.array(R)[:k, :k], np.array(b)[:k])


def multistep_sample(kind, unet, x_T, ctx, timesteps, alphas_cumprod, solver_order=2, final_sigmas_type="zero", disable_corrector=(),
                     lr_latents=None, controlnet=None, control_image=None, intrablock=None, first=0, last=None):
    """States of a run over steps [first, last) that starts COLD at ``first`` with state ``x_T``: [x_first, ..., x_last].  The model
    is called in ``x_T``'s dtype; the solver state is float64."""
    assert kind in ("unipc", "dpmsolver++")
    ts, al, sg, lam = grid(timesteps, alphas_cumprod, final_sigmas_type)
    n = len(ts)
    last = n if last is None else last
    mdt = x_T.dtype
    lr = lr_latents.double() if lr_latents is not None else 0.0
    x = x_T.double()
    traj = [x.to(mdt)]
    ms = {}          # i -> m_i (z space)
    zc_prev = None   # corrected state of the previous step
    order_prev = None
    for i in range(first, last):
        tt = torch.tensor(ts[i], dtype=torch.int64)
        xin = x.to(mdt)
        down = mid = None
        if controlnet is not None:
            down, mid = controlnet(xin, tt, encoder_hidden_states=ctx, controlnet_cond=control_image, return_dict=False)
        kw = {}
        if intrablock is not None:
            kw["down_intrablock_additional_residuals"] = [f.clone() for f in intrablock]
        eps = unet(xin, tt, encoder_hidden_states=ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid,
                   **kw).sample.double()
        z = x - lr
        m = (z - sg[i] * eps) / al[i]
        ms[i] = m
        zc = z
        if kind == "unipc" and i > first and i not in disable_corrector:
            p = order_prev
            h = lam[i] - lam[i - 1]
            phi1 = Bh = math.expm1(-h)
            rks = [(lam[i - 1 - k] - lam[i - 1]) / h for k in range(1, p)] + [1.0]
            rho = unipc_rhos(rks, h, p) if p > 1 else [0.5]
            res = rho[p - 1] * (m - ms[i - 1])
            for k in range(1, p):
                res = res + rho[k - 1] * (ms[i - 1 - k] - ms[i - 1]) / rks[k - 1]
            zc = (sg[i] / sg[i - 1]) * zc_prev - al[i] * phi1 * ms[i - 1] - al[i] * Bh * res
        # order of this predictor step
        p = min(solver_order, i - first + 1)
        if kind == "unipc":
            p = min(p, n - i)
        elif i == n - 1 and (n < 15 or final_sigmas_type == "zero"):
            p = 1
        if i == n - 1 and final_sigmas_type == "zero":
            zn = m  # sigma' = 0, alpha' = 1, e^-h = 0
        else:
            h = lam[i + 1] - lam[i]
            e1 = math.expm1(-h)
            zn = (sg[i + 1] / sg[i]) * zc - al[i + 1] * e1 * m
            if kind == "dpmsolver++" and p == 2:
                r0 = (lam[i] - lam[i - 1]) / h
                zn = zn - 0.5 * al[i + 1] * e1 * (m - ms[i - 1]) / r0
            elif kind == "unipc" and p > 1:
                rks = [(lam[i - k] - lam[i]) / h for k in range(1, p)] + [1.0]
                rho = unipc_rhos(rks, h, p - 1) if p > 2 else [0.5]
                res = 0.0
                for k in range(1, p):
                    res = res + rho[k - 1] * (ms[i - k] - m) / rks[k - 1]
                zn = zn - al[i + 1] * e1 * res
        zc_prev, order_prev = zc, p
        x = zn + lr
        traj.append(x.to(mdt))
    return traj


def apply_rows(rows, unet, x_T, timesteps, lr_latents=None, first=0, last=None, order=3):
    """Drive the folded coefficient rows of the host classes (``coefficient_rows``) exactly as the device kernel does - history ring
    indexed by the step, zeroed at the start - in float64.  Returns the states."""
    ts = [int(t) for t in timesteps]
    last = len(ts) if last is None else last
    lr = lr_latents.double() if lr_latents is not None else torch.zeros_like(x_T, dtype=torch.float64)
    x = x_T.double()
    hist = [torch.zeros_like(x) for _ in range(order)]
    xc = torch.zeros_like(x)
    traj = [x]
    for i in range(first, last):
        r = rows[i]
        eps = unet(x, torch.tensor(ts[i], dtype=torch.int64), encoder_hidden_states=None).sample.double()
        z = x - lr
        h = [hist[(i - k) % order] for k in (1, 2, 3)] if order == 3 else \
            [hist[(i - k) % order] if k <= order else torch.zeros_like(x) for k in (1, 2, 3)]
        m = r[0] * z + r[1] * eps
        zc = r[2] * z + r[3] * eps + r[4] * xc + r[5] * h[0] + r[6] * h[1] + r[7] * h[2]
        zn = r[8] * z + r[9] * eps + r[10] * xc + r[11] * h[0] + r[12] * h[1] + r[13] * h[2]
        hist[i % order] = m
        xc = zc
        x = zn + lr
        traj.append(x)
    return traj
