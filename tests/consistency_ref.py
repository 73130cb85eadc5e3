"""Reference for low-frequency consistency in the graph sampler (ILVR), shared by test_consistency_cpu.py (which
checks THIS file and ``mrisr.consistency_schedule`` on the CPU), test_gpu_consistency_ops.py (the kernel alone) and
test_gpu_consistency.py (the device sampler).  No new oracle code: the loops below are the oracle's own step functions
(``OracleScheduler.ddim_step`` / ``ddpm_step``, ``oracle.sampler.res_shift_reverse_step``, ``multistep_ref.multistep_sample``) with one
hook after every step; guidance, PAG, tiles and the table wrappers go around the networks as in the other *_ref files.

    phi(d, N, filter)   F.interpolate(F.avg_pool2d(d, N), scale_factor=N, mode=filter[, align_corners=False]) in float64
    apply(...)          x + w phi(alpha ref + beta lr + sigma z - x)
    rows(...)           {w, alpha, beta, sigma} per step from the ORACLE scheduler's tables: a_p is the cumulative alpha of the state the
                        step produces, read off the step rule of each kind, independently of ``mrisr.consistency_schedule``"""
import numpy as np
import torch
import torch.nn.functional as F

import multistep_ref as mref


def phi(d, N, filter="bilinear"):
    """The low-pass filter: mean over N x N blocks, upsampled by N.  float64 in, float64 out."""
    p = F.avg_pool2d(d.double(), N)
    if filter == "nearest":
        return F.interpolate(p, scale_factor=N, mode="nearest")
    assert filter == "bilinear"
    return F.interpolate(p, scale_factor=N, mode="bilinear", align_corners=False)


def target(ref, lr, z, row):
    """y = alpha ref + beta lr + sigma z in float64; a missing lr or z contributes 0; z is not read at sigma == 0."""
    _, al, be, sg = (float(v) for v in row)
    y = al * ref.double()
    if lr is not None:
        y = y + be * lr.double()
    if z is not None and sg != 0.0:
        y = y + sg * z.double()
    return y


def apply(x, ref, lr, z, row, N, filter="bilinear"):
    """One consistency update in float64.  A row with w == 0 returns x itself, whatever ref and z hold."""
    w = float(row[0])
    if w == 0.0:
        return x.double()
    return x.double() + w * phi(target(ref, lr, z, row) - x.double(), N, filter)


def inside(i, n, start, end):
    return i / n >= start and (i + 1) / n <= end


def produced_alphas(kind, so, final_sigmas_type="zero"):
    """a_p(i) for every step of the oracle scheduler ``so``: the cumulative alpha of the state step i produces, from the step rule of
    ``kind`` itself (``ddim_step`` / ``ddpm_step``: t - T // n, below zero alphas_cumprod[0] / 1; the Res-SRDiff loop: the next timestep,
    at the end alphas_cumprod[0]; the multistep grid of ``multistep_ref``)."""
    ts = [int(t) for t in so.timesteps]
    ac = so.alphas_cumprod.double()
    n = len(ts)
    if kind in ("unipc", "dpmsolver++"):
        _, al, _, _ = mref.grid(ts, so.alphas_cumprod, final_sigmas_type)
        return [float(al[i + 1] ** 2) for i in range(n)]
    out = []
    for i, t in enumerate(ts):
        if kind == "resshift":
            out.append(float(ac[ts[i + 1] if i + 1 < n else 0]))
        else:
            tp = t - so.num_train_timesteps // n
            out.append(float(ac[tp]) if tp >= 0 else (1.0 if kind == "ddpm" else float(ac[0])))
    return out


def rows(kind, so, anchored, weight=1.0, interval=(0.0, 1.0), noisy=False, final_sigmas_type="zero"):
    """[n, 4] float32 rows {w, sqrt(a_p), 1 - sqrt(a_p) if anchored, sqrt(1 - a_p) if noisy}; w = weight inside the interval, else 0."""
    ap = produced_alphas(kind, so, final_sigmas_type)
    n = len(ap)
    out = np.zeros((n, 4), dtype=np.float32)
    for i, a in enumerate(ap):
        out[i] = (weight if inside(i, n, *interval) else 0.0, a ** 0.5, 1.0 - a ** 0.5 if anchored else 0.0, (1.0 - a) ** 0.5 if noisy else 0.0)
    return out


def make_hook(table, ref, N, filter="bilinear", lr=None, noise=None):
    """hook(i, x): the state after step i (an absolute index, like the rows) -> the consistent state, in x's dtype."""
    def hook(i, x):
        return apply(x, ref, lr, noise[i] if noise is not None else None, table[i], N, filter).to(x.dtype)
    return hook


def first_order_sample(kind, unet, x_T, ctx, so, hook=None, lr_latents=None, step_noise=None, controlnet=None, control_image=None,
                       intrablock=None, first=0, last=None):
    """States [x_first, ..., x_last] of "ddim" / "ddpm" / "resshift" on the oracle scheduler ``so``, ``hook`` applied after every step.
    ``step_noise[i]`` is the draw of step i ("resshift": of the i-th stochastic step, as ``res_srdiff_sample`` counts them)."""
    from oracle import sampler as osa
    ts = so.timesteps.tolist()
    last = len(ts) if last is None else last
    x = x_T
    traj = [x]
    k = sum(1 for i in range(first) if (ts[i + 1] if i + 1 < len(ts) else 0) > 0)
    for i in range(first, last):
        t = ts[i]
        tt = torch.tensor(t, dtype=torch.int64)
        down = mid = None
        if controlnet is not None:
            down, mid = controlnet(x, tt, encoder_hidden_states=ctx, controlnet_cond=control_image, return_dict=False)
        kw = {}
        if intrablock is not None:
            kw["down_intrablock_additional_residuals"] = [f.clone() for f in intrablock]
        eps = unet(x, tt, encoder_hidden_states=ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid, **kw).sample
        if kind == "ddim":
            x = so.ddim_step(eps, t, x)
        elif kind == "ddpm":
            x = so.ddpm_step(eps, t, x, step_noise[i] if step_noise is not None else None)
        else:
            assert kind == "resshift"
            prev_t = ts[i + 1] if i + 1 < len(ts) else 0
            ac = so.alphas_cumprod
            nz = None
            if prev_t > 0:
                nz = step_noise[k]
                k += 1
            x = osa.res_shift_reverse_step(x, eps, lr_latents, ac[t].to(x.dtype), ac[prev_t].to(x.dtype), nz)
        if hook is not None:
            x = hook(i, x)
        traj.append(x)
    return traj


class _HookedAnchor:
    """Stands in for ``lr_latents`` in ``multistep_ref.multistep_sample``, whose loop touches the anchor in exactly two places per step:
    ``z = x - lr`` at its start and ``x = zn + lr`` at its end.  The second is where the step's state is formed, so that is where the
    hook goes: the loop itself stays the reference's, nothing of it is restated here."""

    def __init__(self, lr, hook, first):
        self.lr, self.hook, self.i = lr, hook, first

    def double(self):
        return self

    def __rsub__(self, x):
        return x - self.lr

    def __radd__(self, zn):
        x = self.hook(self.i, zn + self.lr)
        self.i += 1
        return x


def multistep_sample(kind, unet, x_T, ctx, timesteps, alphas_cumprod, hook=None, lr_latents=None, first=0, **kw):
    """``multistep_ref.multistep_sample`` with ``hook`` applied to the state every step forms (the solver's history and corrected state
    are what the step computed; the next step starts from the consistent state)."""
    if hook is None:
        return mref.multistep_sample(kind, unet, x_T, ctx, timesteps, alphas_cumprod, lr_latents=lr_latents, first=first, **kw)
    lr = lr_latents.double() if lr_latents is not None else torch.zeros_like(x_T, dtype=torch.float64)
    return mref.multistep_sample(kind, unet, x_T, ctx, timesteps, alphas_cumprod, lr_latents=_HookedAnchor(lr, hook, first), first=first, **kw)
