"""Host-side scheduler tables: the three members the reference touches - ``alphas_cumprod``
(``src/adapters/res_srdiff.py:13,60``), ``set_timesteps(n, device=)`` (``:53``), ``timesteps`` (``:54``) - with the
diffusers DDPM/DDIM table conventions (config keys nb ResDif c11:44-46).  Tiny, host-only; the
per-step arithmetic runs in the fused HIP step kernels driven by ``mrisr.pipeline``.

Every diffusers option that changes the table or the step is either implemented or refused: nothing is swallowed.
The reference's training config sets ``prediction_type="epsilon"``, ``timestep_spacing="trailing"`` and
``rescale_betas_zero_snr=True`` (nb ResDif c11:44-46)."""
from __future__ import annotations

import numpy as np
import torch

# options whose diffusers DEFAULT is what the fused step kernels implement; any other value raises
_FIXED = {
    "variance_type": ("fixed_small",),
    "clip_sample": (False,),          # x0 clipping is a Sampler argument (clip_sample_range), not scheduler state
    "thresholding": (False,),
    "set_alpha_to_one": (False,),     # the last DDIM step uses alphas_cumprod[0]
    "trained_betas": (None,),
    "dynamic_thresholding_ratio": (0.995,),
    "sample_max_value": (1.0,),
    "clip_sample_range": (1.0,),
}


def rescale_zero_terminal_snr(betas: torch.Tensor) -> torch.Tensor:
    """Lin et al. 2023 ("Common diffusion noise schedules and sample steps are flawed"), Algorithm 1 - what diffusers applies
    for ``rescale_betas_zero_snr=True``: shift sqrt(abar) so that the last entry is exactly 0, rescale so that the first is
    unchanged, and turn the result back into betas."""
    abar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    first, last = abar_sqrt[0].clone(), abar_sqrt[-1].clone()
    abar_sqrt = (abar_sqrt - last) * (first / (first - last))
    abar = abar_sqrt ** 2
    alphas = torch.cat([abar[0:1], abar[1:] / abar[:-1]])
    return 1.0 - alphas


class DDPMScheduler:
    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", timestep_spacing: str = "leading", steps_offset: int = 0,
                 prediction_type: str = "epsilon", rescale_betas_zero_snr: bool = False, **options):
        if prediction_type != "epsilon":
            raise ValueError("only epsilon prediction is used by the reference (nb ResDif c11:44)")
        for k, v in options.items():
            if k not in _FIXED:
                raise ValueError(f"unknown scheduler option {k!r}")
            if v not in _FIXED[k]:
                raise ValueError(f"scheduler option {k}={v!r} is not supported (the fused step implements {k}={_FIXED[k][0]!r})")
        self.num_train_timesteps = num_train_timesteps
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise ValueError(f"unknown beta_schedule {beta_schedule}")
        if rescale_betas_zero_snr:
            betas = rescale_zero_terminal_snr(betas)
        self.rescale_betas_zero_snr = bool(rescale_betas_zero_snr)
        self.betas = betas
        # with a zero terminal SNR the last entry is exactly 0: the forward shift (res_srdiff.py:13-25) is fine with that, the
        # reverse step divides by sqrt(abar_t) (:86) - the C sampler clamps abar_t to 2^-24 there
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        if timestep_spacing not in ("leading", "trailing"):
            raise ValueError(f"unknown timestep_spacing {timestep_spacing}")
        self.timestep_spacing = timestep_spacing
        self.steps_offset = steps_offset
        self.num_inference_steps = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1, dtype=torch.int64)

    def set_timesteps(self, num_inference_steps: int, device=None):
        T, n = self.num_train_timesteps, num_inference_steps
        if n > T:
            raise ValueError("num_inference_steps > num_train_timesteps")
        if self.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].astype(np.int64) + self.steps_offset
        else:  # "trailing"
            ts = np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(ts.copy())
        if device is not None:
            self.timesteps = self.timesteps.to(device)


class DDIMScheduler(DDPMScheduler):
    """eta = 0, set_alpha_to_one=False, no clipping - the sampler BASELINE.json names."""


# ------------------------------------------------------------------------------------------------------------------------------
# multistep solvers: UniPC (bh2) and DPM-Solver++ 2M (midpoint), data prediction
# ------------------------------------------------------------------------------------------------------------------------------
ABAR_MIN = 2.0 ** -24  # the clamp of the C sampler (mrisr_sampler_create): a zero-terminal-SNR table ends in abar = 0 exactly

# diffusers options of the two multistep schedulers whose stated value is the one implemented; any other value raises
_MULTISTEP_FIXED = {
    "thresholding": (False,), "dynamic_thresholding_ratio": (0.995,), "sample_max_value": (1.0,), "trained_betas": (None,),
    "lower_order_final": (True,), "use_karras_sigmas": (False,), "use_exponential_sigmas": (False,), "use_beta_sigmas": (False,),
    "use_flow_sigmas": (False,), "use_lu_lambdas": (False,), "euler_at_final": (False,), "variance_type": (None,),
    "lambda_min_clipped": (-float("inf"),), "solver_p": (None,), "rescale_betas_zero_snr": (False, True),
}


def _unipc_rho(rks, h, k):
    """rho of UniPC-bh2 (Zhao et al. 2023, data prediction): the leading k x k block of R rho = b; rows of R are
    [r_1 .. r_{p-1}, 1]^(j-1), b_j = (phi_{j+1}-recurrence value) j! / B(h), B(h) = expm1(-h)."""
    p, hh = len(rks), -h
    Bh = np.expm1(hh)
    phik, fact = np.expm1(hh) / hh - 1.0, 1.0
    R, b = [], []
    for j in range(1, p + 1):
        R.append(np.power(np.asarray(rks, dtype=np.float64), j - 1))
        b.append(phik * fact / Bh)
        fact *= j + 1
        phik = phik / hh - 1.0 / fact
    return np.linalg.solve(np.stack(R)[:k, :k], np.asarray(b)[:k])


class _MultistepScheduler(DDPMScheduler):
    """Shared part of ``UniPCMultistepScheduler`` / ``DPMSolverMultistepScheduler``: the DDPMScheduler tables and timestep grid, the
    solver options, and ``coefficient_rows`` - the folded per-step coefficients the fused HIP step kernel consumes.

    Parity status: diffusers is not available to this project, so these are the papers' algorithms (Lu et al. 2022, DPM-Solver++;
    Zhao et al. 2023, UniPC) on THIS project's timestep tables, not a bit-for-bit port.  In particular diffusers' UniPC derives its
    timesteps from interpolated sigmas; this one uses ``DDPMScheduler.set_timesteps`` ("leading" / "trailing")."""
    kind = None
    _max_order = 2

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", solver_order: int = 2, prediction_type: str = "epsilon",
                 timestep_spacing: str = "leading", steps_offset: int = 0, final_sigmas_type: str = "zero", **options):
        if prediction_type != "epsilon":
            raise ValueError("prediction_type: only epsilon prediction is implemented")
        own = self._own_options(options)
        for k, v in options.items():
            if k not in _MULTISTEP_FIXED:
                raise ValueError(f"unknown scheduler option {k!r}")
            if v not in _MULTISTEP_FIXED[k]:
                raise ValueError(f"scheduler option {k}={v!r} is not supported (implemented: {k}={_MULTISTEP_FIXED[k][0]!r})")
        if isinstance(solver_order, bool) or solver_order not in range(1, self._max_order + 1):
            raise ValueError(f"solver_order must be 1..{self._max_order} for {type(self).__name__}, got {solver_order!r}")
        if final_sigmas_type not in ("zero", "sigma_min"):
            raise ValueError(f"final_sigmas_type must be 'zero' or 'sigma_min', got {final_sigmas_type!r}")
        super().__init__(num_train_timesteps, beta_start, beta_end, beta_schedule, timestep_spacing, steps_offset, prediction_type,
                         bool(options.get("rescale_betas_zero_snr", False)))
        self.solver_order, self.final_sigmas_type, self.lower_order_final = int(solver_order), final_sigmas_type, True
        self.disable_corrector = []
        self.__dict__.update(own)

    def _own_options(self, options):
        return {}

    def grid(self):
        """(alpha, sigma, lambda) in float64 at t_0 > ... > t_{n-1} and at the final point (n + 1 entries): alpha = sqrt(abar),
        sigma = sqrt(1 - abar), lambda = log(alpha / sigma), abar clamped to 2^-24 as the C sampler does."""
        ts = self.timesteps.cpu().numpy().astype(np.int64)
        if len(ts) > 1 and not (np.diff(ts) < 0).all():
            raise ValueError("multistep solvers need strictly decreasing timesteps")
        ac = self.alphas_cumprod.to(torch.float32).double().numpy()
        abar = np.maximum(np.concatenate([ac[ts], ac[:1]]), ABAR_MIN)
        al, sg = np.sqrt(abar), np.sqrt(1.0 - abar)
        with np.errstate(divide="ignore"):
            lam = np.log(al / sg)
        if self.final_sigmas_type == "zero":
            al[-1], sg[-1], lam[-1] = 1.0, 0.0, np.inf
        return al, sg, lam

    def order_at(self, i: int, first: int = 0) -> int:
        """Order of the predictor step from t_i of a run that starts (cold) at step ``first``."""
        n = len(self.timesteps)
        p = min(self.solver_order, i - first + 1)
        if self.kind == "unipc":
            p = min(p, n - i)  # lower_order_final
        elif i == n - 1 and (n < 15 or self.final_sigmas_type == "zero"):
            p = 1  # diffusers' rule for n < 15; with the "zero" final point h is infinite and only the first-order step exists
        return max(p, 1)

    def corrector_at(self, i: int, first: int = 0) -> bool:
        return self.kind == "unipc" and i > first and i not in self.disable_corrector

    def coefficient_rows(self, first: int = 0) -> np.ndarray:
        """float64 [n, 16]; rows before ``first`` are zero.  With z = x - LR (or x), xc the previous corrected state and h_k the x0
        prediction k steps back, step i computes three linear forms of the raw inputs:

            m  (history slot i) = r[0] z + r[1] eps
            zc (corrected, UniPC) = r[2] z + r[3] eps + r[4] xc + r[5] h_1 + r[6] h_2 + r[7] h_3
            z' (next state)       = r[8] z + r[9] eps + r[10] xc + r[11] h_1 + r[12] h_2 + r[13] h_3

        Order schedule, the cold first step, disabled correctors and the final point are folded in: an absent term has a zero
        coefficient.  The C library builds the same rows (sampler.hip, build_multistep_rows) and rounds them to f32."""
        al, sg, lam = self.grid()
        n = len(self.timesteps)
        rows = np.zeros((n, 16), dtype=np.float64)
        for i in range(first, n):
            ma, mb = 1.0 / al[i], -sg[i] / al[i]
            c = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
            if self.corrector_at(i, first):
                p = self.order_at(i - 1, first)
                h = lam[i] - lam[i - 1]
                phi1 = Bh = np.expm1(-h)
                rks = [(lam[i - 1 - k] - lam[i - 1]) / h for k in range(1, p)] + [1.0]
                rho = _unipc_rho(rks, h, p) if p > 1 else np.array([0.5])
                cm = -al[i] * Bh * rho[p - 1]
                c = np.zeros(6)
                c[0], c[1], c[2] = cm * ma, cm * mb, sg[i] / sg[i - 1]
                c[3] = -al[i] * phi1 + al[i] * Bh * rho[p - 1]
                for k in range(1, p):
                    c[3 + k] = -al[i] * Bh * rho[k - 1] / rks[k - 1]
                    c[3] -= c[3 + k]
            p = self.order_at(i, first)
            ph = np.zeros(3)
            if i == n - 1 and self.final_sigmas_type == "zero":
                pz, pm = 0.0, 1.0
            else:
                h = lam[i + 1] - lam[i]
                e1 = np.expm1(-h)
                pz, pm = sg[i + 1] / sg[i], -al[i + 1] * e1
                if self.kind == "unipc" and p > 1:
                    rks = [(lam[i - k] - lam[i]) / h for k in range(1, p)] + [1.0]
                    rho = _unipc_rho(rks, h, p - 1) if p > 2 else np.array([0.5])
                    for k in range(1, p):
                        ph[k - 1] = -al[i + 1] * e1 * rho[k - 1] / rks[k - 1]
                elif self.kind == "dpmsolver++" and p > 1:
                    r0 = (lam[i] - lam[i - 1]) / h
                    ph[0] = 0.5 * al[i + 1] * e1 / r0
                pm -= ph.sum()
            rows[i, 0], rows[i, 1] = ma, mb
            rows[i, 2:8] = c
            rows[i, 8:14] = [pz * c[0] + pm * ma, pz * c[1] + pm * mb, pz * c[2], pz * c[3] + ph[0], pz * c[4] + ph[1], pz * c[5] + ph[2]]
        return rows


class UniPCMultistepScheduler(_MultistepScheduler):
    """UniPC (Zhao et al. 2023): predictor UniP-p and corrector UniC-p with the bh2 variant, data prediction, multistep.
    ``solver_order`` 1..3 (default 2), ``lower_order_final=True``, ``final_sigmas_type`` "zero" (diffusers' default) or
    "sigma_min", ``predict_x0=True``, ``solver_type="bh2"``, ``disable_corrector`` (list of step indices).  Every other diffusers
    option raises.  See ``_MultistepScheduler`` for the parity status."""
    kind = "unipc"
    _max_order = 3

    def _own_options(self, options):
        predict_x0 = options.pop("predict_x0", True)
        solver_type = options.pop("solver_type", "bh2")
        disable = options.pop("disable_corrector", [])
        if predict_x0 is not True:
            raise ValueError("predict_x0=False (noise prediction) is not implemented")
        if solver_type != "bh2":
            raise ValueError(f"solver_type={solver_type!r} is not implemented (UniPC here is the bh2 variant)")
        disable = [int(i) for i in disable]
        if any(i < 0 for i in disable):
            raise ValueError("disable_corrector: step indices must be >= 0")
        return {"predict_x0": True, "solver_type": "bh2", "disable_corrector": disable}


class DPMSolverMultistepScheduler(_MultistepScheduler):
    """DPM-Solver++ 2M (Lu et al. 2022): multistep, data prediction, midpoint second-order term.  ``solver_order`` 1..2 (default 2),
    ``algorithm_type="dpmsolver++"``, ``solver_type="midpoint"``, ``lower_order_final=True`` (first order on the last step when
    n < 15, and always with the "zero" final point), ``final_sigmas_type`` "zero" or "sigma_min".  Every other diffusers option
    raises (SDE variants, heun, Karras sigmas, ...).  At order 1 this is DDIM term for term.  See ``_MultistepScheduler`` for the
    parity status."""
    kind = "dpmsolver++"
    _max_order = 2

    def _own_options(self, options):
        algorithm_type = options.pop("algorithm_type", "dpmsolver++")
        solver_type = options.pop("solver_type", "midpoint")
        if algorithm_type != "dpmsolver++":
            raise ValueError(f"algorithm_type={algorithm_type!r} is not implemented (only the deterministic dpmsolver++)")
        if solver_type != "midpoint":
            raise ValueError(f"solver_type={solver_type!r} is not implemented (only midpoint)")
        return {"algorithm_type": "dpmsolver++", "solver_type": "midpoint"}
