"""Reference for the conditioning strength of the graph sampler, shared by test_condctl_cpu.py (which checks THIS
file on the CPU) and test_gpu_condctl.py (which checks the device sampler against it).  No new oracle code: like guidance_ref.py and
schedule_ref.py, two small wrappers around ``oracle.unet.OracleControlNet`` / ``OracleUNet``.  The oracle loops call each network once
per step, in order, so the call counter is the step index; ``first`` is the step the run starts at (``Sampler.set_range``).

    ScaledControlNet   on call i, residual k (the mid residual last) is multiplied by  w_k * c_i,   c_i = rows[first + i][0]
    ScaledAdapterUNet  on call i, every intrablock feature is multiplied by            a_i,         a_i = rows[first + i][1]

``w_k`` is 1, or in guess mode diffusers' ``logspace(-1, 0, n_down + 1)[k]`` (``ControlNetModel.forward``).  In guess mode under
classifier-free guidance (``ctx_c`` given) the ControlNet is evaluated with the conditional context only and the wrapper returns
``((zeros, d_c), (zeros, m_c))`` - diffusers' ``cat([zeros_like(d), d])`` - which ``guidance_ref.GuidedUNet`` hands to its two halves.

The two table rules are restated here independently of ``mrisr`` (diffusers is not installed: the formulae are the specification)."""
import numpy as np
import torch


def inside(i, n, start, end):
    """diffusers' ``controlnet_keep``: step i of n keeps the ControlNet iff i / n >= start and (i + 1) / n <= end."""
    return i / n >= start and (i + 1) / n <= end


def table(n, c=1.0, start=0.0, end=1.0, a=1.0, factor=1.0):
    """[n, 4] float32 rows {c_i, a_i, 0, 0}: c inside (start, end) else 0; a on the first int(n * factor) steps else 0."""
    rows = np.zeros((n, 4), dtype=np.float32)
    for i in range(n):
        rows[i, 0] = c if inside(i, n, start, end) else 0.0
        rows[i, 1] = a if i < int(n * factor) else 0.0
    return rows


def constant_rows(n, c=1.0, a=1.0):
    return np.tile(np.asarray((c, a, 0.0, 0.0), dtype=np.float32), (n, 1))


def guess_weights(n_down):
    """float32 logspace(-1, 0, n_down + 1): the down residuals, then the mid residual at 1."""
    return torch.logspace(-1.0, 0.0, n_down + 1, dtype=torch.float64).to(torch.float32)


class ScaledControlNet:
    """``controlnet`` with residual k of call i scaled by w_k * rows[first + i][0].  ``ctx_c``: guess mode under guidance - evaluate with
    that context and return the pair form for ``GuidedUNet``.  ``calls`` counts the calls, ``used`` keeps the c values they read."""

    def __init__(self, controlnet, rows, guess=False, ctx_c=None, first=0):
        self.controlnet, self.rows, self.guess, self.ctx_c, self.first = controlnet, np.asarray(rows, dtype=np.float32), guess, ctx_c, first
        self.calls, self.used = 0, []

    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, return_dict=False):
        c = torch.tensor(self.rows[self.first + self.calls, 0])  # f32, as the device reads it
        self.calls += 1
        self.used.append(float(c))
        ctx = self.ctx_c if self.ctx_c is not None else encoder_hidden_states
        down, mid = self.controlnet(sample, timestep, encoder_hidden_states=ctx, controlnet_cond=controlnet_cond, return_dict=False)

        def scaled(down, mid):
            w = guess_weights(len(down)) if self.guess else torch.ones(len(down) + 1)
            return [d * (w[k] * c) for k, d in enumerate(down)], mid * (w[len(down)] * c)
        if isinstance(down, tuple) and len(down) == 2 and isinstance(down[0], (list, tuple)):  # GuidedControlNet's pair: both halves
            assert self.ctx_c is None
            (du, mu), (dc, mc) = scaled(down[0], mid[0]), scaled(down[1], mid[1])
            return (du, dc), (mu, mc)
        down, mid = scaled(down, mid)
        if self.ctx_c is not None:
            return ([torch.zeros_like(d) for d in down], down), (torch.zeros_like(mid), mid)
        return down, mid


class _Out:
    def __init__(self, sample):
        self.sample = sample


class ScaledAdapterUNet:
    """``unet`` (an oracle UNet or a wrapper of one) with the intrablock features of call i multiplied by rows[first + i][1]."""

    def __init__(self, unet, rows, first=0):
        self.unet, self.rows, self.first = unet, np.asarray(rows, dtype=np.float32), first
        self.calls, self.used = 0, []

    def __call__(self, sample, timestep, encoder_hidden_states=None, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, down_intrablock_additional_residuals=None):
        a = torch.tensor(self.rows[self.first + self.calls, 1])
        self.calls += 1
        self.used.append(float(a))
        kw = {}
        if down_block_additional_residuals is not None:
            kw = dict(down_block_additional_residuals=down_block_additional_residuals, mid_block_additional_residual=mid_block_additional_residual)
        if down_intrablock_additional_residuals is not None:
            kw["down_intrablock_additional_residuals"] = [f * a for f in down_intrablock_additional_residuals]
        return _Out(self.unet(sample, timestep, encoder_hidden_states=encoder_hidden_states, **kw).sample)
