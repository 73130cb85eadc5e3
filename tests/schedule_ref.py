"""Reference for per-step schedules of the guidance and FreeU strengths, shared by test_schedule_cpu.py (which
checks THIS file on the CPU against the constant-strength wrappers) and test_gpu_schedule.py (which checks the device sampler against
it).  No new oracle code and no new formula: ``ScheduledUNet`` wraps the CPU oracle UNet like ``GuidedUNet`` (guidance_ref.py) and
``PagUNet`` (pag_ref.py) do, and call i of a sampler loop combines its parts with ROW i of a schedule table

    row = { g, s, phi, freeu_s1, freeu_s2, freeu_b1, freeu_b2, 0 }

through ``guided_eps`` / ``pag_eps`` of those files; with ``freeu=True`` the forwards of call i run under ``freeu_ref.freeu`` with the
row's four values.  The run kind is fixed by the constructor, as the device's is by the entry point called:

    mode "plain":    e = eps_c                                     (g, s, phi are not read)
    mode "cfg":      e = guided_eps(eps_u, eps_c, g, phi)
    mode "pag":      e = pag_eps(eps_p, None, eps_c, -, s, phi)    (g is not read)
    mode "pag+cfg":  e = pag_eps(eps_p, eps_u, eps_c, g, s, phi)

The oracle loops call the network once per step, in order, so the call counter is the step index; ``first`` is the step the run
starts at (``Sampler.set_range``)."""
import contextlib

import numpy as np

import freeu_ref as fr
from guidance_ref import guided_eps
from pag_ref import pag_eps, perturbed_attention

NEUTRAL = (1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0)


def constant_rows(n, g=1.0, s=0.0, phi=0.0, freeu=(1.0, 1.0, 1.0, 1.0)):
    """[n, 8] float32: the same row for every step."""
    return np.tile(np.asarray((g, s, phi) + tuple(freeu) + (0.0,), dtype=np.float32), (n, 1))


def inside(i, n, lo, hi):
    """diffusers' control_guidance_start / control_guidance_end rule: step i of n lies inside (lo, hi)."""
    return i / n >= lo and (i + 1) / n <= hi


class _Out:
    def __init__(self, sample):
        self.sample = sample


class ScheduledUNet:
    """``unet`` evaluated as the run kind ``mode`` needs, call i combined with ``rows[first + i]``.  ``calls`` counts the calls,
    ``used`` keeps the rows they read."""

    def __init__(self, unet, rows, mode, ctx_c, ctx_u=None, layers=(), freeu=False, cfg=None, first=0):
        assert mode in ("plain", "cfg", "pag", "pag+cfg")
        assert ("cfg" in mode) == (ctx_u is not None) and (not freeu or cfg is not None)
        self.unet, self.rows, self.mode = unet, np.asarray(rows, dtype=np.float32), mode
        self.ctx_c, self.ctx_u, self.layers = ctx_c, ctx_u, tuple(layers)
        self.freeu, self.cfg, self.first = freeu, cfg, first
        self.calls, self.used = 0, []

    def _call(self, sample, timestep, ctx, down, mid, intra):
        kw = {}
        if down is not None:
            kw = dict(down_block_additional_residuals=down, mid_block_additional_residual=mid)
        if intra is not None:
            kw["down_intrablock_additional_residuals"] = [f.clone() for f in intra]
        return self.unet(sample, timestep, encoder_hidden_states=ctx, **kw).sample

    def __call__(self, sample, timestep, encoder_hidden_states=None, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, down_intrablock_additional_residuals=None):
        down, mid, intra = down_block_additional_residuals, mid_block_additional_residual, down_intrablock_additional_residuals
        row = [float(v) for v in self.rows[self.first + self.calls]]
        self.calls += 1
        self.used.append(row)
        g, s, phi, s1, s2, b1, b2 = row[:7]
        scope = fr.freeu(s1, s2, b1, b2, self.cfg) if self.freeu else contextlib.nullcontext()
        with scope:
            eps_c = self._call(sample, timestep, self.ctx_c, down, mid, intra)
            eps_u = self._call(sample, timestep, self.ctx_u, down, mid, intra) if "cfg" in self.mode else None
            eps_p = None
            if "pag" in self.mode:
                with perturbed_attention(self.layers):
                    eps_p = self._call(sample, timestep, self.ctx_c, down, mid, intra)
        if self.mode == "plain":
            e = eps_c
        elif self.mode == "cfg":
            e = guided_eps(eps_u, eps_c, g, phi)
        else:
            e = pag_eps(eps_p, eps_u, eps_c, g, s, phi).to(sample.dtype)
        return _Out(e)
