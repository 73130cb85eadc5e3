"""Reference for classifier-free guidance, shared by test_guidance_cpu.py (which checks THIS file on the CPU) and
test_gpu_guidance.py (which checks the device sampler against it).  No new oracle code: the oracle's sampler loops take the UNet and
the ControlNet as callables, so guidance is two small wrappers around ``oracle.unet.OracleUNet`` / ``OracleControlNet`` that
evaluate the network with the unconditional and with the conditional context and combine the two predictions:

    e = eps_u + g (eps_c - eps_u)
    phi > 0:  e = e (phi std(eps_c) / std(e) + (1 - phi))      torch.std over (C, h, w) of every sample, unbiased

(Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", sec. 3.4; diffusers' ``rescale_noise_cfg``)."""
import torch


def guided_eps(eps_u, eps_c, g, phi):
    e = eps_u + g * (eps_c - eps_u)
    if phi > 0:
        e = e * (phi * eps_c.std(dim=(1, 2, 3), keepdim=True) / e.std(dim=(1, 2, 3), keepdim=True) + (1 - phi))
    return e


class _Out:
    def __init__(self, sample):
        self.sample = sample


class GuidedControlNet:
    """ControlNet residuals per context: returns ((down_u, down_c), (mid_u, mid_c)), which only ``GuidedUNet`` understands.  The
    loops hand them through untouched.  Both halves see the same condition image (diffusers' default, not guess mode)."""

    def __init__(self, controlnet, ctx_u, ctx_c):
        self.controlnet, self.ctx_u, self.ctx_c = controlnet, ctx_u, ctx_c

    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, return_dict=False):
        du, mu = self.controlnet(sample, timestep, encoder_hidden_states=self.ctx_u, controlnet_cond=controlnet_cond, return_dict=False)
        dc, mc = self.controlnet(sample, timestep, encoder_hidden_states=self.ctx_c, controlnet_cond=controlnet_cond, return_dict=False)
        return (du, dc), (mu, mc)


class GuidedUNet:
    """``unet`` evaluated with ``ctx_u`` and with ``ctx_c`` (the loop's own ``encoder_hidden_states`` is ignored); ``.sample`` is the
    guided prediction.  ``last`` keeps (eps_u, eps_c, e) of the latest call."""

    def __init__(self, unet, ctx_u, ctx_c, guidance_scale, guidance_rescale=0.0):
        self.unet, self.ctx_u, self.ctx_c = unet, ctx_u, ctx_c
        self.g, self.phi = float(guidance_scale), float(guidance_rescale)
        self.last = None

    def __call__(self, sample, timestep, encoder_hidden_states=None, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, down_intrablock_additional_residuals=None):
        down, mid = down_block_additional_residuals, mid_block_additional_residual
        eps = []
        for k, ctx in enumerate((self.ctx_u, self.ctx_c)):
            kw = {}
            if down is not None:
                kw = dict(down_block_additional_residuals=down[k], mid_block_additional_residual=mid[k])
            if down_intrablock_additional_residuals is not None:  # the UNet adds into its skip list in place: a fresh copy per call
                kw["down_intrablock_additional_residuals"] = [f.clone() for f in down_intrablock_additional_residuals]
            eps.append(self.unet(sample, timestep, encoder_hidden_states=ctx, **kw).sample)
        e = guided_eps(eps[0], eps[1], self.g, self.phi)
        self.last = (eps[0], eps[1], e)
        return _Out(e)
