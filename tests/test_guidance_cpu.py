"""CPU: classifier-free guidance - the argument rules of ``Sampler.run`` / ``fit`` (checked on shapes, before a device is touched)
and the reference the GPU tests compare against (tests/guidance_ref.py), so that a wrong reference cannot pass unnoticed there."""
import pytest
import torch

from guidance_ref import GuidedControlNet, GuidedUNet, guided_eps

torch.set_grad_enabled(False)


def test_check_guidance_rules():
    import mrisr
    chk = mrisr.check_guidance
    ehs, B = (2, 77, 64), 2
    # off: nothing asked for, or g == 1 with an unconditional context (the conditional prediction: the plain call is taken)
    assert chk(1.0, 0.0, ehs, None, B) is False
    assert chk(1.0, 0.0, ehs, (1, 77, 64), B) is False
    # on
    assert chk(3.0, 0.0, ehs, (1, 77, 64), B) is True
    assert chk(7.5, 0.7, (1, 77, 64), (2, 77, 64), B) is True
    assert chk(0.0, 1.0, ehs, ehs, B) is True
    for bad in (dict(g=3.0, phi=0.0, u=None),                  # a scale without the unconditional context
                dict(g=3.0, phi=-0.1, u=(1, 77, 64)),          # rescale outside [0, 1]
                dict(g=3.0, phi=1.5, u=(1, 77, 64)),
                dict(g=1.0, phi=0.5, u=None),                  # rescale without active guidance
                dict(g=1.0, phi=0.5, u=(1, 77, 64)),
                dict(g=3.0, phi=0.0, u=(1, 76, 64)),           # other L
                dict(g=3.0, phi=0.0, u=(1, 77, 32)),           # other D
                dict(g=3.0, phi=0.0, u=(3, 77, 64)),           # neither 1 nor B rows
                dict(g=3.0, phi=0.0, u=(77, 64)),              # rank
                dict(g=float("nan"), phi=0.0, u=(1, 77, 64))):
        with pytest.raises(ValueError):
            chk(bad["g"], bad["phi"], ehs, bad["u"], B)
    with pytest.raises(ValueError):
        chk(3.0, 0.0, (3, 77, 64), (1, 77, 64), B)  # the conditional context does not expand to the batch either


def test_fit_validation_guidance_rules():
    from mrisr.fit import check_validation_guidance
    emb = {"": torch.zeros(77, 64), "a scan": torch.ones(77, 64)}
    assert check_validation_guidance(1.0, 0.0, emb) is False
    assert check_validation_guidance(1.0, 0.0, {"a scan": emb["a scan"]}) is False
    assert check_validation_guidance(3.0, 0.7, emb) is True
    with pytest.raises(ValueError, match="validation_guidance_scale"):
        check_validation_guidance(3.0, 0.0, {"a scan": emb["a scan"]})
    with pytest.raises(ValueError):
        check_validation_guidance(3.0, 1.2, emb)
    with pytest.raises(ValueError):
        check_validation_guidance(1.0, 0.5, emb)
    # fit() itself refuses before any GPU work: no model, no device needed to get the error
    import mrisr
    with pytest.raises(ValueError, match="validation_guidance_scale"):
        mrisr.fit(mrisr.TrainConfig(proportion_empty_prompts=0.0), None, None, None, {"a scan": emb["a scan"]}, validation_guidance_scale=2.0)
    # trailing keyword arguments only: the reference's call expressions keep binding as before
    import inspect
    names = list(inspect.signature(mrisr.log_validation).parameters)
    assert names[-3:] == ["guidance_scale", "guidance_rescale", "uncond_embeds"] and names[:10] == [
        "unet", "controlnet", "vae", "val_dataloader", "noise_scheduler", "weight_dtype", "accelerator", "fixed_embeds",
        "num_inference_steps", "adapter"]
    names = list(inspect.signature(mrisr.Sampler.run).parameters)
    assert names[-3:] == ["guidance_scale", "guidance_rescale", "uncond_hidden_states"] and names[-4] == "use_graph"


def test_guided_eps_formulae():
    g = torch.Generator().manual_seed(11)
    eu, ec = torch.randn((3, 4, 8, 8), generator=g, dtype=torch.float64), 1.7 * torch.randn((3, 4, 8, 8), generator=g, dtype=torch.float64)
    assert torch.equal(guided_eps(eu, ec, 0.0, 0.0), eu)
    assert torch.allclose(guided_eps(eu, ec, 1.0, 0.0), ec, rtol=0, atol=1e-15)
    assert torch.allclose(guided_eps(eu, ec, 7.5, 0.0), 7.5 * ec - 6.5 * eu, rtol=0, atol=1e-12)
    # phi = 1: every sample of the guided prediction has the standard deviation of the conditional one (unbiased, per sample)
    for gs in (0.0, 3.5, 7.5):
        e = guided_eps(eu, ec, gs, 1.0)
        assert torch.allclose(e.std(dim=(1, 2, 3)), ec.std(dim=(1, 2, 3)), rtol=1e-12, atol=0)
        # ... and the same direction as the unrescaled one
        plain = guided_eps(eu, ec, gs, 0.0)
        assert torch.allclose(e / e.flatten(1).norm(dim=1).view(-1, 1, 1, 1), plain / plain.flatten(1).norm(dim=1).view(-1, 1, 1, 1), atol=1e-12)
    # phi in between interpolates the factor linearly
    f1 = ec.std(dim=(1, 2, 3), keepdim=True) / guided_eps(eu, ec, 3.5, 0.0).std(dim=(1, 2, 3), keepdim=True)
    assert torch.allclose(guided_eps(eu, ec, 3.5, 0.7), guided_eps(eu, ec, 3.5, 0.0) * (0.7 * f1 + 0.3), rtol=1e-12, atol=0)
    # per SAMPLE: changing sample 1 leaves sample 0 alone
    ec2 = ec.clone()
    ec2[1] *= 5.0
    assert torch.equal(guided_eps(eu, ec2, 3.5, 0.7)[0], guided_eps(eu, ec, 3.5, 0.7)[0])
    assert not torch.equal(guided_eps(eu, ec2, 3.5, 0.7)[1], guided_eps(eu, ec, 3.5, 0.7)[1])


@pytest.fixture(scope="module")
def tiny_oracle():
    from oracle import unet as ou
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=2101, perturb_norm=True)
    up.update(ou.init_lora_params(up, rank=4, seed=2103))
    cp = ou.init_controlnet_params(cfg, seed=2102, perturb_norm=True)
    g = torch.Generator().manual_seed(2105)
    x = torch.randn((2, 4, 8, 8), generator=g)
    ctx_c = torch.randn((2, 77, cfg.cross_attention_dim), generator=g)
    ctx_u = torch.randn((1, 77, cfg.cross_attention_dim), generator=g).expand(2, -1, -1).contiguous()
    cond = torch.randn((2, 3, 64, 64), generator=g)
    return cfg, ou.OracleUNet(up, cfg), ou.OracleControlNet(cp, cfg), x, ctx_u, ctx_c, cond


def test_wrapped_oracle_at_scale_one_is_the_plain_oracle_loop(tiny_oracle):
    """g = 1, phi = 0: the wrapped loop (which ignores the loop's own context) reproduces the plain loop run with the conditional
    context, for the DDIM loop with ControlNet residuals and for the Res-SRDiff loop: the wrappers route the right context and the
    right residuals to the right half."""
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, unet, cnet, x, ctx_u, ctx_c, cond = tiny_oracle
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(3)
    plain = osa.ddim_sample(unet, x, ctx_c, so, controlnet=cnet, control_image=cond)
    wrapped = osa.ddim_sample(GuidedUNet(unet, ctx_u, ctx_c, 1.0), x, None, so, controlnet=GuidedControlNet(cnet, ctx_u, ctx_c),
                              control_image=cond)
    for a, b in zip(wrapped, plain):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    # g = 0 is the plain loop with the UNCONDITIONAL context (the halves are not swapped)
    plain_u = osa.ddim_sample(unet, x, ctx_u, so, controlnet=cnet, control_image=cond)
    wrapped_u = osa.ddim_sample(GuidedUNet(unet, ctx_u, ctx_c, 0.0), x, None, so, controlnet=GuidedControlNet(cnet, ctx_u, ctx_c),
                                control_image=cond)
    assert torch.allclose(wrapped_u[-1], plain_u[-1], rtol=1e-5, atol=1e-6)
    assert not torch.allclose(plain_u[-1], plain[-1], rtol=1e-3, atol=1e-4)  # the two contexts do give different trajectories
    g = torch.Generator().manual_seed(2107)
    lr = 0.2 * torch.randn((2, 4, 8, 8), generator=g)
    n0, zs = torch.randn((2, 4, 8, 8), generator=g), [torch.randn((2, 4, 8, 8), generator=g) for _ in range(2)]
    plain = osa.res_srdiff_sample(unet, None, lr, ctx_c, None, so.timesteps, so.alphas_cumprod, n0, zs)
    wrapped = osa.res_srdiff_sample(GuidedUNet(unet, ctx_u, ctx_c, 1.0), None, lr, None, None, so.timesteps, so.alphas_cumprod, n0, zs)
    for a, b in zip(wrapped, plain):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_wrapped_oracle_rescale_gives_the_conditional_std(tiny_oracle):
    cfg, unet, cnet, x, ctx_u, ctx_c, cond = tiny_oracle
    w = GuidedUNet(unet, ctx_u, ctx_c, 5.0, 1.0)
    e = w(x, torch.tensor(601)).sample
    eu, ec, e_last = w.last
    assert e is e_last
    assert torch.allclose(e.std(dim=(1, 2, 3)), ec.std(dim=(1, 2, 3)), rtol=1e-5, atol=0)
    assert torch.allclose(eu, unet(x, torch.tensor(601), encoder_hidden_states=ctx_u).sample, rtol=1e-5, atol=1e-6)
    assert torch.allclose(ec, unet(x, torch.tensor(601), encoder_hidden_states=ctx_c).sample, rtol=1e-5, atol=1e-6)
    # without the rescale the guided prediction is wider than the conditional one here (what the rescale is for)
    w0 = GuidedUNet(unet, ctx_u, ctx_c, 5.0, 0.0)
    assert bool((w0(x, torch.tensor(601)).sample.std(dim=(1, 2, 3)) > ec.std(dim=(1, 2, 3))).all())
