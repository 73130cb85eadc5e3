"""CPU: perturbed-attention guidance - the argument rules of ``Sampler.run(pag_scale=, pag_applied_layers=)`` (``check_pag``: numbers
and names alone, before a device is touched), the prefix -> block-mask resolution, and the reference the GPU tests compare against
(tests/pag_ref.py), so that a wrong reference cannot pass unnoticed there."""
import os
import re

import pytest
import torch

from guidance_ref import guided_eps
from pag_ref import PagUNet, block_names, mask_of, pag_eps, perturbed_attention

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-12))


def test_block_names_tiny_and_sd15():
    import mrisr
    from oracle import unet as ou
    for cfg in (ou.TINY, ou.SD15):
        names = mrisr.transformer_block_names(cfg)
        assert names == block_names(cfg) and len(names) == 16
        assert names[:2] == ["down_blocks.0.attentions.0", "down_blocks.0.attentions.1"]
        assert names[6] == "mid_block.attentions.0"
        assert names[7] == "up_blocks.1.attentions.0" and names[-1] == "up_blocks.3.attentions.2"
    assert mrisr.transformer_block_names(mrisr.UNetConfig()) == block_names(ou.SD15)


def test_check_pag_accepts_and_resolves_prefixes():
    import mrisr
    from oracle import unet as ou
    chk = mrisr.check_pag
    for cfg in (ou.TINY, ou.SD15):
        names = mrisr.transformer_block_names(cfg)
        assert chk(0.0, ("mid",), names) == 0                       # off: the plain call
        assert chk(0, ("mid",), names, has_cache=True, fp8_attention=True) == 0  # off means off, whatever else is set
        assert chk(0.0, (), names) == 0
        assert chk(3.0, ("mid",), names) == 1 << 6
        assert chk(3.0, "mid", names) == 1 << 6                     # a bare string is one prefix
        assert chk(3.0, ("mid_block",), names) == 1 << 6
        assert chk(3.0, ("mid_block.attentions.0",), names) == 1 << 6
        assert chk(1.0, ("down_blocks.0",), names) == 0b11
        assert chk(1.0, ("down_blocks.2",), names) == 0b110000
        assert chk(1.0, ("up_blocks.1.attentions.0",), names) == 1 << 7
        assert chk(1.0, ("up_blocks.3",), names) == 0b111 << 13
        assert chk(1.0, ("down_blocks.0", "up_blocks.3"), names) == 0b11 | (0b111 << 13)
        assert chk(0.5, ("down_blocks", "mid", "up_blocks"), names) == (1 << 16) - 1
        assert chk(0.5, ("up_blocks.3", "up_blocks.3.attentions.1"), names) == 0b111 << 13  # overlapping entries
        for layers in (("mid",), ("down_blocks.0", "up_blocks.3"), ("down_blocks", "mid", "up_blocks")):
            assert chk(1.0, layers, names) == mask_of(layers, block_names(cfg))


def test_check_pag_refusals_name_the_argument():
    import mrisr
    from oracle import unet as ou
    chk = mrisr.check_pag
    names = mrisr.transformer_block_names(ou.TINY)
    for bad in (-1.0, -1e-9, float("nan"), float("inf"), -float("inf"), "three", None, True):
        with pytest.raises(ValueError, match="pag_scale"):
            chk(bad, ("mid",), names)
    for layers in (("down_blocks.3",),            # the attention-free level has no transformer block
                   ("up_blocks.0",),
                   ("mid_block.attentions.1",),
                   ("down_blocks.0", "nope"),
                   ("down",),                     # not at a component boundary
                   ("down_blocks.1.attentions.0.transformer_blocks",),
                   ("mi",), ("",), (3,)):
        with pytest.raises(ValueError, match="pag_applied_layers"):
            chk(1.0, layers, names)
        with pytest.raises(ValueError, match="pag_applied_layers"):
            chk(0.0, layers, names)               # a bad entry is an error even while PAG is off
    with pytest.raises(ValueError, match="pag_applied_layers"):
        chk(1.0, (), names)
    with pytest.raises(ValueError, match="cache"):
        chk(1.0, ("mid",), names, has_cache=True)
    with pytest.raises(ValueError, match="fp8_attention"):
        chk(1.0, ("mid",), names, fp8_attention=True)


def test_new_symbols_are_declared():
    from mrisr import _lib
    hdr = open(os.path.join(ROOT, "include", "mrisr.h")).read()
    declared = set(re.findall(r"^(?:int|void|int64_t|size_t|const char\*)\s+(mrisr_[a-z0-9_]+)\(", hdr, flags=re.M))
    new = {"mrisr_model_set_pag", "mrisr_model_num_transformer_blocks", "mrisr_sampler_set_pag", "mrisr_sampler_run_pag",
           "mrisr_sampler_num_captures", "mrisr_op_attn_identity", "mrisr_op_pag_step", "mrisr_op_pag_multistep_step"}
    assert new <= declared and new <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.fixture(scope="module")
def tiny():
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=2501, perturb_norm=True)
    p.update(ou.init_lora_params(p, rank=4, seed=2503))
    g = torch.Generator().manual_seed(2502)
    x = torch.randn((2, 4, 16, 16), generator=g)
    ctx = torch.randn((2, 77, cfg.cross_attention_dim), generator=g)
    net = ou.OracleUNet(p, cfg)
    return dict(cfg=cfg, p=p, net=net, x=x, ctx=ctx, t=torch.tensor(500), eps=net(x, torch.tensor(500), encoder_hidden_states=ctx).sample)


def test_patched_oracle_with_no_block_selected_is_the_oracle(tiny):
    with perturbed_attention(()):
        e = tiny["net"](tiny["x"], tiny["t"], encoder_hidden_states=tiny["ctx"]).sample
    assert torch.equal(e, tiny["eps"])
    # ... and the patch is gone afterwards, also after an exception inside the block
    from oracle import unet as ou
    orig = ou.attention
    with pytest.raises(RuntimeError):
        with perturbed_attention(("mid",)):
            assert ou.attention is not orig
            raise RuntimeError("x")
    assert ou.attention is orig
    assert torch.equal(tiny["net"](tiny["x"], tiny["t"], encoder_hidden_states=tiny["ctx"]).sample, tiny["eps"])


def test_perturbation_is_real_and_row_local(tiny):
    net, x, t, ctx, eps = (tiny[k] for k in ("net", "x", "t", "ctx", "eps"))
    change = {}
    for layers in (("mid",), ("down_blocks.0",), ("up_blocks.3",), ("down_blocks", "mid", "up_blocks")):
        with perturbed_attention(layers):
            change[layers] = rel(net(x, t, encoder_hidden_states=ctx).sample, eps)
    print("relative L2 change of the oracle's prediction:", {".".join(k) if len(k) == 1 else "all": f"{v:.3e}" for k, v in change.items()})
    assert change[("mid",)] >= 5e-3
    assert change[("down_blocks", "mid", "up_blocks")] >= 0.3
    assert change[("down_blocks.0",)] >= 0.1 and change[("up_blocks.3",)] >= 0.1
    # rows: only the perturbed sample moves, and it moves exactly as in the all-rows call
    with perturbed_attention(("down_blocks.0", "up_blocks.3")):
        full = net(x, t, encoder_hidden_states=ctx).sample
    with perturbed_attention(("down_blocks.0", "up_blocks.3"), rows=slice(0, 1)):
        part = net(x, t, encoder_hidden_states=ctx).sample
    assert torch.equal(part[1], eps[1]) and rel(part[0], full[0]) < 1e-5 and rel(part[0], eps[0]) > 0.1


def test_pag_unet_combines_as_the_contract_says(tiny):
    net, x, t, ctx, eps = (tiny[k] for k in ("net", "x", "t", "ctx", "eps"))
    layers = ("down_blocks.0", "up_blocks.3")
    # s = 0 returns eps_c
    w0 = PagUNet(net, ctx, 0.0, layers)
    assert torch.equal(w0(x, t).sample, eps)
    # two-way: e = eps_c + s (eps_c - eps_p), and .last keeps the parts
    w = PagUNet(net, ctx, 3.0, layers)
    e = w(x, t).sample
    ep, eu, ec, e64 = w.last
    assert eu is None and torch.equal(ec, eps) and rel(ep, eps) > 0.1
    assert rel(e, eps.double() + 3.0 * (eps.double() - ep.double())) < 1e-6 and torch.equal(e, e64.to(e.dtype))
    # three-way with rescale
    g = torch.Generator().manual_seed(2504)
    ctx_u = torch.randn((1, 77, tiny["cfg"].cross_attention_dim), generator=g).expand(2, -1, -1)
    w3 = PagUNet(net, ctx, 1.5, layers, ctx_u=ctx_u, guidance_scale=3.0, guidance_rescale=0.7)
    e3 = w3(x, t).sample
    ep, eu, ec, _ = w3.last
    raw = eu.double() + 3.0 * (ec.double() - eu.double()) + 1.5 * (ec.double() - ep.double())
    want = raw * (0.7 * ec.double().std(dim=(1, 2, 3), keepdim=True) / raw.std(dim=(1, 2, 3), keepdim=True) + 0.3)
    assert rel(e3, want) < 1e-6
    # the three-way combine at s = 0 equals guided_eps
    for phi in (0.0, 0.7):
        assert torch.equal(pag_eps(ep, eu, ec, 3.0, 0.0, phi), guided_eps(eu.double(), ec.double(), 3.0, phi))
    # the two-way combine is the guided combine with eps_0 := eps_p and g := 1 + s (what the device step computes)
    assert rel(pag_eps(ep, None, ec, 1.0, 2.0, 0.7), guided_eps(ep.double(), ec.double(), 3.0, 0.7)) < 1e-12
