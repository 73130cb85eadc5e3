"""Pins tests/xtail_ref.py, the yardstick of test_gpu_xtail_op.py, on the CPU: ``*_exact`` is the literal torch composition of the
block (diffusers' BasicTransformerBlock as oracle/unet.py restates it) in float64, and ``*_emulated`` (the kernels' rounding points)
stays at the distance from it that a handful of bf16 roundings explain - for every operand recipe the GPU tests use, printed per case.

Where the bands come from: one bf16 rounding moves a value by at most 2^-9 of it (half an ulp, 8 significant bits) and by about
2^-9 / sqrt(3) ~ 1.1e-3 in the root mean square.  The middle rounds x1, the LayerNorm output, q, P, o and x2 (the two residual sums
twice each: eight roundings) and, with adapters, z of each projection (eleven); each reaches the output with a gain near one, so the
relative L2 distance is sqrt(8 .. 11) x 1.1e-3 = 3.2e-3 .. 3.7e-3 if none is damped, less where one is: above 2^-10 (the last
rounding alone) and below 2^-7 (twice the undamped estimate); the largest single deviation is below eight half ulps of the largest
value, 2^-6 of it, and so is every single row.  Recipes built to be exact in bf16 (one key per head) show almost no distance."""
import math

import pytest
import torch
import torch.nn.functional as F

import xtail_ref as xr

D = torch.float64


def _literal_middle(op):
    """F.linear / F.layer_norm / F.scaled_dot_product_attention in float64, an adapter folded into its weight (W + s B A)."""
    r = lambda w: w.float().to(torch.bfloat16).to(D)
    d = lambda v: None if v is None else v.to(D)

    def weight(name, i):
        w = r(op[name])
        if op.get("lora"):
            a, b = op["lora"][i]
            w = w + (b.float() * torch.tensor(op["lora_scale"])).to(D) @ r(a)
        return w

    ntok, nk = op["ntok"], op["nk"]
    ao, x0 = op["ao"][:, :320].to(D), op["t"][:, :320].to(D)
    x1 = F.linear(ao, weight("w1", 0), d(op["b1"])) + x0
    q = F.linear(F.layer_norm(x1, (320,), d(op["gamma"]), d(op["beta"]), 1e-5), weight("wq", 1), d(op["bq"]))
    hm = lambda t, n: t.reshape(-1, n, 8, 40).transpose(1, 2)
    o = F.scaled_dot_product_attention(hm(q, ntok), hm(op["k"][:, :nk].to(D), nk), hm(op["v"][:, :nk].to(D), nk))
    return F.linear(o.transpose(1, 2).reshape(-1, 320), weight("w2", 2), d(op["b2"])) + x1


def _literal_ff(op):
    r = lambda w: w.float().to(torch.bfloat16).to(D)
    d = lambda v: None if v is None else v.to(D)
    x = op["x"].to(D)
    u, g = F.linear(F.layer_norm(x, (320,), d(op["gamma"]), d(op["beta"]), 1e-5), r(op["w1"]), d(op["b1"])).chunk(2, dim=-1)
    f = F.linear(u * F.gelu(g), r(op["w2"]), d(op["b2"])) + (x if op["residual"] else 0)
    return F.linear(f, r(op["wp"]), d(op["bp"])) + op["xres"].to(D)


# every operand recipe of test_gpu_xtail_op.py: (id, builder, family)
MIDDLE = [(f"random-nk{nk}-lora{int(lo)}-bias{int(bi)}", (lambda nk=nk, lo=lo, bi=bi: xr.middle_random(nk=nk, lora=lo, bias=bi, seed=nk)), "random")
          for nk in (1, 15, 16, 17, 63, 64, 65, 77, 79, 80) for lo, bi in ((False, True), (True, True), (True, False), (False, False))]
MIDDLE += [("one-hot", lambda: xr.middle_one_hot()[0], "exact")]
MIDDLE += [(f"uniform-nk{nk}", (lambda nk=nk: xr.middle_uniform(nk)), "random") for nk in (1, 17, 64, 65, 77)]
MIDDLE += [(f"softmax-{kind}", (lambda kind=kind: xr.middle_softmax_range(kind)), "softmax") for kind in ("last", "equal")]
MIDDLE += [(f"layernorm-{kind}", (lambda kind=kind: xr.middle_layernorm(kind)), "layernorm") for kind in ("offset", "spike", "constant", "affine")]
MIDDLE += [("strides", lambda: xr.middle_random(lora=True, seed=71, ldao=328, ldt=384), "random"),
           ("ntok128-B3", lambda: xr.middle_random(M=384, ntok=128, lora=True, seed=72), "random"),
           ("ntok1024-B1", lambda: xr.middle_random(M=1024, ntok=1024, lora=True, seed=73), "random"),
           # (the 320-workgroup case is this recipe at M = 40,960: too large for a CPU test, and no other input)
           ("48-workgroups", lambda: xr.middle_random(M=128 * 48, ntok=1024, lora=True, seed=80 + 48), "random")]


@pytest.mark.parametrize("name,build,family", MIDDLE, ids=[m[0] for m in MIDDLE])
def test_middle_reference(name, build, family):
    op = build()
    exact, lit, emu = xr.middle_exact(op), _literal_middle(op), xr.middle_emulated(op)
    assert exact.dtype == D and bool(torch.isfinite(exact).all())
    assert float((exact - lit).abs().max()) <= 1e-12 * float(lit.abs().max())
    m1, m2, m3 = xr.measures(emu, exact)
    print(f"middle {name}: emulated vs exact max-abs {m1:.3e} rel-L2 {m2:.3e} worst row {m3:.3e}")
    assert torch.equal(emu, xr.bf(emu))                     # a bf16 result
    if family == "exact":
        assert m1 < 1e-4 and m2 < 1e-4 and m3 < 1e-4, (m1, m2, m3)
    else:
        # (softmax / layernorm recipes: fewer roundings are live - rows of +-1, a zero projection - so only the upper bounds hold)
        assert m2 < 2.0 ** -7 and m1 < 2.0 ** -6, (m1, m2, m3)
        if family == "random":
            assert m2 > 2.0 ** -10, m2
    assert m3 < 2.0 ** -6, m3


def test_one_hot_recipe_selects_one_key_per_head():
    """The claim test_gpu_xtail_op.py asserts on the kernel, on the reference first: x2 - x1 is the selected row of V, exactly."""
    op, sel = xr.middle_one_hot()
    emu = xr.middle_emulated(op)
    x1 = op["t"].to(D)
    B, ntok = sel.shape[0], sel.shape[2]
    for h in range(8):
        cs = slice(40 * h, 40 * h + 40)
        want = torch.gather(op["v"].to(D)[:, :, cs], 1, sel[:, h, :, None].expand(-1, -1, 40)).reshape(B * ntok, 40)
        assert torch.equal(emu[:, cs] - x1[:, cs], want), h
    assert len({tuple(sel[0, h].tolist()) for h in range(8)}) == 8   # a permutation of its own per head


def test_uniform_recipe_is_the_mean_of_the_live_rows():
    op = xr.middle_uniform(17)
    exact = xr.middle_exact(op)
    x1 = F.linear(op["ao"].to(D), op["w1"].to(torch.bfloat16).to(D), op["b1"].to(D)) + op["t"].to(D)
    mean = op["v"][:, :17].to(D).mean(1).repeat_interleave(op["ntok"], 0)
    assert float((exact - x1 - mean).abs().max()) < 1e-12
    assert float(op["v"][:, 17:].abs().min()) == 1000.0 and op["v"].shape[1] == 80


@pytest.mark.parametrize("kind,lo,hi", [("last", 140.0, 160.0), ("equal", 140.0, 160.0)])
def test_softmax_recipe_reaches_the_scores_it_claims(kind, lo, hi):
    op = xr.middle_softmax_range(kind)
    x1 = op["t"].to(D)
    q = F.linear(F.layer_norm(x1, (320,)), op["wq"].to(D))
    s = (xr._heads(q, op["ntok"]) @ xr._heads(op["k"].to(D), op["nk"]).transpose(-1, -2)) / math.sqrt(40)
    top = s.abs().amax(-1)
    print(f"softmax-{kind}: |score| max per row in [{float(top.min()):.1f}, {float(top.max()):.1f}]")
    assert float(top.min()) > lo and float(top.max()) < hi
    if kind == "last":   # in the rows +p the maximum is the last key
        plus = s[..., -1] > 0
        assert bool((s.argmax(-1)[plus] == op["nk"] - 1).all()) and bool(plus.any()) and bool((~plus).any())
    else:
        assert float((s - s[..., :1]).abs().max()) < 1e-9


FFN = [(128, 1280, True), (128, 64, False), (128 * 40, 64, True)]   # (the larger GPU cases: the same recipe with more rows)


@pytest.mark.parametrize("M,H,bias", FFN)
def test_feed_forward_reference(M, H, bias):
    op = xr.ff_random(M, H, bias, seed=H + bias)
    exact, lit, emu = xr.ff_exact(op), _literal_ff(op), xr.ff_emulated(op)
    assert float((exact - lit).abs().max()) <= 1e-12 * float(lit.abs().max())
    m1, m2, m3 = xr.measures(emu, exact)
    print(f"ff M={M} H={H} bias={bias}: emulated vs exact max-abs {m1:.3e} rel-L2 {m2:.3e} worst row {m3:.3e}")
    # six roundings (LayerNorm output, hidden activation, FF2, + x, proj_out, + xres): the same band as the middle
    assert 2.0 ** -10 < m2 < 2.0 ** -7 and m1 < 2.0 ** -6 and m3 < 2.0 ** -6, (m1, m2, m3)


def test_measures():
    e = torch.tensor([[3.0, 4.0], [0.0, 1.0]], dtype=D)
    y = e.clone()
    y[1, 1] = 1.5
    m1, m2, m3 = xr.measures(y, e)
    assert m1 == 0.5 / 4 and abs(m2 - 0.5 / math.sqrt(26)) < 1e-15 and m3 == 0.5
