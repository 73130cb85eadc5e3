"""The two row-local fused kernels of a C = 320 transformer block as single ops, element-wise against float64:
`ops.xattn_tail` (csrc/xtail.hip: attn1.to_out + residual, LayerNorm2, attn2.to_q, 8-head cross-attention over the packed prompt
K / V, attn2.to_out + residual - one launch) and `ops.mlp(..., wp=, xres=)` (the proj_out continuation of mlp_fused_kernel).

Yardstick (tests/xtail_ref.py, pinned on the CPU by test_xtail_ref_cpu.py): `exact` is float64 on the operands the kernel is given,
`emulated` the same chain with the kernel's rounding points.  Three measures of a result against `exact` - largest deviation over
largest value, relative L2, the worst row's relative L2 - are taken for the kernel and for `emulated` on the same operands, and the
kernel's must be at most MARGIN times the emulation's.  The margin covers what `emulated` does not model: f32 accumulation order,
v_exp_f32, and a maximum taken over 1e5 .. 1e7 rounding events.  A layout, mask or head-mapping fault moves the first measure to
O(0.1 .. 1) against a yardstick of about 5e-3.

Measured on an MI355X, kernel / emulation per measure (largest deviation, relative L2, worst row), every case of a family:
  random operands, 40 cases (emulation 4.4e-3 .. 8.2e-3, 2.7e-3 .. 3.7e-3, 3.1e-3 .. 6.3e-3)   1.000  0.999 .. 1.000  1.000
  one key per head (emulation 2.3e-6, 1.3e-7, 1.0e-6: the recipe is exact in bf16)             1.000  1.000  1.000
  uniform attention, nk = 1 / 17 / 64 / 65 / 77                                                1.000  1.000  1.000
  scores of +-150, maximum in the last key / all equal                                         1.000  1.000  1.000
  LayerNorm rows: offset 30, spike of 100, constant, gamma / beta far from 1 / 0               1.000  1.000  1.000
  pitches 328 / 384; ntok = 128 with 3 images; ntok = 1024; 48 and 320 workgroups              1.000  1.000  1.000
  feed-forward + proj_out, six cases (emulation 4.1e-3 .. 6.2e-3, 3.1e-3 .. 3.4e-3, 3.6e-3 .. 4.6e-3)   1.000  1.000  1.000
  (and 1.76e-3 .. 1.78e-3 relative L2 from the separate launches: the one rounding they do not share)
so the starting margins stand: MARGIN = (2, 1.5, 2), no rounding point had to be added.  That the checks bite was tried by hand
on a wrapper built wrong (not committed): nk + 1 handed to the pack and the kernel - the uniform cases gave 2.0 .. 70 / 9.0 .. 289 /
10 .. 340 against bounds of ~1e-2 (ratios 350 .. 114,000); to_q's weight left in natural K order - the one-key-per-head case gave
1.33 / 0.86 / 1.06 and wrong elements in every head.  nk + 1 handed to the pack ALONE changes nothing: the kernel masks every key
>= nk itself, the pack's zeroes are a second line.
"""
import ctypes as C
import json

import pytest
import torch

import xtail_ref as xr

pytestmark = pytest.mark.gpu

MARGIN = (2.0, 1.5, 2.0)   # largest deviation, relative L2, worst row
LDS_POISON = 2048


def _middle(op):
    from mrisr import ops
    c = xr.to(op, "cuda")
    return ops.xattn_tail(c["ao"], c["t"], c["ntok"], c["w1"], c["b1"], c["gamma"], c["beta"], c["wq"], c["bq"], c["w2"], c["b2"],
                          c["k"], c["v"], nk=c["nk"], lora=c["lora"], lora_scale=c["lora_scale"])


def _ff(op):
    from mrisr import ops
    c = xr.to(op, "cuda")
    return ops.mlp(c["x"], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["b2"], residual=c["residual"], wp=c["wp"], bp=c["bp"],
                   xres=c["xres"])


def _held(name, y, op, exact_fn, emulated_fn):
    """The three measures of ``y`` against those of the emulation; the references on the device where the operands are large."""
    dev = "cuda" if y.shape[0] > 2048 else "cpu"
    o = xr.to(op, dev)
    exact = exact_fn(o)
    km, em = xr.measures(y[:, :320].to(dev), exact), xr.measures(emulated_fn(o), exact)
    ratio = [k / e if e > 0 else (1.0 if k == 0 else float("inf")) for k, e in zip(km, em)]
    print(f"{name}: kernel " + " ".join(f"{v:.3e}" for v in km) + " | emulated " + " ".join(f"{v:.3e}" for v in em) +
          " | ratio " + " ".join(f"{v:.3f}" for v in ratio))
    assert bool(torch.isfinite(y.float()).all()), name
    for k, e, mg in zip(km, em, MARGIN):
        assert k <= mg * e, (name, km, em)


def _held_middle(name, y, op):
    _held(name, y, op, xr.middle_exact, xr.middle_emulated)


def _profiled(fn):
    """(result or the MrisrError raised, {kernel class: launches}) of one call."""
    from mrisr import _lib as L
    lib = L.lib()
    lib.mrisr_prof_reset(); lib.mrisr_prof_enable(1)
    try:
        try:
            out = fn()
        except L.MrisrError as e:
            out = e
        torch.cuda.synchronize()
    finally:
        lib.mrisr_prof_enable(0)
    buf = C.create_string_buffer(1 << 20)
    n = lib.mrisr_prof_report(buf, len(buf))
    lib.mrisr_prof_reset()
    return out, {k: v["launches"] for k, v in json.loads(buf.value[:n].decode()).items()}


def _repeatable(run, first, what):
    """Three more launches, then three with every workgroup's LDS pre-filled with NaN bytes: the same bits each time."""
    from mrisr import _lib as L
    lib = L.lib()
    for i in range(3):
        assert torch.equal(first, run()), f"{what}: not repeatable ({i})"
    try:
        lib.mrisr_debug_gemm_flags(C.c_int(LDS_POISON))
        for i in range(3):
            assert torch.equal(first, run()), f"{what}: depends on stale LDS ({i})"
    finally:
        lib.mrisr_debug_gemm_flags(C.c_int(0))


# ------------------------------------------------------------------------------------------------------------------------------
# the middle
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lora,bias", [(False, True), (True, True), (True, False), (False, False)])
@pytest.mark.parametrize("nk", [1, 15, 16, 17, 63, 64, 65, 77, 79, 80])
def test_middle_random_operands(nk, lora, bias):
    """Two workgroups, two images (the image changes at every workgroup: img = m0 / ntok), every key count at which a fragment
    fills or the masking rule of the softmax (`i == 4 || nk <= 64`) changes sides; adapters and biases present and absent (absent
    biases read the zero page)."""
    op = xr.middle_random(nk=nk, lora=lora, bias=bias, seed=nk)
    _held_middle(f"random nk={nk} lora={lora} bias={bias}", _middle(op), op)


def test_middle_head_mapping():
    """One key per (row, head), a permutation of its own per head (xtail_ref.middle_one_hot): x2 - x1 must be the selected row of V
    in each head's 40 columns, bit for bit - and in the four 16-column blocks that two heads share (columns 32-47 and 112-127 of
    each 160-column group), which `carry` hands from the even head to the odd one."""
    op, sel = xr.middle_one_hot()
    y = _middle(op)
    _held_middle("one key per head", y, op)
    d = (y.float() - op["t"].cuda().float()).cpu()
    B, ntok = sel.shape[0], sel.shape[2]
    want = torch.cat([torch.gather(op["v"].float()[:, :, 40 * h:40 * h + 40], 1, sel[:, h, :, None].expand(-1, -1, 40)) for h in range(8)],
                     dim=-1).reshape(B * ntok, 320)
    for h in range(8):
        cs = slice(40 * h, 40 * h + 40)
        assert torch.equal(d[:, cs], want[:, cs]), f"head {h}: {int((d[:, cs] != want[:, cs]).sum())} wrong elements"
    for c0 in (32, 112, 192, 272):
        assert torch.equal(d[:, c0:c0 + 16], want[:, c0:c0 + 16]), f"shared block at column {c0}"


@pytest.mark.parametrize("nk", [1, 17, 64, 65, 77])
def test_middle_key_masking(nk):
    """Uniform attention (Wq = 0) over the first nk of 80 buffer rows; rows >= nk of K and V hold +-1000 and nk goes through the
    op, so only the pack's and the kernel's masks keep them out: one leaked key moves the result by ~ 1000 / (nk + 1)."""
    op = xr.middle_uniform(nk)
    y = _middle(op)
    _held_middle(f"uniform nk={nk}", y, op)


@pytest.mark.parametrize("kind", ["last", "equal"])
def test_middle_softmax_range(kind):
    """Scores of +-150 (before log2 e): the maximum in the last key, and all scores equal; finite and within the bound."""
    op = xr.middle_softmax_range(kind)
    _held_middle(f"softmax {kind}", _middle(op), op)


@pytest.mark.parametrize("kind", ["offset", "spike", "constant", "affine"])
def test_middle_layernorm_rows(kind):
    """Rows with a large common offset, one dominant element 0, zero variance, and gamma / beta far from 1 / 0: the kernel's
    statistics are f32 with the variance shifted by the row's element 0."""
    op = xr.middle_layernorm(kind)
    _held_middle(f"layernorm {kind}", _middle(op), op)


def test_middle_row_pitches():
    """ldao = 328, ldt = 384: the 320 columns right, every padding column of t untouched."""
    op = xr.middle_random(lora=True, seed=71, ldao=328, ldt=384)
    y = _middle(op)
    assert y.shape == (256, 384)
    _held_middle("pitches 328 / 384", y, op)
    assert bool((y[:, 320:].float() == xr.PAD).all()), "padding of t written"


@pytest.mark.parametrize("M,ntok,seed", [(384, 128, 72), (1024, 1024, 73)])
def test_middle_tokens_per_image(M, ntok, seed):
    """Tokens per image of exactly one panel with three images, and eight panels inside one image."""
    op = xr.middle_random(M=M, ntok=ntok, lora=True, seed=seed)
    _held_middle(f"M={M} ntok={ntok}", _middle(op), op)


@pytest.mark.parametrize("panels", [48, 320])
def test_middle_schedule_coverage(panels):
    """48 workgroups: every DMA rotation rot_q = (blockIdx.x >> 2) % 10 and every rot_w; 320: more workgroups than CUs, so a
    workgroup inherits the LDS of one that has finished.  With adapters.  The first launch is held to the three measures; three more
    give the same bits, and so do three with poisoned LDS."""
    op = xr.middle_random(M=128 * panels, ntok=1024, lora=True, seed=80 + panels)
    first = _middle(op)
    _held_middle(f"{panels} workgroups", first, op)
    _repeatable(lambda: _middle(op), first, f"{panels} workgroups")


def test_middle_refusals_launch_nothing():
    """What xattn_tail_ok and the launcher's requirements refuse comes back as MrisrError before any launch of the kernel."""
    from mrisr import _lib as L
    good = xr.middle_random(lora=True, seed=90)
    y, cls = _profiled(lambda: _middle(good))
    assert torch.is_tensor(y) and cls.get("xattn_tail_c320") == 1, cls    # (the profiler does see this kernel)

    def variant(**kw):
        op = dict(good)
        op.update(kw)
        return op

    pair = good["lora"][0]
    r8 = (torch.zeros(8, 320), torch.zeros(320, 8))
    cases = {
        "nk = 0": variant(nk=0),
        "nk = 81": xr.middle_random(nk=81, seed=91),
        "M = 192": xr.middle_random(M=192, ntok=64, seed=92),
        "ntok = 192": xr.middle_random(M=384, ntok=192, seed=93),
        "adapters on two projections": variant(lora=[pair, pair, None]),
        "rank 8": variant(lora=[r8, r8, r8]),
        "f32 rows": variant(ao=good["ao"].float(), t=good["t"].float()),
    }
    for name, op in cases.items():
        out, cls = _profiled(lambda: _middle(op))
        assert isinstance(out, L.MrisrError), f"{name}: not refused"
        assert "xattn_tail_c320" not in cls, (name, cls)


# ------------------------------------------------------------------------------------------------------------------------------
# the feed-forward with its proj_out continuation
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,bias", [(128, 1280, True), (128, 64, False), (128 * 40, 1280, False), (128 * 40, 64, True),
                                      (128 * 300, 1280, True), (128 * 300, 64, False)])
def test_feed_forward_with_proj_out(M, H, bias):
    """One panel, 40, and 300 (more than CUs); the benchmark's hidden width and the smallest; proj_out's bias present and absent.
    Held to its own exact / emulated pair; against the separate-launch chain (ops.mlp, then ops.linear, + xres in f32), from which
    it differs by the last rounding (2^-9 of an element at most) and accumulation order; repeatable bits, poisoned LDS too."""
    from mrisr import ops
    op = xr.ff_random(M, H, bias, seed=H + bias)
    first = _ff(op)
    _held(f"ff M={M} H={H} bias={bias}", first, op, xr.ff_exact, xr.ff_emulated)
    c = xr.to(op, "cuda")
    mid = ops.mlp(c["x"], c["gamma"], c["beta"], c["w1"], c["b1"], c["w2"], c["b2"], residual=True)
    two = ops.linear(mid, c["wp"], c["bp"]).float() + c["xres"].float()
    d = float((first.float() - two).norm() / two.norm())
    print(f"ff M={M} H={H}: against the separate launches {d:.3e}")
    assert d < 2.0 ** -8, d
    _repeatable(lambda: _ff(op), first, f"ff M={M} H={H}")


def test_feed_forward_with_proj_out_refuses_a_ragged_panel():
    from mrisr import _lib as L
    y, cls = _profiled(lambda: _ff(xr.ff_random(128, 64, True, seed=1)))
    assert torch.is_tensor(y) and cls.get("mlp_fused_c320") == 1, cls
    out, cls = _profiled(lambda: _ff(xr.ff_random(200, 64, True, seed=2)))
    assert isinstance(out, L.MrisrError) and "mlp_fused_c320" not in cls, (out, cls)
