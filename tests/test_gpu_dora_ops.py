"""GPU: the two DoRA kernels on their own (csrc/dora.hip) through ``mrisr_op_dora_scale`` / ``mrisr_op_dora_mag_grad``, against the closed
formula in float64 on the CPU.  Method and bounds of tests/test_gpu_bwd_ops.py:

  * inputs are drawn in f32 and rounded to the dtype under test; the reference is evaluated in float64 on those rounded inputs and rounds
    nowhere else; where the kernel adds into an existing tensor the reference is ``prior + g``;
  * coarse: relative L2 <= 1e-3 (f32 outputs) or 1.2e-2 (bf16 outputs);
  * element-wise, no element excluded: |got - ref| <= r |ref| + floor, r = 2^-8 for a bf16 output (one round-to-nearest of an f32 result),
    r = 0 for an f32 output;
  * bits repeat over three more launches (neither kernel uses atomics).

``floor`` stands for f32 arithmetic noise, measured without a GPU and without the kernels: the same formula in plain torch float32 on the
CPU against the float64 reference, on this module's own inputs, largest absolute deviation over all cases of the output class; the floor
is 8 x that.  ``python tests/test_gpu_dora_ops.py`` prints the table again.

    output class        largest |f32 torch - f64|   floor (x 8)
    -------------------------------------------------------------
    dora.g              2.664e-07                   2.131e-06
    dora.mag_grad       1.085e-04                   8.679e-04
    dora.rows           3.437e-07                   2.749e-06
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
TOL = {"f32": 1e-3, "bf16": 1.2e-2}   # tests/test_gpu_bwd_ops.py
F64 = torch.float64

# measured: largest |plain torch f32 - f64 reference| over the cases of the class (see the module docstring); the floor is 8 x this
MEASURED = {
    "dora.g": 2.664e-07,
    "dora.mag_grad": 1.085e-04,
    "dora.rows": 3.437e-07,
}
FLOOR = {k: 8.0 * v for k, v in MEASURED.items()}


def _packed_rows(half):
    """mrisr.ops.geglu_packed_rows: raw row g * half + j is stored at (j >> 4) * 32 + (j & 15) + 16 g"""
    j = torch.arange(half, dtype=torch.int64)
    p = (j >> 4) * 32 + (j & 15)
    return torch.cat([p, p + 16])


# ---- dora_mag_grad: (C, M, pitch padding, R, bias, geglu_half) ----------------------------------------------------------------------
MAG_CASES = [
    (64, 154, 0, False, False, 0),
    (64, 154, 8, True, True, 0),
    (320, 1024, 16, True, False, 0),
    (320, 1024, 0, False, True, 160),      # GEGLU half 160
    (1280, 4136, 8, True, True, 0),
    (2560, 154, 8, True, True, 1280),      # GEGLU half 1280
]
MAG_IDS = [f"C{c}-M{m}-pad{p}{'-R' if r else ''}{'-bias' if b else ''}{'-half%d' % h if h else ''}" for c, m, p, r, b, h in MAG_CASES]


@functools.lru_cache(maxsize=None)
def _mag_inputs(dt, case):
    Cc, M, pad, has_r, has_b, half = MAG_CASES[case]
    g = torch.Generator().manual_seed(7000 + 10 * case + (dt == "bf16"))
    P, Y = (torch.randn((M, Cc), generator=g).to(DT[dt]) for _ in range(2))
    R = torch.randn((M, Cc), generator=g).to(DT[dt]) if has_r else None
    bias = torch.randn((Cc,), generator=g) if has_b else None
    mag = 0.5 + torch.rand((Cc,), generator=g)
    prior = torch.randn((Cc,), generator=g)
    return P, Y, R, bias, mag, prior


def _mag_formula(P, Y, R, bias, mag, prior, half, prec):
    P, Y = P.to(prec), Y.to(prec)
    d = Y if R is None else Y - R.to(prec)
    col = (P * d).sum(0)
    if bias is not None:
        col = col - bias.to(prec) * P.sum(0)
    if half:
        col = col[_packed_rows(half)]   # raw row c reads the interleaved column of c
    return prior.to(prec) + col / mag.to(prec)


@pytest.mark.parametrize("case", range(len(MAG_CASES)), ids=MAG_IDS)
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_dora_mag_grad(dt, case):
    from mrisr import ops
    Cc, M, pad, has_r, has_b, half = MAG_CASES[case]
    P, Y, R, bias, mag, prior = _mag_inputs(dt, case)
    ref = _mag_formula(P, Y, R, bias, mag, prior, half, F64)

    def padded(t, loud):  # rows of pitch C + pad, the columns beyond C loud garbage
        if t is None:
            return None
        buf = torch.full((M, Cc + pad), loud, dtype=t.dtype)
        buf[:, :Cc] = t
        return buf.cuda()

    Pd, Yd, Rd = padded(P, 3e4), padded(Y, -7e4), padded(R, float("nan"))
    bd, md = (None if bias is None else bias.cuda()), mag.cuda()

    def run():
        gm = prior.cuda().clone()
        return ops.dora_mag_grad(Pd, Yd, md, gm, M, Cc, R=Rd, bias=bd, geglu_half=half)

    got = run()
    _check("dora.mag_grad", f"dora_mag_grad[{dt} {MAG_IDS[case]}]", got, ref, "f32")
    for _ in range(3):
        assert torch.equal(run(), got), "bits changed between launches"


# ---- dora_scale: (n, k, r, geglu_half, pitch padding) x scale -----------------------------------------------------------------------
SCALE_CASES = [
    (64, 72, 4, 0, 8),          # ragged k: not a multiple of the 256 lanes of a row
    (320, 320, 16, 0, 0),
    (1280, 5120, 4, 0, 0),
    (2560, 320, 64, 1280, 64),  # the GEGLU interleave, a high rank, the [W | sB] pitch
]
SCALE_IDS = [f"n{n}-k{k}-r{r}{'-half%d' % h if h else ''}" for n, k, r, h, _ in SCALE_CASES]
SCALES = [0.375, -2.5]


@functools.lru_cache(maxsize=None)
def _scale_inputs(case, si):
    n, k, r, half, pad = SCALE_CASES[case]
    g = torch.Generator().manual_seed(7100 + 10 * case + si)
    W = 0.05 * torch.randn((n, k), generator=g)
    A = 0.1 * torch.randn((r, k), generator=g)
    B = 0.1 * torch.randn((n, r), generator=g)
    wn = torch.linalg.vector_norm(W.double() + SCALES[si] * (B.double() @ A.double()), dim=1)
    mag = (wn * (1 + 0.1 * (torch.rand((n,), generator=g, dtype=F64) * 2 - 1))).float()   # +- 10 % around the norm
    return W, A, B, mag


def _scale_formula(W, A, B, mag, s, merged, prec):
    v = W.to(prec) + s * (B.to(prec) @ A.to(prec))
    g = mag.to(prec) / torch.linalg.vector_norm(v, dim=1)
    return g, g[:, None] * (v if merged else W.to(prec))


@pytest.mark.parametrize("merged", [False, True], ids=["apart", "merged"])
@pytest.mark.parametrize("si", range(len(SCALES)), ids=[f"s{s}" for s in SCALES])
@pytest.mark.parametrize("case", range(len(SCALE_CASES)), ids=SCALE_IDS)
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_dora_scale(dt, case, si, merged):
    from mrisr import ops
    n, k, r, half, pad = SCALE_CASES[case]
    W, A, B, mag = _scale_inputs(case, si)
    g_ref, rows_ref = _scale_formula(W, A, B, mag, SCALES[si], merged, F64)
    assert float((g_ref - 1).abs().max()) > 0.05  # the magnitudes are off the norm: g != 1
    Wd, Ad, Bd, md = W.cuda(), A.cuda(), B.cuda(), mag.cuda()

    def run():
        return ops.dora_scale(Wd, Ad, Bd, md, SCALES[si], DT[dt], ld=k + pad, geglu_half=half, merged=merged)

    g, rows = run()
    perm = _packed_rows(half).cuda() if half else torch.arange(n).cuda()   # packed[perm] = raw
    name = f"dora_scale[{dt} {SCALE_IDS[case]} s={SCALES[si]} {'merged' if merged else 'apart'}]"
    _check("dora.g", name + " g", g[perm], g_ref, "f32")
    _check("dora.rows", name + " rows", rows[perm][:, :k], rows_ref, dt)
    if pad:
        assert bool(torch.isnan(rows[:, k:].float()).all()), "columns beyond k inside the pitch were written"
    for _ in range(3):
        g2, rows2 = run()
        assert torch.equal(g2, g) and torch.equal(rows2[:, :k], rows[:, :k]), "bits changed between launches"


# ---- refusals: before any launch (every buffer is large enough for the call it refuses) ---------------------------------------------
def _refused(fn, *a, **kw):
    from mrisr import MrisrError
    with pytest.raises(MrisrError):
        fn(*a, **kw)


def test_dora_ops_refuse_bad_arguments():
    from mrisr import _lib as L, ops
    big = lambda dt: torch.zeros((64, 128), dtype=dt, device="cuda")
    vec = lambda n=256: torch.ones((n,), dtype=torch.float32, device="cuda")
    for dt in (torch.bfloat16, torch.float32):
        P, Y = big(dt), big(dt)
        ops.dora_mag_grad(P, Y, vec(), vec(), 64, 64)                                   # the well-formed call runs
        _refused(ops.dora_mag_grad, P, Y, vec(), vec(), 64, 64, ldp=56)                 # pitch below the row
        _refused(ops.dora_mag_grad, P, Y, vec(), vec(), 64, 64, R=big(dt), ldr=32)
        _refused(ops.dora_mag_grad, P, Y, vec(), vec(), 64, 60)                         # C % 8
        _refused(ops.dora_mag_grad, P, Y, vec(), vec(), 0, 64)                          # no rows
        _refused(ops.dora_mag_grad, P.view(-1)[1:], Y, vec(), vec(), 32, 64, ldp=128)   # misaligned P
        _refused(ops.dora_mag_grad, P, Y, vec()[1:], vec(), 64, 64)                     # misaligned mag
        _refused(ops.dora_mag_grad, P, Y, vec(), vec(), 64, 64, geglu_half=24)          # C != 2 * half / half % 16
        _refused(ops.dora_mag_grad, P, Y, vec(), vec(), 64, 48, geglu_half=24)
        with pytest.raises(L.MrisrError):                                               # null operand
            L.check(L.lib().mrisr_op_dora_mag_grad(L.dtype_id(dt), None, 128, Y.data_ptr(), 128, None, 0, None, vec().data_ptr(),
                                                   vec().data_ptr(), 64, 64, 0, L.stream_ptr()))
    W, A, B, m = (torch.ones(s, device="cuda") for s in ((64, 64), (160, 64), (64, 160), (80,)))
    A4, B4, m64 = A[:4], B[:, :4].contiguous(), m[:64]
    for dt in (torch.bfloat16, torch.float32):
        ops.dora_scale(W, A4, B4, m64, 1.0, dt)                                         # the well-formed call runs
        for r in (5, 20, 24, 144):                                                      # rank outside the accepted set
            _refused(ops.dora_scale, W, A[:r], B[:, :r].contiguous(), m64, 1.0, dt)
        _refused(ops.dora_scale, W, A4, B4, m64, 1.0, dt, ld=56)                        # pitch below the row
        _refused(ops.dora_scale, W, A4, B4, m[1:65], 1.0, dt)                           # misaligned mag
        _refused(ops.dora_scale, W, A4, B4, m64, 1.0, dt, geglu_half=16)                # n != 2 * half
        _refused(ops.dora_scale, W, A4, B4, m64, 1.0, dt, geglu_half=24)
        with pytest.raises(L.MrisrError):                                               # null operand
            L.check(L.lib().mrisr_op_dora_scale(L.dtype_id(dt), W.data_ptr(), None, B4.data_ptr(), m64.data_ptr(), 1.0, m.data_ptr(),
                                                W.data_ptr(), 64, 64, 64, 4, 0, 0, L.stream_ptr()))


def _check(key, name, got, ref, out_dt):
    """coarse relative L2 + the element-wise bound of the module docstring; `ref` float64 (CPU), `got` a GPU tensor"""
    ref = ref.to(F64).cuda()
    got = got.to(F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name
    l2 = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    r = 2.0 ** -8 if out_dt == "bf16" else 0.0
    excess = float(((got - ref).abs() - r * ref.abs()).max())
    print(f"{name}: rel-L2 {l2:.3e} (<= {TOL[out_dt]:.1e})  max(|d| - r|ref|) {excess:.3e} (<= floor[{key}] {FLOOR[key]:.3e})")
    assert l2 <= TOL[out_dt], (name, l2)
    assert excess <= FLOOR[key], (name, excess, FLOOR[key])


if __name__ == "__main__":   # the floors: plain torch f32 against float64 on this module's inputs, on the CPU
    worst = {k: 0.0 for k in MEASURED}
    for dt in ("bf16", "f32"):
        for case in range(len(MAG_CASES)):
            P, Y, R, bias, mag, prior = _mag_inputs(dt, case)
            half = MAG_CASES[case][5]
            d = (_mag_formula(P, Y, R, bias, mag, prior, half, torch.float32).double() - _mag_formula(P, Y, R, bias, mag, prior, half, F64)).abs().max()
            worst["dora.mag_grad"] = max(worst["dora.mag_grad"], float(d))
    for case in range(len(SCALE_CASES)):
        for si in range(len(SCALES)):
            for merged in (False, True):
                W, A, B, mag = _scale_inputs(case, si)
                g32, r32 = _scale_formula(W, A, B, mag, SCALES[si], merged, torch.float32)
                g64, r64 = _scale_formula(W, A, B, mag, SCALES[si], merged, F64)
                worst["dora.g"] = max(worst["dora.g"], float((g32.double() - g64).abs().max()))
                worst["dora.rows"] = max(worst["dora.rows"], float((r32.double() - r64).abs().max()))
    print("    output class        largest |f32 torch - f64|   floor (x 8)")
    for k in sorted(worst):
        print(f"    {k:<19} {worst[k]:<27.3e} {8 * worst[k]:.3e}")
