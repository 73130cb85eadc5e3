"""GPU: the LoRA weight-gradient kernel for ranks 32 .. 128 on its own (csrc/bwd.hip: lora_wgrad_hr_kernel on the bf16 MFMA through transposed
LDS reads; the f32 engine walks the streaming kernel over 16 columns of Q at a time) through ``mrisr_op_lora_wgrad_hr``.

    out_j (+)= scale * sum_m P[m][c] Q[m][j * rp + q],   q < r;   rp = r rounded up to 64 (bf16) / 32 (f32)

Method and bounds are those of tests/test_gpu_bwd_ops.py, restated: inputs are drawn in f32 and rounded to the dtype under test (Q is of the
engine's type here); the reference is ``prior + scale * g`` in float64 on the rounded inputs, the outputs pre-filled and non-zero.

  * coarse: relative L2 <= 1e-3;
  * element-wise, no element excluded: |got - ref| <= floor;
  * the bits of three further launches equal the first.

Every column of Q is drawn non-zero, the padding columns [r, rp) of each module included: none of them may reach an output.

``floor`` stands for f32 arithmetic noise: 8 x the largest |plain torch float32 - float64| of the same formula over this module's own cases,
measured on the CPU without the kernel (``python tests/test_gpu_lora_wgrad_hr.py`` prints it again):

    output class        largest |f32 torch - f64|   floor (x 8)
    -------------------------------------------------------------
    lora.wgrad_hr       2.007e-04                   1.606e-03

In mode 0 (dB) a case's C is the width of one module's section: P has nmod * C columns (C = 64 cannot be cut into three sections of whole
vectors, and fused Q / K / V are three sections of C anyway).  In mode 1 (dA) C is the width of x.
"""
import ctypes as C_
import functools
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
F64 = torch.float64
TOL = 1e-3
MEASURED = {"lora.wgrad_hr": 2.007e-04}  # largest |plain torch f32 - f64| over ALL_CASES (see the module docstring); the floor is 8 x this
FLOOR = {k: 8.0 * v for k, v in MEASURED.items()}

SHAPES = ((64, 154), (320, 1024), (1280, 4136))  # (C, M): M = 154 and 4136 are ragged against the 32-row step and any slab; C = 64 is one tile


def _case(dt, Cc, M, r, nmod, mode, scale=1.0, ldp=None, ldq=None, null=(), garbage=1.0, half=0):
    return (dt, Cc, M, r, nmod, mode, scale, ldp, ldq, tuple(null), garbage, half)


GRID = [_case("bf16", Cc, M, r, nmod, mode) for (Cc, M) in SHAPES for r in (32, 48, 64, 128) for nmod in (1, 3) for mode in (0, 1)]
GRID_F32 = [_case("f32", 320, 154, r, nmod, mode) for r in (32, 64) for nmod in (1, 3) for mode in (0, 1)]


def _extras(dt):
    return [
        _case(dt, 320, 1024, 32, 3, 0, null=(1,)),                  # no adapter on the middle module, dB: its section of dY is skipped
        _case(dt, 320, 1024, 32, 3, 1, null=(1,)),                  # ... and dA: its columns of dz
        _case(dt, 320, 4136, 32, 1, 1, ldp=960),                    # x is a column slice of wider rows
        _case(dt, 320, 1024, 32, 3, 0, ldq=3 * 64 + 40),            # Q rows wider than nmod * rp
        _case(dt, 320, 1024, 64, 1, 1, ldq=128),
        _case(dt, 320, 1024, 32, 1, 0, scale=0.375),
        _case(dt, 320, 1024, 32, 3, 1, scale=-2.5),
        _case(dt, 320, 1024, 32, 1, 0, half=160),                   # the GEGLU scatter: P's columns interleaved, out rows raw
        _case(dt, 2560, 1024, 32, 1, 0, half=1280),
        _case(dt, 320, 1024, 48, 3, 0, garbage=1.0e4),              # r = 48: 16 padding columns per module, loud
        _case(dt, 320, 1024, 48, 3, 1, garbage=1.0e4),
        _case(dt, 104, 154, 32, 3, 0),                              # sections of 104 channels: the second tile of each is ragged
        _case(dt, 312, 154, 32, 3, 1),
    ]


LONG = [_case("bf16", 320, 65536 + 8, 32, 1, mode) for mode in (0, 1)]  # level 0 at bs = 64: the slab count is capped, the slabs grow
ALL_CASES = GRID + GRID_F32 + _extras("bf16") + _extras("f32") + LONG


def _rp(dt, r):
    kt = 64 if dt == "bf16" else 32
    return (r + kt - 1) // kt * kt


@functools.lru_cache(maxsize=4)
def _draw(shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(DT[dt])


def _inputs(case):
    """-> P [M, ldp], Q [M, ldq] (T), priors (f32 or None per module), P in raw column order for the reference"""
    dt, Cc, M, r, nmod, mode, scale, ldp, ldq, null, garbage, half = case
    Ctot = Cc * nmod if (mode == 0 and not half) else Cc
    rp = _rp(dt, r)
    ldp, ldq = ldp or Ctot, ldq or nmod * rp
    P = _draw((M, ldp), dt, 701)
    Q = _draw((M, ldq), dt, 702)
    if garbage != 1.0:
        Q = Q.clone()
        for j in range(nmod):
            Q[:, j * rp + r:(j + 1) * rp] *= garbage
        Q[:, nmod * rp:] *= garbage
    raw = P[:, :Ctot]
    if half:  # P is the packed form of `raw`: raw column g * half + i lies at packed column (i >> 4) * 32 + (i & 15) + 16 g
        i = torch.arange(half)
        perm = torch.cat([(i >> 4) * 32 + (i & 15), (i >> 4) * 32 + (i & 15) + 16])
        P = torch.empty_like(raw)
        P[:, perm] = raw
    secN = Cc
    priors = [None if j in null else _draw((secN, r) if mode == 0 else (r, Cc), "f32", 710 + j) for j in range(nmod)]
    return P, Q, priors, raw, Ctot, secN, rp, ldp, ldq


def _ref(case, prec):
    dt, Cc, M, r, nmod, mode, scale = case[:7]
    P, Q, priors, raw, Ctot, secN, rp, _, _ = _inputs(case)
    Pp, Qp, outs = raw.to(prec), Q.to(prec), []
    for j in range(nmod):
        if priors[j] is None:
            outs.append(None)
            continue
        Qj = Qp[:, j * rp:j * rp + r]
        g = Pp[:, j * secN:(j + 1) * secN].t() @ Qj if mode == 0 else Qj.t() @ Pp
        outs.append(priors[j].to(prec) + scale * g)
    return outs


def _launch(case):
    from mrisr import ops
    dt, Cc, M, r, nmod, mode, scale, _, _, null, garbage, half = case
    P, Q, priors, raw, Ctot, secN, rp, ldp, ldq = _inputs(case)
    outs = [None if p is None else p.cuda().clone() for p in priors]   # pre-filled non-zero: the kernel adds into them
    ops.lora_wgrad_hr(P.cuda().contiguous(), Q.cuda().contiguous(), M, Ctot, mode, r, nmod, secN if mode == 0 else 320, outs, scale, ldp=ldp,
                      ldq=ldq, geglu_half=half)
    return outs


def _run(case, repeat=True):
    ref = _ref(case, F64)
    outs = _launch(case)
    name = "lora_wgrad_hr[%s C=%d M=%d r=%d nmod=%d mode=%d scale=%g ldp=%s ldq=%s null=%s garbage=%g half=%d]" % case
    for j, (got, want) in enumerate(zip(outs, ref)):
        assert (got is None) == (want is None)
        if got is None:
            continue
        want = want.cuda()
        got64 = got.to(F64)
        assert got64.shape == want.shape, (name, got64.shape, want.shape)
        assert bool(torch.isfinite(got64).all()), name
        l2 = float((got64 - want).norm() / want.norm().clamp_min(1e-30))
        worst = float((got64 - want).abs().max())
        print(f"{name}.out{j}: rel-L2 {l2:.3e} (<= {TOL:.1e})  max |d| {worst:.3e} (<= floor {FLOOR['lora.wgrad_hr']:.3e})")
        assert l2 <= TOL, (name, j, l2)
        assert worst <= FLOOR["lora.wgrad_hr"], (name, j, worst, FLOOR["lora.wgrad_hr"])
    if repeat:
        for _ in range(3):
            for a, b in zip(_launch(case), outs):
                if a is not None:
                    assert torch.equal(a, b), (name, "bits changed between launches")


def _prof(fn):
    """kernel classes (ProfScope names) launched by fn()"""
    from mrisr import _lib as L
    lib = L.lib()
    lib.mrisr_prof_reset(); lib.mrisr_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.mrisr_prof_enable(0)
    buf = C_.create_string_buffer(1 << 20)
    n = lib.mrisr_prof_report(buf, len(buf))
    classes = json.loads(buf.value[:n].decode())
    lib.mrisr_prof_reset()
    return set(classes)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d-M%d" % s)
@pytest.mark.parametrize("mode", [0, 1])
def test_lora_wgrad_hr_bf16(shape, mode):
    """r in {32, 48, 64, 128} x nmod in {1, 3}: rp = 64 / 64 / 64 / 128, so one or two 64-column blocks of Q per module; at C = 1280, r = 128,
    nmod = 3 dA meets 3 x 128 columns (six blocks) over 20 channel tiles; M = 4136 -> 17 slabs, the last of 40 rows"""
    mine = [c for c in GRID if (c[1], c[2]) == shape and c[5] == mode]
    assert len(mine) == 8
    for c in mine:
        _run(c)


def test_lora_wgrad_hr_f32():
    assert len(GRID_F32) == 8
    for c in GRID_F32:
        _run(c)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_lora_wgrad_hr_null_pitch_scale_geglu_padding(dt):
    for c in _extras(dt):
        _run(c)


def test_lora_wgrad_hr_64k_rows():
    """M = 65,544: 257 rows per slab round up to 288 -> 228 slabs"""
    for c in LONG:
        _run(c)


def test_lora_wgrad_hr_profiler_names():
    from mrisr import ops
    assert "lora_wgrad_hr" in _prof(lambda: _launch(_case("bf16", 64, 154, 32, 1, 0)))
    P = torch.zeros(154, 64, dtype=torch.bfloat16, device="cuda")
    Q = torch.zeros(154, 16, dtype=torch.float32, device="cuda")
    out = torch.zeros(64, 16, dtype=torch.float32, device="cuda")
    names = _prof(lambda: ops.lora_wgrad(P, Q, 154, 64, 0, 16, 1, 64, [out]))
    assert "lora_wgrad" in names and "lora_wgrad_hr" not in names, names


def test_lora_wgrad_hr_bad_arguments_are_refused():
    from mrisr import _lib as L
    from mrisr import ops
    bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device="cuda")
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    bad = [
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 64), 64, 320, 1, 16, 1, 320, [f32(16, 320)]),               # rank 16: the other entry point
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 64), 64, 320, 1, 20, 1, 320, [f32(20, 320)]),               # rank 20
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 64), 64, 320, 1, 40, 1, 320, [f32(40, 320)]),               # rank 40
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 192), 64, 320, 1, 144, 1, 320, [f32(144, 320)]),            # rank 144
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 64), 64, 320, 1, 32, 1, 320, [f32(32, 320)], ldp=312),      # P pitch below the row
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 128), 64, 320, 1, 32, 3, 320, [f32(32, 320)] * 3),          # ldq = 128 < 3 * 64
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 48), 64, 320, 1, 48, 1, 320, [f32(48, 320)]),               # ldq = r < rp
        lambda: ops.lora_wgrad_hr(f32(64, 320), f32(64, 48), 64, 320, 1, 48, 1, 320, [f32(48, 320)]),             # ... f32: rp = 64
        lambda: ops.lora_wgrad_hr(bf(64 * 320 + 8)[1:1 + 64 * 320].reshape(64, 320), bf(64, 64), 64, 320, 1, 32, 1, 320, [f32(32, 320)]),  # P 2 bytes off
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64 * 64 + 8)[1:1 + 64 * 64].reshape(64, 64), 64, 320, 1, 32, 1, 320, [f32(32, 320)]),    # Q 2 bytes off
        lambda: ops.lora_wgrad_hr(bf(64, 324), bf(64, 64), 64, 324, 1, 32, 1, 324, [f32(32, 324)]),               # C % 8
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 128), 64, 320, 0, 32, 2, 120, [f32(120, 32)] * 2),          # C != nmod * secN
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 64), 64, 320, 2, 32, 1, 320, [f32(32, 320)]),               # mode 2
        lambda: ops.lora_wgrad_hr(bf(64, 320), bf(64, 64), 64, 320, 0, 32, 1, 320, [f32(320, 32)], geglu_half=128),  # C != 2 * half
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(L.MrisrError):
            fn()
            pytest.fail(f"bad-argument case {i} was accepted")
    torch.cuda.synchronize()
    # ... and the process is still healthy
    _run(_case("bf16", 64, 154, 32, 1, 0), repeat=False)


def measure_floor():
    worst = 0.0
    for case in ALL_CASES:
        for a, b in zip(_ref(case, torch.float32), _ref(case, F64)):
            if a is not None:
                worst = max(worst, float((a.to(F64) - b).abs().max()))
    return worst


if __name__ == "__main__":
    torch.set_num_threads(8)
    w = measure_floor()
    print(f"    {'lora.wgrad_hr':<20s}{w:<28.3e}{8 * w:.3e}")
    print(f'MEASURED = {{"lora.wgrad_hr": {w:.3e}}}')
