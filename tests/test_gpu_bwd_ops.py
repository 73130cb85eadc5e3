"""GPU: every backward kernel on its own (csrc/bwd.hip, csrc/train_ops.h) through the mrisr_op_* entry points (csrc/capi_ops.hip), against
float64 autograd or the closed formula on the CPU.

Reference: inputs are drawn in f32 and rounded to the dtype under test; the reference is evaluated in float64 on those rounded inputs and
rounds nowhere else; where a kernel adds into an existing tensor the reference is ``prior + g``.

Assertions per output:
  * coarse: relative L2 <= 1e-3 (f32 outputs, which include every f32-accumulated LoRA / conv / bias / affine gradient of bf16 inputs) or
    1.2e-2 (bf16 outputs) - the bounds of tests/test_gpu_ops.py;
  * element-wise, no element excluded: |got - ref| <= r |ref| + floor, r = 2^-8 for a bf16 output (one round-to-nearest of an f32 result),
    r = 0 for an f32 output;
  * bits repeat over three more launches for the outputs built without atomics.

``floor`` stands for f32 arithmetic noise.  It is measured without a GPU and without the kernels: the same formula evaluated in plain torch
float32 on the CPU against the float64 reference, on this module's own inputs, largest absolute deviation over all cases of the output
class; the floor is 8 x that (a different summation order, the fast exp of silu_grad / gelu_grad).  ``python tests/test_gpu_bwd_ops.py``
prints the table again.

    output class        largest |f32 torch - f64|   floor (x 8)
    -------------------------------------------------------------
    conv.dgrad          2.425e-06                   1.940e-05
    conv.wgrad          3.710e-05                   2.968e-04
    conv.wgrad_bias     6.538e-06                   5.230e-05
    geglu.bwd           2.484e-06                   1.987e-05
    geglu.fwd           2.809e-06                   2.247e-05
    gn.affine           1.752e-04                   1.402e-03
    gn.dx               2.415e-06                   1.932e-05
    ln.affine           1.184e-04                   9.471e-04
    ln.dx               7.048e-07                   5.639e-06
    lora.wgrad          3.358e-04                   2.686e-03
    pw.colsum           1.784e-05                   1.427e-04
    pw.mse_grad         1.325e-08                   1.060e-07
    pw.mse_loss         2.912e-07                   2.329e-06
    pw.relu_bwd         0.000e+00                   0.000e+00
    pw.rowvec_grad      8.401e-06                   6.721e-05
    pw.silu_bwd         1.316e-06                   1.053e-05
    pw.sumpool2         8.941e-07                   7.153e-06
    small.dgrad         5.143e-06                   4.114e-05
    small.wgrad         1.141e-05                   9.131e-05
    softmax_bwd         1.401e-08                   1.121e-07
"""
import ctypes as C_
import functools
import json

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
TOL = {"f32": 1e-3, "bf16": 1.2e-2}   # tests/test_gpu_ops.py
F64 = torch.float64

# measured: largest |plain torch f32 - f64 reference| over the cases of the class (see the module docstring); the floor is 8 x this
MEASURED = {
    "conv.dgrad": 2.425e-06,
    "conv.wgrad": 3.710e-05,
    "conv.wgrad_bias": 6.538e-06,
    "geglu.bwd": 2.484e-06,
    "geglu.fwd": 2.809e-06,
    "gn.affine": 1.752e-04,
    "gn.dx": 2.415e-06,
    "ln.affine": 1.184e-04,
    "ln.dx": 7.048e-07,
    "lora.wgrad": 3.358e-04,
    "pw.colsum": 1.784e-05,
    "pw.mse_grad": 1.325e-08,
    "pw.mse_loss": 2.912e-07,
    "pw.relu_bwd": 0.000e+00,
    "pw.rowvec_grad": 8.401e-06,
    "pw.silu_bwd": 1.316e-06,
    "pw.sumpool2": 8.941e-07,
    "small.dgrad": 5.143e-06,
    "small.wgrad": 1.141e-05,
    "softmax_bwd": 1.401e-08,
}
FLOOR = {k: 8.0 * v for k, v in MEASURED.items()}


def _rnd(shape, dt, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(DT[dt])


def _leaf(t, prec):
    return t.detach().to(prec).clone().requires_grad_(True)


def _dev(t):
    return None if t is None else t.cuda().contiguous()


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


def _repeat(fn, first, n=3):
    for _ in range(n):
        again = fn()
        again = again if isinstance(again, (tuple, list)) else (again,)
        for a, b in zip(again, first if isinstance(first, (tuple, list)) else (first,)):
            if a is not None:
                assert torch.equal(a, b), "bits changed between launches"


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


# =====================================================================================================================
# GroupNorm backward
# =====================================================================================================================
def _gn_fused_geometry(c0, c1, groups, HW, ve):
    """csrc/norm.hip: gn_fused_geometry (the one-pass kernels' slab); None: two-kernel path"""
    Cc = c0 + c1
    Cg = Cc // groups
    base = Cg
    while base % ve:
        base += Cg
    if Cc % base:
        return None
    best, best_active = 0, 0
    f = 1
    while f * base <= 640 and f * base <= Cc:
        slab = f * base
        f += 1
        if Cc % slab or c0 % ve or c1 % ve:
            continue
        slots = slab // ve
        if slots > 256 or slab // Cg > 80:
            continue
        RL = min(256 // slots, HW)
        if (HW + RL - 1) // RL > 24:
            continue
        if slots * RL > best_active:
            best, best_active = slab, slots * RL
        if slots * RL >= 200:
            break
    return best or None


def _gn_branch(dt, B, c0, c1, HW, fused_on):
    """which kernels launch_groupnorm_bwd picks: ('fused', ve) or ('two', vpt)"""
    Cc = c0 + c1
    if dt == "bf16" and fused_on:
        slab = _gn_fused_geometry(c0, c1, 32, HW, 8)
        if slab:
            s4 = _gn_fused_geometry(c0, c1, 32, HW, 4) if B * (Cc // slab) < 512 else None
            return ("fused", 4 if s4 and Cc // s4 > Cc // slab else 8)
    nvec = Cc // (8 if dt == "bf16" else 4)
    vpt = 1
    while nvec // vpt > 256 or nvec % vpt:
        vpt += 1
    return ("two", vpt)


# the 14 geometries of test_gpu_ops.py::test_groupnorm_one_pass_kernel (group widths 2 ... 80, skip-concat split inside a slab, odd and
# non-square images, B a multiple of 8 and not), then:
#   (4, 1280, 0, 4, 4) / (2, 320, 320, 8, 8) / (3, 640, 0, 16, 16): B * nslab < 512 and the 4-wide slab is narrower -> the 8-byte-vector
#       variant (asserted below through _gn_branch, the arithmetic of launch_groupnorm_bwd);
#   C = 1920 / 2560: two-kernel widths (run with the one-pass kernel switched off): bf16 1920 -> 240 vectors, vpt 1; bf16 2560 -> 320
#       vectors, vpt 2; f32 2560 -> 640 vectors, vpt 4
GN_GEOM = [
    (8, 320, 0, 32, 32), (8, 320, 320, 32, 32), (3, 640, 0, 16, 16), (8, 1280, 640, 16, 16), (8, 640, 320, 16, 16), (8, 1280, 0, 8, 8),
    (16, 1280, 1280, 8, 8), (8, 1280, 640, 8, 8), (5, 1280, 0, 4, 4), (8, 1280, 1280, 4, 4), (8, 640, 320, 32, 32), (8, 64, 0, 5, 7),
    (2, 128, 128, 64, 64), (8, 512, 0, 24, 40),
    (4, 1280, 0, 4, 4), (2, 320, 320, 8, 8),
    (2, 1920, 0, 8, 8), (3, 1280, 1280, 4, 4), (2, 1280, 640, 6, 5),
]
GN_VE4 = [(5, 1280, 0, 4, 4), (4, 1280, 0, 4, 4), (2, 320, 320, 8, 8)]          # must select the 8-byte-vector one-pass kernel
GN_TWO = {(2, 1920, 0, 8, 8): 1, (3, 1280, 1280, 4, 4): 2}                      # bf16, one-pass off: vpt
GN_F32 = [(3, 640, 0, 16, 16), (8, 64, 0, 5, 7), (2, 320, 320, 8, 8), (3, 1280, 1280, 4, 4), (2, 1280, 640, 6, 5), (8, 640, 320, 16, 16)]
GN_F32_VPT = {(3, 1280, 1280, 4, 4): 4, (2, 1280, 640, 6, 5): 2, (3, 640, 0, 16, 16): 1}


@functools.lru_cache(maxsize=4)
def _gn_inputs(dt, B, c0, c1, H, W):
    HW = H * W
    x = _rnd((B, HW, c0), dt, 201, 1.7, 0.3)
    x2 = _rnd((B, HW, c1), dt, 202, 0.6, -1.0) if c1 else None
    dy = _rnd((B, HW, c0 + c1), dt, 203)
    gamma, beta = 1 + 0.2 * _rnd((c0 + c1,), "f32", 204), 0.2 * _rnd((c0 + c1,), "f32", 205)
    p0, p1 = _rnd((B, HW, c0), dt, 206), (_rnd((B, HW, c1), dt, 207) if c1 else None)
    pg, pb = _rnd((c0 + c1,), "f32", 208), _rnd((c0 + c1,), "f32", 209)
    return x, x2, dy, gamma, beta, p0, p1, pg, pb


@torch.enable_grad()   # other test modules switch autograd off process-wide when they are imported
def _gn_ref(inp, silu, prec):
    """autograd of [SiLU o] GroupNorm(32 groups, eps 1e-5) in `prec`: (dx over all channels, g_gamma, g_beta)"""
    x, x2, dy, gamma, beta = inp[:5]
    xc = _leaf(x if x2 is None else torch.cat([x, x2], 2), prec)
    ga, be = _leaf(gamma, prec), _leaf(beta, prec)
    y = F.group_norm(xc.transpose(1, 2), 32, ga, be, 1e-5)
    if silu:
        y = F.silu(y)
    y.backward(dy.to(prec).transpose(1, 2))
    return xc.grad, ga.grad, be.grad


def _gn_run(dt, geom, check):
    from mrisr import _lib as L
    from mrisr import ops
    B, c0, c1, H, W = geom
    inp = _gn_inputs(dt, *geom)
    x, x2, dy, gamma, beta, p0, p1, pg, pb = inp
    x_, x2_, dy_, ga_, be_ = _dev(x), _dev(x2), _dev(dy), _dev(gamma), _dev(beta)
    xcat_ = x_ if x2 is None else torch.cat([x_, x2_], 2).contiguous()
    lib = L.lib()
    try:
        for silu in (True, False):
            rdx, rgg, rgb = _gn_ref(inp, silu, F64)
            for fused_on in ((1, 0) if dt == "bf16" else (1,)):
                lib.mrisr_debug_gn_fused(C_.c_int(fused_on))
                branch = _gn_branch(dt, B, c0, c1, H * W, fused_on)
                for acc0, acc1 in ((0, 0), (1, 1), (1, 0), (0, 1)):
                    if c1 == 0 and acc1:
                        continue
                    def run():
                        o0 = _dev(p0).clone() if acc0 else torch.full_like(x_, float("nan"))
                        o1 = None if x2 is None else (_dev(p1).clone() if acc1 else torch.full_like(x2_, float("nan")))
                        return ops.groupnorm_backward(x_, dy_, ga_, be_, 32, 1e-5, silu, x2=x2_, dx=o0, dx2=o1, acc=acc0, acc2=acc1)
                    if (acc0, acc1) == (0, 0):
                        classes = _prof(run)
                        want = {"groupnorm_bwd_fused"} if branch[0] == "fused" else {"groupnorm_bwd_stats", "groupnorm_bwd_apply"}
                        assert want <= classes and not ({"groupnorm_bwd_fused", "groupnorm_bwd_stats"} - want) & classes, (branch, classes)
                    g0, g1 = run()
                    tag = f"gn_bwd[{dt} {geom} silu={int(silu)} {branch} acc={acc0}{acc1}]"
                    check("gn.dx", tag + ".dx0", g0, rdx[:, :, :c0] + (p0.to(F64) if acc0 else 0), dt)
                    if c1:
                        check("gn.dx", tag + ".dx1", g1, rdx[:, :, c0:] + (p1.to(F64) if acc1 else 0), dt)
                    _repeat(run, (g0, g1))
            # affine gradients (full-parameter training): the single-source form the trainer uses, added into non-zero tensors
            gg, gb = _dev(pg).clone(), _dev(pb).clone()
            ops.groupnorm_backward(xcat_, dy_, ga_, be_, 32, 1e-5, silu, g_gamma=gg, g_beta=gb)
            check("gn.affine", f"gn_bwd[{dt} {geom} silu={int(silu)}].g_gamma", gg, rgg + pg.to(F64), "f32")
            check("gn.affine", f"gn_bwd[{dt} {geom} silu={int(silu)}].g_beta", gb, rgb + pb.to(F64), "f32")
    finally:
        lib.mrisr_debug_gn_fused(C_.c_int(1))


@pytest.mark.parametrize("geom", GN_GEOM, ids=str)
def test_groupnorm_backward_bf16(geom):
    B, c0, c1, H, W = geom
    if geom in GN_VE4:
        assert _gn_branch("bf16", B, c0, c1, H * W, 1) == ("fused", 4) and B * ((c0 + c1) // _gn_fused_geometry(c0, c1, 32, H * W, 8)) < 512
    if geom in GN_TWO:
        assert _gn_branch("bf16", B, c0, c1, H * W, 0) == ("two", GN_TWO[geom])
    _gn_run("bf16", geom, _check)


@pytest.mark.parametrize("geom", GN_F32, ids=str)
def test_groupnorm_backward_f32(geom):
    B, c0, c1, H, W = geom
    if geom in GN_F32_VPT:
        assert _gn_branch("f32", B, c0, c1, H * W, 1) == ("two", GN_F32_VPT[geom])
    _gn_run("f32", geom, _check)


# =====================================================================================================================
# LayerNorm backward
# =====================================================================================================================
# MAXV = ceil(C / VE / 64), VE = 8 (bf16) / 4 (f32): bf16 320 -> 1, 1024 -> 2, 1280 -> 3, 2560 -> 5;  f32 64 -> 1, 320 -> 2, 640 -> 3, 1280 -> 5
LN_CASES = [("bf16", c) for c in (320, 1024, 1280, 2560)] + [("f32", c) for c in (64, 320, 640, 1280)]
LN_M = (7, 33, 4099)
LN_AFF_C, LN_AFF_M = (64, 320, 1280, 1536), (1, 31, 33, 4100)


def _ln_inputs(dt, M, Cc):
    return (_rnd((M, Cc), dt, 301, 2.0, 0.5), _rnd((M, Cc), dt, 302), 1 + 0.2 * _rnd((Cc,), "f32", 303), _rnd((M, Cc), dt, 304),
            _rnd((Cc,), "f32", 305), _rnd((Cc,), "f32", 306))


@torch.enable_grad()   # other test modules switch autograd off process-wide when they are imported
def _ln_ref(inp, prec):
    x, dy, gamma = inp[:3]
    xc, ga = _leaf(x, prec), _leaf(gamma, prec)
    be = _leaf(torch.zeros_like(gamma), prec)
    F.layer_norm(xc, (x.shape[1],), ga, be, 1e-5).backward(dy.to(prec))
    return xc.grad, ga.grad, be.grad


@pytest.mark.parametrize("dt,Cc", LN_CASES)
def test_layernorm_backward(dt, Cc):
    from mrisr import ops
    for M in LN_M:
        inp = _ln_inputs(dt, M, Cc)
        x, dy, gamma, prior = inp[:4]
        rdx = _ln_ref(inp, F64)[0]
        x_, dy_, ga_ = _dev(x), _dev(dy), _dev(gamma)
        for acc in (0, 1):
            def run():
                o = _dev(prior).clone() if acc else torch.full_like(x_, float("nan"))
                return ops.layernorm_backward(x_, dy_, ga_, 1e-5, dx=o, acc=acc)
            got = run()
            _check("ln.dx", f"ln_bwd[{dt} M={M} C={Cc} acc={acc}]", got, rdx + (prior.to(F64) if acc else 0), dt)
            _repeat(run, got)
        assert "layernorm_bwd" in _prof(run)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("Cc", LN_AFF_C)
def test_layernorm_affine_grad(dt, Cc):
    from mrisr import ops
    for M in LN_AFF_M:
        inp = _ln_inputs(dt, M, Cc)
        x, dy, gamma, _, pg, pb = inp
        _, rgg, rgb = _ln_ref(inp, F64)
        gg, gb = _dev(pg).clone(), _dev(pb).clone()
        ops.layernorm_backward(_dev(x), _dev(dy), _dev(gamma), 1e-5, g_gamma=gg, g_beta=gb, need_dx=(dt == "bf16" or Cc <= 1280))
        _check("ln.affine", f"ln_affine[{dt} M={M} C={Cc}].g_gamma", gg, rgg + pg.to(F64), "f32")
        _check("ln.affine", f"ln_affine[{dt} M={M} C={Cc}].g_beta", gb, rgb + pb.to(F64), "f32")


# =====================================================================================================================
# GEGLU on the interleaved pre-activation
# =====================================================================================================================
GEGLU_CASES = [(256, 1037), (1280, 259), (2560, 131), (5120, 67)]   # (half, ragged M)


def _il(nat):
    """natural [M][u | g] -> the projection's packed layout: 16 value columns, then their 16 gate columns, and so on"""
    M, two = nat.shape
    half = two // 2
    return torch.stack([nat[:, :half].reshape(M, half // 16, 16), nat[:, half:].reshape(M, half // 16, 16)], 2).reshape(M, two).contiguous()


def _unil(pk):
    M, two = pk.shape
    v = pk.reshape(M, two // 32, 2, 16)
    return torch.cat([v[:, :, 0].reshape(M, two // 2), v[:, :, 1].reshape(M, two // 2)], 1)


def _geglu_inputs(dt, half, M):
    return _rnd((M, 2 * half), dt, 401, 1.5), _rnd((M, half), dt, 402)


@torch.enable_grad()   # other test modules switch autograd off process-wide when they are imported
def _geglu_ref(inp, prec):
    pre, dout = inp
    nat = _leaf(_unil(pre), prec)
    half = dout.shape[1]
    out = nat[:, :half] * F.gelu(nat[:, half:])
    out.backward(dout.to(prec))
    return out.detach(), _il(nat.grad)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("half,M", GEGLU_CASES)
def test_geglu_forward_backward(dt, half, M):
    from mrisr import ops
    inp = _geglu_inputs(dt, half, M)
    rout, rdpre = _geglu_ref(inp, F64)
    pre_, dout_ = _dev(inp[0]), _dev(inp[1])
    out = ops.geglu(pre_)
    _check("geglu.fwd", f"geglu_fwd[{dt} half={half} M={M}]", out, rout, dt)
    dpre = ops.geglu(pre_, dout_)
    _check("geglu.bwd", f"geglu_bwd[{dt} half={half} M={M}]", dpre, rdpre, dt)
    _repeat(lambda: ops.geglu(pre_), out)
    _repeat(lambda: ops.geglu(pre_, dout_), dpre)
    assert "geglu_bwd" in _prof(lambda: ops.geglu(pre_, dout_))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_geglu_layout_is_the_gemm_epilogues(dt):
    """geglu_fwd on the interleaved pre-activation == the GEGLU epilogue of the projection GEMM on the same operands: ties the
    (de)interleave of this module to the packed layout of ff.net.0.proj (bound: the forward test's)."""
    from mrisr import _lib as L
    from mrisr import ops
    M, K, half = 200, 320, 1280
    x, w, b = _rnd((M, K), dt, 411), _rnd((2 * half, K), "f32", 412, K ** -0.5), _rnd((2 * half,), "f32", 413)
    fused = ops.linear(_dev(x), _dev(w), _dev(b), act=L.ACT_GEGLU)
    pre_nat = ops.linear(_dev(x), _dev(w), _dev(b))                 # [M][u | g], rounded to dt as the training step stores it
    mine = ops.geglu(_il(pre_nat))
    err = float((mine.double() - fused.double()).norm() / fused.double().norm())
    print(f"geglu_fwd(interleave(pre)) vs linear(act=GEGLU) [{dt}]: rel-L2 {err:.3e}")
    assert err < TOL[dt]
    # and a wrong interleave is far away (the check has teeth)
    wrong = ops.geglu(pre_nat.contiguous())
    assert float((wrong.double() - fused.double()).norm() / fused.double().norm()) > 0.5


# =====================================================================================================================
# the pointwise / reduction group
# =====================================================================================================================
PW_BIG = 8192 * 256 + 12345      # above one full grid (8192 blocks x 256 threads): the grid-stride loop iterates
PW_SIZES = (1, 255, 2049, 70001, PW_BIG)


def _silu_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_silu_relu_backward(dt):
    from mrisr import ops
    for n in PW_SIZES:
        dy, pre = _rnd((n,), dt, 501), _rnd((n,), dt, 502, 2.0)
        dy_, pre_ = _dev(dy), _dev(pre)
        for kind, key, ref in ((ops.PW_SILU_BWD, "pw.silu_bwd", dy.to(F64) * _silu_grad(pre.to(F64))),
                               (ops.PW_RELU_BWD, "pw.relu_bwd", torch.where(pre.to(F64) > 0, dy.to(F64), torch.zeros((), dtype=F64)))):
            def run():
                out = torch.full_like(dy_, float("nan"))
                ops.pointwise_backward(kind, dy_, pre_, out=out, n=n)
                return out
            got = run()
            _check(key, f"{key}[{dt} n={n}]", got, ref, dt)
            _repeat(run, got)


SUMPOOL_CASES = [(2, 3, 5, 37), (1, 8, 8, 320), (3, 7, 4, 1), (1, 64, 65, 129)]   # (B, H, W, C): odd C, odd extents


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_sumpool2(dt):
    from mrisr import ops
    for B, H, W, Cc in SUMPOOL_CASES:
        src, prior = _rnd((B, 2 * H, 2 * W, Cc), dt, 511), _rnd((B, H, W, Cc), dt, 512)
        ref = src.to(F64).reshape(B, H, 2, W, 2, Cc).sum((2, 4))
        src_ = _dev(src)
        for acc in (0, 1):
            def run():
                out = _dev(prior).clone() if acc else torch.full_like(_dev(prior), float("nan"))
                ops.pointwise_backward(ops.PW_SUMPOOL2, src_, out=out, B=B, H=H, W=W, Cc=Cc, flag=acc)
                return out
            got = run()
            _check("pw.sumpool2", f"sumpool2[{dt} {(B, H, W, Cc)} acc={acc}]", got, ref + (prior.to(F64) if acc else 0), dt)
            _repeat(run, got)


MSE_CASES = [(2, 4, 16, 16), (3, 5, 7, 9), (1, 4, 3, 3), (5, 4, 64, 64), (2, 3, 512, 517)]   # the last: 1.59 M > 1024 x 256: the loop iterates


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_mse_grad(dt):
    from mrisr import ops
    for B, Cc, H, W in MSE_CASES:
        pred, tgt = _rnd((B, H, W, Cc), dt, 521), _rnd((B, Cc, H, W), "f32", 522)
        d = pred.to(F64) - tgt.to(F64).permute(0, 2, 3, 1)
        pred_, tgt_ = _dev(pred), _dev(tgt)
        def run():
            out, loss = torch.full_like(pred_, float("nan")), torch.full((1,), 7.0, device="cuda")
            ops.pointwise_backward(ops.PW_MSE_GRAD, pred_, tgt_, out=out, out_f32=loss, B=B, H=H, W=W, Cc=Cc)
            return out, loss
        got, loss = run()
        _check("pw.mse_grad", f"mse_grad[{dt} {(B, Cc, H, W)}].dpred", got, 2 * d / d.numel(), dt)
        _check("pw.mse_loss", f"mse_grad[{dt} {(B, Cc, H, W)}].loss", loss, (d * d).mean().reshape(1), "f32")
        _repeat(lambda: run()[0], got)


ROWVEC_CASES = [(1, 64, 320, 0, 0), (5, 35, 77, 0, 3), (5, 35, 77, 1, 3), (1, 9, 1280, 1, 64), (5, 256, 640, 0, 128)]  # (B, HW, C, scalar_t, off)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_rowvec_grad_and_colsum(dt):
    from mrisr import ops
    for B, HW, Cc, scalar_t, off in ROWVEC_CASES:
        dh = _rnd((B, HW, Cc), dt, 531)
        ld = off + Cc + 5
        prior = _rnd((B, ld), "f32", 532)
        ref = prior.to(F64).clone()
        s = dh.to(F64).sum(1)
        if scalar_t:
            ref[0, off:off + Cc] += s.sum(0)
        else:
            ref[:, off:off + Cc] += s
        out = _dev(prior).clone()
        ops.pointwise_backward(ops.PW_ROWVEC_GRAD, _dev(dh), out_f32=out, B=B, H=HW, W=1, Cc=Cc, flag=scalar_t, ld_out=ld, off=off)
        _check("pw.rowvec_grad", f"rowvec_grad[{dt} {(B, HW, Cc, scalar_t, off)}]", out, ref, "f32")
    for M, Cc in ((1, 64), (513, 77), (2050, 320), (4099, 1)):
        dy, prior = _rnd((M, Cc), dt, 541), _rnd((Cc,), "f32", 542)
        out = _dev(prior).clone()
        ops.pointwise_backward(ops.PW_COLSUM, _dev(dy), out_f32=out, B=1, H=M, W=1, Cc=Cc)
        _check("pw.colsum", f"colsum[{dt} M={M} C={Cc}]", out, prior.to(F64) + dy.to(F64).sum(0), "f32")


# =====================================================================================================================
# LoRA weight gradients
# =====================================================================================================================
LORA_C = (64, 320, 640, 960, 1280, 2560, 5120)
LORA_M = (154, 1024, 4096 + 40)


def _lora_geom(dt, M, Cc):
    """csrc/bwd.hip: lora_wgrad_geom -> (gx, cxb, RL, rpb, gy, re-slabbed)"""
    ve = 8 if dt == "bf16" else 4
    cx = Cc // ve
    gx = (cx + 255) // 256
    cxb = (cx + gx - 1) // gx
    RL = 256 // cxb
    rpb = RL * 16
    gy = (M + rpb - 1) // rpb
    re = gy > 512
    if re:
        rpb = ((M + 511) // 512 + RL - 1) // RL * RL
        gy = (M + rpb - 1) // rpb
    return gx, cxb, RL, rpb, gy, re


def _lora_cases():
    """r x nmod x mode for every width, the row counts rotating through LORA_M (every (C, M) pair occurs); mode 0 needs C = nmod sections
    of whole vectors.  nmod * r = 24 / 36 / 48 in mode 1: one pass per module (nmod * r > 16)."""
    cases, i = [], 0
    for Cc in LORA_C:
        for r in (4, 8, 12, 16):
            for nmod in (1, 2, 3):
                for mode in (0, 1):
                    if mode == 0 and (Cc % nmod or (Cc // nmod) % 8):
                        continue
                    cases.append((Cc, r, nmod, mode, LORA_M[i % 3]))
                    i += 1
    return cases


LORA_CASES = _lora_cases()


@functools.lru_cache(maxsize=3)
def _lora_P(dt, M, ldp):
    return _rnd((M, ldp), dt, 601)


@functools.lru_cache(maxsize=8)
def _lora_Q(M, ldq):
    return _rnd((M, ldq), "f32", 602)


def _lora_ref(P, Q, Cc, mode, r, nmod, secN, scale, priors, prec):
    Pp, Qp, outs = P[:, :Cc].to(prec), Q.to(prec), []
    for j in range(nmod):
        if priors[j] is None:
            outs.append(None)
            continue
        Qj = Qp[:, j * r:(j + 1) * r]
        g = Pp[:, j * secN:(j + 1) * secN].t() @ Qj if mode == 0 else Qj.t() @ Pp
        outs.append(priors[j].to(prec) + scale * g)
    return outs


def _lora_priors(Cc, mode, r, nmod, secN, null=()):
    return [None if j in null else _rnd((secN, r) if mode == 0 else (r, Cc), "f32", 610 + j) for j in range(nmod)]


def _lora_run(dt, Cc, r, nmod, mode, M, scale=1.0, ldp=None, ldq=None, null=(), check=None):
    from mrisr import ops
    secN = Cc // nmod if mode == 0 else 320
    ldp, ldq = ldp or Cc, ldq or nmod * r
    P, Q = _lora_P(dt, M, ldp), _lora_Q(M, ldq)
    priors = _lora_priors(Cc, mode, r, nmod, secN, null)
    ref = _lora_ref(P, Q, Cc, mode, r, nmod, secN, scale, priors, F64)
    outs = [None if p is None else _dev(p).clone() for p in priors]      # pre-filled non-zero: the kernel adds into them
    ops.lora_wgrad(_dev(P), _dev(Q), M, Cc, mode, r, nmod, secN, outs, scale, ldp=ldp, ldq=ldq)
    for j in range(nmod):
        if outs[j] is not None:
            _check("lora.wgrad", f"lora_wgrad[{dt} C={Cc} r={r} nmod={nmod} mode={mode} M={M} geom={_lora_geom(dt, M, Cc)}].out{j}", outs[j], ref[j], "f32")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("Cc", LORA_C)
def test_lora_wgrad(dt, Cc):
    """bf16: C = 64 / 320 / 640 -> RL = 32 / 6 / 3 (LDS fold); 960 -> cxb 120, RL 2; 1280 -> cxb 160, RL 1 (plain stores); 2560 -> gx 2, cxb 160;
    5120 -> gx 3, cxb 214 (the last block has 2 dead chunks).  f32 (4-wide vectors): RL = 1 from C = 640, gx = 2 / 3 / 5 at 1280 / 2560 / 5120."""
    mine = [c for c in LORA_CASES if c[0] == Cc and (dt == "bf16" or (c[1] in (4, 16) and c[2] in (1, 3)))]
    assert mine
    for (_, r, nmod, mode, M) in mine:
        _lora_run(dt, Cc, r, nmod, mode, M)
    g = _lora_geom(dt, 154, Cc)
    if dt == "bf16":
        assert (g[2] > 1) == (Cc < 1280) and (g[0] > 1) == (Cc > 2048), g


def test_lora_wgrad_branches_are_all_reached():
    assert {(r, nmod, mode) for (_, r, nmod, mode, _) in LORA_CASES} == {(r, n, m) for r in (4, 8, 12, 16) for n in (1, 2, 3) for m in (0, 1)}
    assert {(c, m) for (c, _, _, _, m) in LORA_CASES} == {(c, m) for c in LORA_C for m in LORA_M}
    assert {n * r for (_, r, n, mode, _) in LORA_CASES if mode == 1} >= {4, 8, 12, 16, 24, 36, 48}


def test_lora_wgrad_reslab_64k_rows():
    """level 0 at bs = 64: M = 65,536 + 8 rows of C = 320 bf16: RL 6, 96 rows per block -> gy = 683 > 512 -> re-slab to 132 rows, gy = 497"""
    assert _lora_geom("bf16", 65536 + 8, 320) == (1, 40, 6, 132, 497, True)
    for mode in (0, 1):
        _lora_run("bf16", 320, 4, 1, mode, 65536 + 8)
    _lora_run("bf16", 320, 4, 3, 1, 65536 + 8)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_lora_wgrad_null_pitch_scale(dt):
    _lora_run(dt, 960, 4, 3, 0, 1024, null=(1,))                   # no adapter on the middle module (mode 0: section 1 of dY skipped)
    _lora_run(dt, 320, 8, 3, 1, 154, null=(1,))                    # ... and in the per-module passes of dA (nmod * r = 24)
    _lora_run(dt, 320, 4, 2, 1, 1024, null=(0,))
    _lora_run(dt, 320, 4, 1, 1, 4136, ldp=960)                     # x is a column slice of wider rows (ldp > C)
    _lora_run(dt, 640, 4, 2, 0, 154, ldp=1928, ldq=16)             # dY / z pitches beyond the operand
    _lora_run(dt, 320, 4, 1, 0, 1024, scale=0.375)
    _lora_run(dt, 1280, 16, 2, 1, 154, scale=-2.5)
    assert "lora_wgrad" in _prof(lambda: _lora_run(dt, 64, 4, 1, 0, 154))


# =====================================================================================================================
# transpose, softmax backward
# =====================================================================================================================
# (R, C, ld_src, ld_dst, batch, r_valid): multiples of the 16-byte vector everywhere -> transpose_vec_kernel (64 x 64 tiles, ragged against the
# tile); anything odd -> the 32 x 32 scalar kernel
TR_CASES = [(64, 64, 64, 64, 1, 64), (200, 72, 72, 200, 1, 200), (77, 40, 40, 77, 1, 77), (1280, 320, 320, 1280, 1, 1280),
            (128, 64, 64, 128, 6, 77), (136, 40, 48, 144, 5, 130), (33, 65, 70, 40, 3, 20), (64, 128, 128, 64, 4, 0), (1, 1, 1, 1, 1, 1)]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_transpose(dt):
    from mrisr import ops
    for R, Cc, lds, ldd, batch, rv in TR_CASES:
        ve = 8 if dt == "bf16" else 4
        bs_s, bs_d = R * lds + (0 if R % ve == 0 and lds % ve == 0 else 3), Cc * ldd
        src = _rnd((batch * bs_s + 8,), dt, 701)
        ref = torch.full((batch, Cc, ldd), -7.0, dtype=F64)                      # pitch padding must stay untouched
        for z in range(batch):
            m = src[z * bs_s:z * bs_s + R * lds].reshape(R, lds)[:, :Cc].to(F64).clone()
            m[rv:] = 0
            ref[z, :, :R] = m.t()
        src_ = _dev(src)
        def run():
            dst = torch.full((batch, Cc, ldd), -7.0, dtype=DT[dt], device="cuda")
            ops.transpose(src_, dst, R, Cc, lds, ldd, bs_s, bs_d, batch, rv)
            return dst
        got = run()
        assert torch.equal(got.double().cpu(), ref), (dt, R, Cc, lds, ldd, batch, rv)   # a copy: exact
        _repeat(run, got)
    assert "transpose" in _prof(run)


# key counts 16 / 77 / 256 / 1024 in head buffers padded to 64 (ld % 4 == 0, ld <= 4096: softmax_bwd_vec_kernel, MAXV = ceil(ld / 256) ->
# 1, 1, 1, 4), 300 / 2000 / 4096 (MAXV 2, 8, 16); ld = 77 (odd pitch) and ld = 4160 > 4096: softmax_bwd_kernel (scalar)
SM_CASES = [(16, 64, 37), (77, 128, 203), (256, 256, 64), (1024, 1024, 9), (300, 320, 50), (2000, 2048, 7), (4096, 4096, 5), (77, 77, 41),
            (4100, 4160, 6), (3, 6, 2)]


def _sm_inputs(dt, nk, ld, rows):
    p = torch.softmax(_rnd((rows, nk), "f32", 711, 2.0).float(), -1)
    P = torch.cat([p, _rnd((rows, ld - nk), "f32", 712)], 1).to(DT[dt])        # pad columns hold garbage: the kernel must not use them
    return P.contiguous(), _rnd((rows, ld), "f32", 713)


def _sm_ref(inp, nk, scale, prec):
    P, dP = inp[0].to(prec), inp[1].to(prec)
    out = torch.zeros_like(P)
    p, d = P[:, :nk], dP[:, :nk]
    out[:, :nk] = scale * p * (d - (d * p).sum(-1, keepdim=True))
    return out


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_softmax_backward(dt):
    from mrisr import ops
    for nk, ld, rows in SM_CASES:
        inp = _sm_inputs(dt, nk, ld, rows)
        P_, dP_ = _dev(inp[0]), _dev(inp[1])
        got = ops.softmax_backward(P_, dP_, nk, 0.125)
        _check("softmax_bwd", f"softmax_bwd[{dt} nk={nk} ld={ld} rows={rows}]", got, _sm_ref(inp, nk, 0.125, F64), dt)
        _repeat(lambda: ops.softmax_backward(P_, dP_, nk, 0.125), got)
    assert "softmax_bwd" in _prof(lambda: ops.softmax_backward(P_, dP_, nk, 0.125))


# =====================================================================================================================
# the tiny dense layers of the time-embedding MLP
# =====================================================================================================================
def _small_inputs(wdt, rows, N, K):
    return (_rnd((rows, N + 3), "f32", 801), _rnd((rows, K + 5), "f32", 802), _rnd((N, K), wdt, 803, K ** -0.5), _rnd((rows, K + 2), "f32", 804),
            _rnd((N, K), "f32", 805), _rnd((N,), "f32", 806))


def _small_ref(inp, N, K, silu_in, use_pre, prec):
    dY, X, Wt, pre, pW, pB = (t.to(prec) for t in inp)
    xa = X[:, :K]
    if silu_in:
        xa = xa * torch.sigmoid(xa)
    gW = pW + dY[:, :N].t() @ xa
    gB = pB + dY[:, :N].sum(0)
    dX = dY[:, :N] @ Wt
    if use_pre:
        dX = dX * _silu_grad(pre[:, :K])
    return gW, gB, dX


SMALL_SHAPES = [(320, 64), (1280, 320), (77, 129)]   # (N, K)


@pytest.mark.parametrize("wdt", ["bf16", "f32"])
@pytest.mark.parametrize("rows", [1, 2, 64])
def test_small_dense_backward(wdt, rows):
    from mrisr import ops
    for N, K in SMALL_SHAPES:
        inp = _small_inputs(wdt, rows, N, K)
        dY, X, Wt, pre, pW, pB = inp
        for silu_in, use_pre in ((0, 0), (1, 1)):
            rW, rB, rX = _small_ref(inp, N, K, silu_in, use_pre, F64)
            gW, gB = _dev(pW).clone(), _dev(pB).clone()
            ops.small_wgrad(_dev(dY), _dev(X), N, K, gW, gB if silu_in else None, silu_in=bool(silu_in))
            tag = f"[{wdt} rows={rows} N={N} K={K} silu/pre={silu_in}]"
            _check("small.wgrad", "small_wgrad" + tag + ".gW", gW, rW, "f32")
            if silu_in:
                _check("small.wgrad", "small_wgrad" + tag + ".gB", gB, rB, "f32")
            else:
                assert torch.equal(gB.cpu(), pB)                    # gB NULL: untouched
            dX = ops.small_dgrad(_dev(dY), _dev(Wt), N, K, pre=_dev(pre) if use_pre else None)
            _check("small.dgrad", "small_dgrad" + tag, dX, rX, "f32")


# =====================================================================================================================
# conv / linear weight gradients (the wgrad composite of the training step)
# =====================================================================================================================
# (B, Cin, Cout, ks, stride, H, W)
WG_CONV = [(2, 3, 16, 3, 1, 16, 16),      # 27 im2col columns pad to 28 (one zero column)
           (2, 4, 320, 3, 1, 8, 8), (2, 16, 32, 3, 2, 16, 16), (2, 320, 320, 3, 1, 8, 8),
           (3, 64, 96, 1, 1, 5, 7)]       # M = 105: not a multiple of 64 (zero-padded pixel columns)


def _wg_inputs(dt, B, cin_src, ldy, H, W, Ho, Wo):
    return _rnd((B, H, W, cin_src), dt, 901), _rnd((B * Ho * Wo, ldy), dt, 902)


@torch.enable_grad()   # other test modules switch autograd off process-wide when they are imported
def _wg_ref(x, dy_nat, B, Ho, Wo, ks, stride, cout, cin, pW, pB, prec):
    """dy_nat: [M][cout_src] columns already cut out / de-interleaved; autograd of conv2d with respect to the weight, cut to the raw tensor"""
    xs = x.to(prec).permute(0, 3, 1, 2)
    w = torch.zeros((dy_nat.shape[1], x.shape[3], ks, ks), dtype=prec, requires_grad=True)
    y = F.conv2d(xs, w, padding=ks // 2, stride=stride)
    d = dy_nat.to(prec).reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2)
    y.backward(d)
    return pW.to(prec) + w.grad[:cout, :cin], pB.to(prec) + d.sum((0, 2, 3))[:cout]


def _wg_run(dt, x, dY, B, Ho, Wo, ks, stride, col0, cout_src, cout, cin, geglu_half, bias, name):
    from mrisr import ops
    pW, pB = _rnd((cout, cin, ks, ks), "f32", 903), _rnd((cout,), "f32", 904)
    nat = dY[:, col0:col0 + cout_src]
    if geglu_half:
        nat = _unil(nat)
    rW, rB = _wg_ref(x, nat, B, Ho, Wo, ks, stride, cout, cin, pW, pB, F64)
    gW, gB = _dev(pW).clone(), _dev(pB).clone()
    ops.conv_wgrad(_dev(x), _dev(dY), gW, gB if bias else None, ks=ks, stride=stride, col0=col0, cout_src=cout_src, cout=cout, cin=cin,
                   geglu_half=geglu_half)
    _check("conv.wgrad", name + ".gW", gW, rW, "f32")
    if bias:
        _check("conv.wgrad_bias", name + ".gB", gB, rB, "f32")
    else:
        assert torch.equal(gB.cpu(), pB)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", WG_CONV, ids=str)
def test_conv_wgrad(dt, case):
    B, cin, cout, ks, stride, H, W = case
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, dY = _wg_inputs(dt, B, cin, cout, H, W, Ho, Wo)
    for bias in (1, 0):
        _wg_run(dt, x, dY, B, Ho, Wo, ks, stride, 0, cout, cout, cin, 0, bias, f"conv_wgrad[{dt} {case} bias={bias}]")
    if case[1] == 3:
        assert "im2col_all_T" in _prof(lambda: _wg_run(dt, x, dY, B, Ho, Wo, ks, stride, 0, cout, cout, cin, 0, 1, "conv_wgrad[prof]"))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_linear_wgrad_sections_geglu_padding(dt):
    # a fused qkv projection: the gradient of the middle module reads columns secN .. 2 secN of rows of pitch 3 secN
    M, K, secN = 200, 320, 320
    x, dY = _wg_inputs(dt, 1, K, 3 * secN, M, 1, M, 1)
    for col0 in (secN, 2 * secN, 0):
        _wg_run(dt, x, dY, 1, M, 1, 1, 1, col0, secN, secN, K, 0, 1, f"linear_wgrad[{dt} qkv col0={col0}]")
    # ff.net.0.proj: dY rows in the GEGLU interleave, gradient rows in PyTorch's [u | g] order
    half = 640
    x, dY = _wg_inputs(dt, 1, 320, 2 * half, 131, 1, 131, 1)
    for bias in (1, 0):
        _wg_run(dt, x, dY, 1, 131, 1, 1, 1, 0, 2 * half, 2 * half, 320, half, bias, f"linear_wgrad[{dt} geglu half={half} bias={bias}]")
    # zero-padded layers (the condition embedding: 3 -> 16 channels stored as 64 / 64): raw tensor smaller than the stored activations
    B, H, W = 2, 8, 8
    x, dY = _wg_inputs(dt, B, 64, 64, H, W, H, W)
    _wg_run(dt, x, dY, B, H, W, 3, 1, 0, 64, 16, 3, 0, 1, f"conv_wgrad[{dt} padded 3->16 in 64->64]")
    x, dY = _wg_inputs(dt, B, 64, 128, 2 * H, 2 * W, H, W)
    _wg_run(dt, x, dY, B, H, W, 3, 2, 0, 128, 96, 32, 0, 1, f"conv_wgrad[{dt} padded 32->96 in 64->128 stride 2]")


# =====================================================================================================================
# conv input gradients (the conv_dgrad composite)
# =====================================================================================================================
# (B, Cin, Cout, H, W of dy, stride): implicit GEMM; 128 -> 4 (conv_out): the direct kernel; stride 2: zero-stuffed dY
DG_CASES = [(2, 64, 64, 16, 16, 1), (2, 320, 640, 8, 8, 1), (2, 128, 4, 8, 8, 1), (2, 64, 128, 8, 8, 2), (1, 64, 64, 5, 7, 1), (3, 128, 64, 3, 5, 2)]


def _dg_inputs(dt, B, cin, cout, H, W, stride):
    return (_rnd((B, H, W, cout), dt, 1001), _rnd((cout, cin, 3, 3), dt, 1002, (9 * cin) ** -0.5), _rnd((B, H * stride, W * stride, cin), dt, 1003))


@torch.enable_grad()   # other test modules switch autograd off process-wide when they are imported
def _dg_ref(inp, stride, prec):
    dy, w, prior = inp
    B, H, W, _ = dy.shape
    x = torch.zeros((B, w.shape[1], H * stride, W * stride), dtype=prec, requires_grad=True)
    y = F.conv2d(x, w.to(prec), padding=1, stride=stride)
    (g,) = torch.autograd.grad(y, x, dy.to(prec).permute(0, 3, 1, 2))
    return g.permute(0, 2, 3, 1)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", DG_CASES, ids=str)
def test_conv_dgrad(dt, case):
    from mrisr import ops
    B, cin, cout, H, W, stride = case
    inp = _dg_inputs(dt, *case)
    dy, w, prior = inp
    ref = _dg_ref(inp, stride, F64)
    dy_, w_ = _dev(dy), _dev(w.float())
    for acc in (0, 1):
        def run():
            out = _dev(prior).clone() if acc else torch.full_like(_dev(prior), float("nan"))
            return ops.conv_dgrad(dy_, w_, stride=stride, dx=out, acc=acc)
        got = run()
        _check("conv.dgrad", f"conv_dgrad[{dt} {case} acc={acc}]", got, ref + (prior.to(F64) if acc else 0), dt)
        _repeat(run, got)


# =====================================================================================================================
# refusals: a bad argument is an error raised before any launch, never a fault
# =====================================================================================================================
def test_bad_arguments_are_refused():
    from mrisr import _lib as L
    from mrisr import ops
    bf = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device="cuda")
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    bad = [
        lambda: ops.groupnorm_backward(bf(1, 16, 100), bf(1, 16, 100), f32(100), f32(100), groups=25),        # 100 channels: not whole 8-vectors
        lambda: ops.groupnorm_backward(bf(1, 16, 1040), bf(1, 16, 1040), f32(1040), f32(1040), groups=65),    # > 64 groups
        lambda: ops.layernorm_backward(bf(4, 2568), bf(4, 2568), f32(2568)),                                  # row longer than 5 x 64 vectors
        lambda: ops.layernorm_backward(f32(4, 66), f32(4, 66), f32(66)),                                      # 66 floats: not whole 4-vectors
        lambda: ops.geglu(bf(4, 2 * 24)),                                                                     # half % 16
        lambda: ops.pointwise_backward(ops.PW_ROWVEC_GRAD, bf(2, 4, 64), out_f32=f32(2, 64), B=2, H=4, W=1, Cc=64, ld_out=64, off=8),
        lambda: ops.pointwise_backward(9, bf(8), bf(8), out=bf(8), n=8),
        lambda: ops.lora_wgrad(bf(64, 320), f32(64, 6), 64, 320, 1, 6, 1, 320, [f32(6, 320)]),                # rank 6
        lambda: ops.lora_wgrad(bf(64, 320), f32(64, 20), 64, 320, 1, 20, 1, 320, [f32(20, 320)]),             # rank 20
        lambda: ops.lora_wgrad(bf(64, 320), f32(64, 6), 64, 320, 1, 4, 1, 320, [f32(4, 320)], ldq=6),         # ldq % 4
        lambda: ops.lora_wgrad(bf(64, 324), f32(64, 4), 64, 324, 1, 4, 1, 324, [f32(4, 324)]),                # C % 8
        lambda: ops.lora_wgrad(bf(64, 320), f32(64, 8), 64, 320, 0, 4, 2, 120, [f32(120, 4), f32(120, 4)]),   # C != nmod * secN
        lambda: ops.lora_wgrad(bf(64 * 320 + 8)[1:1 + 64 * 320].reshape(64, 320), f32(64, 4), 64, 320, 1, 4, 1, 320, [f32(4, 320)]),  # P 2 bytes off
        lambda: ops.transpose(bf(64, 64), bf(64, 64), 64, 64, 32, 64),                                        # pitch below the row
        lambda: ops.transpose(bf(64, 64), bf(64, 64), 64, 64, 64, 64, r_valid=65),
        lambda: ops.softmax_backward(bf(4, 64), f32(4, 64), 65, 1.0),                                         # nk > ld
        lambda: ops.small_wgrad(f32(65, 8), f32(65, 8), 8, 8, f32(8, 8)),                                     # 65 rows
        lambda: ops.conv_wgrad(bf(1, 4, 4, 64), bf(16, 64), f32(64, 64, 2, 2), ks=2),                         # 2 x 2 taps
        lambda: ops.conv_wgrad(bf(1, 4, 4, 64), bf(16, 64), f32(64, 64, 3, 3), col0=8),                       # columns past the pitch
        lambda: ops.conv_wgrad(bf(1, 4, 4, 64), bf(16, 64), f32(64, 96, 3, 3)),                               # cin > cin_src
        lambda: ops.conv_dgrad(bf(1, 4, 4, 4), f32(4, 128, 3, 3), stride=2),                                  # strided dgrad of a tiny conv
        lambda: ops.conv_dgrad(bf(1, 4, 4, 64), f32(64, 64, 3, 3), stride=3),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(L.MrisrError):
            fn()
            pytest.fail(f"bad-argument case {i} was accepted")
    torch.cuda.synchronize()
    # ... and the process is still healthy
    assert "layernorm_bwd" in _prof(lambda: ops.layernorm_backward(bf(4, 320), bf(4, 320), f32(320)))


# =====================================================================================================================
# the floor table: plain torch float32 against the float64 reference on this module's inputs (CPU only; no kernel involved)
# =====================================================================================================================
def measure_floors():
    worst = {}

    def note(key, a32, a64):
        worst[key] = max(worst.get(key, 0.0), float((a32.to(F64) - a64).abs().max()))

    for dt, geoms in (("bf16", GN_GEOM), ("f32", GN_F32)):
        for geom in geoms:
            inp = _gn_inputs(dt, *geom)
            p0, p1, pg, pb = inp[5:]
            prior = p0 if p1 is None else torch.cat([p0, p1], 2)
            for silu in (True, False):
                r64, r32 = _gn_ref(inp, silu, F64), _gn_ref(inp, silu, torch.float32)
                note("gn.dx", r32[0], r64[0])
                note("gn.dx", r32[0] + prior.float(), r64[0] + prior.to(F64))
                for k, pr in ((1, pg), (2, pb)):
                    note("gn.affine", r32[k] + pr, r64[k] + pr.to(F64))
    for dt, Cc in LN_CASES:
        for M in LN_M:
            inp = _ln_inputs(dt, M, Cc)
            r64, r32 = _ln_ref(inp, F64), _ln_ref(inp, torch.float32)
            note("ln.dx", r32[0], r64[0])
            note("ln.dx", r32[0] + inp[3].float(), r64[0] + inp[3].to(F64))
    for dt in ("bf16", "f32"):
        for Cc in LN_AFF_C:
            for M in LN_AFF_M:
                inp = _ln_inputs(dt, M, Cc)
                r64, r32 = _ln_ref(inp, F64), _ln_ref(inp, torch.float32)
                for k, pr in ((1, inp[4]), (2, inp[5])):
                    note("ln.affine", r32[k] + pr, r64[k] + pr.to(F64))
        for half, M in GEGLU_CASES:
            inp = _geglu_inputs(dt, half, M)
            r64, r32 = _geglu_ref(inp, F64), _geglu_ref(inp, torch.float32)
            note("geglu.fwd", r32[0], r64[0])
            note("geglu.bwd", r32[1], r64[1])
        for n in PW_SIZES:
            dy, pre = _rnd((n,), dt, 501), _rnd((n,), dt, 502, 2.0)
            note("pw.silu_bwd", dy.float() * _silu_grad(pre.float()), dy.to(F64) * _silu_grad(pre.to(F64)))
        worst.setdefault("pw.relu_bwd", 0.0)    # a select: exact
        for B, H, W, Cc in SUMPOOL_CASES:
            src, prior = _rnd((B, 2 * H, 2 * W, Cc), dt, 511), _rnd((B, H, W, Cc), dt, 512)
            s32, s64 = src.float().reshape(B, H, 2, W, 2, Cc).sum((2, 4)), src.to(F64).reshape(B, H, 2, W, 2, Cc).sum((2, 4))
            note("pw.sumpool2", s32, s64)
            note("pw.sumpool2", s32 + prior.float(), s64 + prior.to(F64))
        for B, Cc, H, W in MSE_CASES:
            pred, tgt = _rnd((B, H, W, Cc), dt, 521), _rnd((B, Cc, H, W), "f32", 522)
            d32, d64 = pred.float() - tgt.permute(0, 2, 3, 1), pred.to(F64) - tgt.to(F64).permute(0, 2, 3, 1)
            note("pw.mse_grad", 2 * d32 / d32.numel(), 2 * d64 / d64.numel())
            note("pw.mse_loss", (d32 * d32).mean(), (d64 * d64).mean())
        for B, HW, Cc, scalar_t, off in ROWVEC_CASES:
            dh, prior = _rnd((B, HW, Cc), dt, 531), _rnd((B, off + Cc + 5), "f32", 532)
            pr = prior[:, off:off + Cc]
            if scalar_t:
                note("pw.rowvec_grad", pr[0] + dh.float().sum((0, 1)), pr[0].to(F64) + dh.to(F64).sum((0, 1)))
            else:
                note("pw.rowvec_grad", pr + dh.float().sum(1), pr.to(F64) + dh.to(F64).sum(1))
        for M, Cc in ((1, 64), (513, 77), (2050, 320), (4099, 1)):
            dy, prior = _rnd((M, Cc), dt, 541), _rnd((Cc,), "f32", 542)
            note("pw.colsum", prior + dy.float().sum(0), prior.to(F64) + dy.to(F64).sum(0))
        lora = [(c, r, n, m, M, 1.0, None, None) for (c, r, n, m, M) in LORA_CASES if dt == "bf16" or (r in (4, 16) and n in (1, 3))]
        lora += [(960, 4, 3, 0, 1024, 1.0, None, None), (320, 8, 3, 1, 154, 1.0, None, None), (320, 4, 2, 1, 1024, 1.0, None, None),
                 (320, 4, 1, 1, 4136, 1.0, 960, None), (640, 4, 2, 0, 154, 1.0, 1928, 16), (320, 4, 1, 0, 1024, 0.375, None, None),
                 (1280, 16, 2, 1, 154, -2.5, None, None)]
        if dt == "bf16":
            lora += [(320, 4, 1, 0, 65544, 1.0, None, None), (320, 4, 1, 1, 65544, 1.0, None, None), (320, 4, 3, 1, 65544, 1.0, None, None)]
        for Cc, r, nmod, mode, M, scale, ldp, ldq in lora:
            secN = Cc // nmod if mode == 0 else 320
            P, Q = _lora_P(dt, M, ldp or Cc), _lora_Q(M, ldq or nmod * r)
            pri = _lora_priors(Cc, mode, r, nmod, secN)
            for a, b in zip(_lora_ref(P, Q, Cc, mode, r, nmod, secN, scale, pri, torch.float32), _lora_ref(P, Q, Cc, mode, r, nmod, secN, scale, pri, F64)):
                note("lora.wgrad", a, b)
        for nk, ld, rows in SM_CASES:
            inp = _sm_inputs(dt, nk, ld, rows)
            note("softmax_bwd", _sm_ref(inp, nk, 0.125, torch.float32), _sm_ref(inp, nk, 0.125, F64))
        for rows in (1, 2, 64):
            for N, K in SMALL_SHAPES:
                inp = _small_inputs(dt, rows, N, K)
                for silu_in, use_pre in ((0, 0), (1, 1)):
                    a, b = _small_ref(inp, N, K, silu_in, use_pre, torch.float32), _small_ref(inp, N, K, silu_in, use_pre, F64)
                    note("small.wgrad", a[0], b[0]); note("small.wgrad", a[1], b[1]); note("small.dgrad", a[2], b[2])
        wg = []
        for (B, cin, cout, ks, stride, H, W) in WG_CONV:
            Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
            x, dY = _wg_inputs(dt, B, cin, cout, H, W, Ho, Wo)
            wg.append((x, dY, B, Ho, Wo, ks, stride, cout, cin))
        x, dY = _wg_inputs(dt, 1, 320, 960, 200, 1, 200, 1)
        wg += [(x, dY[:, c:c + 320], 1, 200, 1, 1, 1, 320, 320) for c in (0, 320, 640)]
        x, dY = _wg_inputs(dt, 1, 320, 1280, 131, 1, 131, 1)
        wg.append((x, _unil(dY), 1, 131, 1, 1, 1, 1280, 320))
        x, dY = _wg_inputs(dt, 2, 64, 64, 8, 8, 8, 8)
        wg.append((x, dY, 2, 8, 8, 3, 1, 16, 3))
        x, dY = _wg_inputs(dt, 2, 64, 128, 16, 16, 8, 8)
        wg.append((x, dY, 2, 8, 8, 3, 2, 96, 32))
        for x, nat, B, Ho, Wo, ks, stride, cout, cin in wg:
            pW, pB = _rnd((cout, cin, ks, ks), "f32", 903), _rnd((cout,), "f32", 904)
            a, b = _wg_ref(x, nat, B, Ho, Wo, ks, stride, cout, cin, pW, pB, torch.float32), _wg_ref(x, nat, B, Ho, Wo, ks, stride, cout, cin, pW, pB, F64)
            note("conv.wgrad", a[0], b[0]); note("conv.wgrad_bias", a[1], b[1])
        for case in DG_CASES:
            inp = _dg_inputs(dt, *case)
            a, b = _dg_ref(inp, case[5], torch.float32), _dg_ref(inp, case[5], F64)
            note("conv.dgrad", a, b)
            note("conv.dgrad", a + inp[2].float(), b + inp[2].to(F64))
    return worst


if __name__ == "__main__":
    torch.set_num_threads(8)
    w = measure_floors()
    for k in sorted(w):
        print(f"    {k:<20s}{w[k]:<28.3e}{8 * w[k]:.3e}")
    print("MEASURED = {")
    for k in sorted(w):
        print(f'    "{k}": {w[k]:.3e},')
    print("}")
