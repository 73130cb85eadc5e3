"""GPU: the two kernels of perturbed-attention guidance alone.

* identity attention (``mrisr_op_attn_identity``): head-major v^T -> token rows for a sample range.  A copy, so the check is exact
  equality with a torch gather; the pads of the source hold garbage (they must never reach the output) and the output is pre-filled
  with NaN (rows outside the range must still be NaN afterwards).
* the three-way fused step (``mrisr_op_pag_step``) against the float64 formulae of include/mrisr.h at 1e-5 - a handful of f32
  operations per element and two tree sums over <= 20736 f32 terms, each a few 1e-7, the bound test_gpu_guidance.py uses for the
  two-way kernel - and, at s = 0, bit for bit against ``mrisr_op_guided_step``; the multistep kinds (the history ring, UniPC's
  corrected state) through ``mrisr_op_pag_multistep_step`` against the row layout of include/mrisr.h in float64, and at s = 0 bit for
  bit against ``mrisr_op_multistep_step``'s guided form."""
import ctypes as C

import numpy as np
import pytest
import torch

from pag_ref import pag_eps
from pag_testlib import DDIM, DPMSOLVERPP, RESSHIFT, UNIPC, coef_row, kernel_cases, maxrel, rel

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ identity attention
def op_identity(vt, out, B, H, N, hd, npad, dpad, b0, nb):
    import mrisr
    L = mrisr._lib
    L.check(L.lib().mrisr_op_attn_identity(L.dtype_id(vt.dtype), vt.data_ptr(), out.data_ptr(), B, H, N, hd, npad, dpad, b0, nb, L.stream_ptr()))


def pads(mode, N, hd):
    if mode == "equal":
        return N, hd
    if mode == "model":  # what the UNet's workspace plan uses, made larger than the valid extent on both axes
        return (N + 63) // 64 * 64 + (64 if N % 64 == 0 else 0), (hd + 31) // 32 * 32 + (32 if hd % 32 == 0 else 0)
    return N + 3, hd + 1  # rows that are not 16-byte multiples: the element-wise read path


@pytest.mark.parametrize("mode", ["equal", "model", "odd"])
@pytest.mark.parametrize("N", [16, 64, 1024])
@pytest.mark.parametrize("hd", [8, 12, 40, 80, 160])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_identity_attention_is_an_exact_gather(dtype, hd, N, mode):
    H = 2
    npad, dpad = pads(mode, N, hd)
    gen = torch.Generator().manual_seed(2600 + hd * 7 + N)
    for B, b0, nb in ((4, 0, 4), (4, 0, 2), (3, 1, 1)):  # all samples, the first half, an interior one out of three
        vt = torch.randn((B * H, dpad, npad), generator=gen).to(dtype).cuda()  # pads hold garbage, not zeros
        want = vt.view(B, H, dpad, npad)[:, :, :hd, :N].permute(0, 3, 1, 2).reshape(B, N, H * hd)
        out = torch.full((B, N, H * hd), float("nan"), dtype=dtype, device="cuda")
        op_identity(vt, out, B, H, N, hd, npad, dpad, b0, nb)
        torch.cuda.synchronize()
        assert torch.equal(out[b0:b0 + nb], want[b0:b0 + nb]), (B, b0, nb)
        rest = torch.cat([out[:b0], out[b0 + nb:]])
        assert bool(torch.isnan(rest).all()), (B, b0, nb)


def test_identity_attention_refusals():
    import mrisr
    B, H, N, hd, npad, dpad = 2, 2, 16, 8, 64, 32
    vt = torch.randn((B * H, dpad, npad)).cuda()
    out = torch.full((B, N, H * hd), float("nan")).cuda()
    L = mrisr._lib

    def call(vp, op, *geo):
        L.check(L.lib().mrisr_op_attn_identity(L.MRISR_F32, vp, op, *geo, L.stream_ptr()))

    good = (B, H, N, hd, npad, dpad, 0, B)
    for vp, op, geo, what in ((None, out.data_ptr(), good, "null"),
                              (vt.data_ptr(), None, good, "null"),
                              (vt.data_ptr() + 2, out.data_ptr(), good, "misaligned"),
                              (vt.data_ptr(), out.data_ptr() + 1, good, "misaligned"),
                              (vt.data_ptr(), out.data_ptr(), (B, H, N, hd, N - 1, dpad, 0, B), "npad"),
                              (vt.data_ptr(), out.data_ptr(), (B, H, N, hd, npad, hd - 1, 0, B), "dpad"),
                              (vt.data_ptr(), out.data_ptr(), (B, H, N, hd, npad, dpad, 1, B), "range"),
                              (vt.data_ptr(), out.data_ptr(), (B, H, N, hd, npad, dpad, -1, 1), "range"),
                              (vt.data_ptr(), out.data_ptr(), (B, H, N, hd, npad, dpad, 0, B + 1), "range"),
                              (vt.data_ptr(), out.data_ptr(), (B, H, N, hd, npad, dpad, 0, -1), "range")):
        with pytest.raises(RuntimeError, match=what):
            call(vp, op, *geo)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())  # nothing was launched
    call(vt.data_ptr(), out.data_ptr(), *good)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------ the three-way step
def op_pag_step(kind, x, eps3, row, g, s, phi, lr=None, noise=None, clip=0.0):
    """mrisr_op_pag_step on copies: returns (new x, staging buffer [3B])."""
    import mrisr
    L = mrisr._lib
    x = x.clone()
    x3 = torch.full((3 * x.shape[0],) + tuple(x.shape[1:]), float("nan"), device=x.device)
    t = {k: L.as_tensor(v) for k, v in (("x", x), ("x3", x3), ("e", eps3), ("lr", lr), ("nz", noise)) if v is not None}
    L.check(L.lib().mrisr_op_pag_step(kind, C.byref(t["x"]), C.byref(t["x3"]), C.byref(t["e"]),
                                      C.byref(t["lr"]) if lr is not None else None, C.byref(t["nz"]) if noise is not None else None,
                                      (C.c_float * 8)(*row), clip, g, s, phi, L.stream_ptr()))
    return x, x3


def op_guided_step(kind, x, eps2, row, g, phi, lr=None, noise=None, clip=0.0):
    """mrisr_op_guided_step on copies: the new x."""
    import mrisr
    L = mrisr._lib
    x = x.clone()
    x2 = torch.empty((2 * x.shape[0],) + tuple(x.shape[1:]), device=x.device)
    t = {k: L.as_tensor(v) for k, v in (("x", x), ("x2", x2), ("e", eps2), ("lr", lr), ("nz", noise)) if v is not None}
    L.check(L.lib().mrisr_op_guided_step(kind, C.byref(t["x"]), C.byref(t["x2"]), C.byref(t["e"]),
                                         C.byref(t["lr"]) if lr is not None else None, C.byref(t["nz"]) if noise is not None else None,
                                         (C.c_float * 8)(*row), clip, g, phi, L.stream_ptr()))
    return x


def ref_pag_step(kind, x, eps3, row, g, s, phi, lr=None, noise=None, clip=0.0):
    """The formulae of include/mrisr.h in float64 on the same (f32-valued) inputs."""
    B = x.shape[0]
    x = x.double()
    e = pag_eps(eps3[:B], eps3[B:2 * B], eps3[2 * B:], float(np.float32(g)), float(np.float32(s)), float(np.float32(phi)))
    if kind == DDIM:
        return row[0] * x + row[1] * e
    if kind == RESSHIFT:
        sat, s1mat, sap, sig = row
        x0 = (x - (1 - sat) * lr.double() - s1mat * e) / sat
        v = sap * x0 + (1 - sap) * lr.double()
    else:
        ia, ie, c0, cx, sig = row
        x0 = ia * x - ie * e
        if clip > 0:
            x0 = x0.clamp(-clip, clip)
        v = c0 * x0 + cx * x
    return v + sig * noise.double() if noise is not None else v


# (1, 4, 72): 20736 elements per sample, above the 16 Ki the registers hold - the re-reading variant
# (2, 4, 40): 6400 elements per sample - the two-pieces-per-thread variant (4096 < per <= 8192), 1600 pieces on 1024 threads: a masked tail
@pytest.mark.parametrize("B,Cc,h", [(1, 4, 16), (3, 4, 32), (2, 4, 64), (1, 4, 72), (2, 4, 40)])
def test_pag_step_kernel_matches_float64_formulae(B, Cc, h):
    gen = torch.Generator().manual_seed(2700 + B * 100 + h)
    x = torch.randn((B, Cc, h, h), generator=gen).cuda()
    eps3 = torch.randn((3 * B, Cc, h, h), generator=gen)
    # correlated parts with a mean, as three forwards of one network give: [perturbed; unconditional; conditional]
    eps3[B:2 * B] = 0.8 * eps3[B:2 * B] + 0.5 * eps3[2 * B:] + 0.05
    eps3[:B] = 0.6 * eps3[:B] + 0.7 * eps3[2 * B:] - 0.03
    eps3 = eps3.cuda()
    lr = (0.3 * torch.randn((B, Cc, h, h), generator=gen)).cuda()
    nz = torch.randn((B, Cc, h, h), generator=gen).cuda()
    worst = (0.0, 0.0)
    for kind, with_noise, clip in kernel_cases():
        row = coef_row(kind)
        kw = dict(lr=lr if kind == RESSHIFT else None, noise=nz if with_noise else None, clip=clip)
        for g in (1.0, 3.5):
            for phi in (0.0, 0.7):
                for s in (0.0, 1.0, 3.0):
                    out, x3 = op_pag_step(kind, x, eps3, row, g, s, phi, **kw)
                    ref = ref_pag_step(kind, x, eps3, row, g, s, phi, **kw)
                    r, m = rel(out, ref), maxrel(out, ref)
                    worst = (max(worst[0], r), max(worst[1], m))
                    assert r <= 1e-5 and m <= 1e-5, (kind, with_noise, clip, g, s, phi, r, m)
                    # the next forward's input: all three thirds of the staging buffer are the new state, bit for bit
                    assert torch.equal(x3[:B], out) and torch.equal(x3[B:2 * B], out) and torch.equal(x3[2 * B:], out), (kind, g, s, phi)
                    if s == 0.0:  # the guided step on [eps_u; eps_c], bit for bit
                        two = op_guided_step(kind, x, eps3[B:].contiguous(), row, g, phi, **kw)
                        assert torch.equal(out, two), (kind, with_noise, clip, g, phi)
    print(f"pag step kernel B={B} C={Cc} h={h}: worst rel {worst[0]:.3e} maxrel {worst[1]:.3e}")


def test_pag_step_refusals():
    import mrisr
    x = torch.randn((1, 4, 16, 16)).cuda()
    eps3 = torch.randn((3, 4, 16, 16)).cuda()
    row = coef_row(DDIM)
    with pytest.raises(mrisr.MrisrError, match="pag_scale"):
        op_pag_step(DDIM, x, eps3, row, 3.0, -1.0, 0.0)
    with pytest.raises(mrisr.MrisrError, match="pag_scale"):
        op_pag_step(DDIM, x, eps3, row, 3.0, float("nan"), 0.0)
    with pytest.raises(mrisr.MrisrError, match="eps3"):
        op_pag_step(DDIM, x, eps3[:2].contiguous(), row, 3.0, 1.0, 0.0)
    with pytest.raises(mrisr.MrisrError, match="guidance_rescale"):
        op_pag_step(DDIM, x, eps3, row, 3.0, 1.0, 1.5)


# ------------------------------------------------------------------------------------------------ the three-way step, multistep kinds
def op_pag_multistep_step(kind, x, eps3, row, order, slot, hist, xc, g, s, phi, lr=None, two_way=False):
    """mrisr_op_pag_multistep_step (two_way: mrisr_op_multistep_step's guided form on [2B]) on copies: (new x, history, corrected
    state or None, staging buffer)."""
    import mrisr
    L = mrisr._lib
    K = 2 if two_way else 3
    x, hist = x.clone(), hist.clone()
    xc = xc.clone() if kind == UNIPC else None
    xk = torch.full((K * x.shape[0],) + tuple(x.shape[1:]), float("nan"), device=x.device)
    ts = {k: L.as_tensor(v) for k, v in (("x", x), ("xk", xk), ("e", eps3), ("lr", lr), ("xc", xc)) if v is not None}
    t_h = L.as_tensor(hist, shape=(hist.shape[0] * hist.shape[1],) + tuple(hist.shape[2:]))
    args = [kind, C.byref(ts["x"]), C.byref(ts["xk"]), C.byref(ts["e"]), C.byref(ts["lr"]) if lr is not None else None, C.byref(t_h),
            C.byref(ts["xc"]) if xc is not None else None, (C.c_float * 16)(*row), order, slot]
    if two_way:
        L.check(L.lib().mrisr_op_multistep_step(*args, g, phi, L.stream_ptr()))
    else:
        L.check(L.lib().mrisr_op_pag_multistep_step(*args, g, s, phi, L.stream_ptr()))
    return x, hist, xc, xk


def ref_pag_multistep_step(kind, x, eps3, row, order, slot, hist, xc, g, s, phi, lr=None):
    """The row layout of include/mrisr.h in float64 on the same (f32-valued) inputs:
    row = {m: z, eps | corrected state: z, eps, xc, h1, h2, h3 | next state: z, eps, xc, h1, h2, h3 | 0, 0}, z = x - lr."""
    B = x.shape[0]
    e = pag_eps(eps3[:B], eps3[B:2 * B], eps3[2 * B:], float(np.float32(g)), float(np.float32(s)), float(np.float32(phi)))
    x, hist = x.double(), hist.double().clone()
    xc = xc.double() if kind == UNIPC else torch.zeros_like(x)
    anchor = lr.double() if lr is not None else 0.0
    z = x - anchor
    h = [hist[(slot - k) % order] if k <= order else torch.zeros_like(x) for k in (1, 2, 3)]
    r = [float(v) for v in row]
    m = r[0] * z + r[1] * e
    zc = r[2] * z + r[3] * e + r[4] * xc + r[5] * h[0] + r[6] * h[1] + r[7] * h[2]
    zn = r[8] * z + r[9] * e + r[10] * xc + r[11] * h[0] + r[12] * h[1] + r[13] * h[2]
    hist[slot % order] = m
    return zn + anchor, hist, zc


# (1, 4, 72): the re-reading variant; orders: every ring size of each solver
@pytest.mark.parametrize("kind,order", [(UNIPC, 1), (UNIPC, 2), (UNIPC, 3), (DPMSOLVERPP, 1), (DPMSOLVERPP, 2)])
@pytest.mark.parametrize("B,Cc,h", [(1, 4, 16), (3, 4, 32), (1, 4, 72)])
def test_pag_multistep_step_kernel_matches_float64_formulae(kind, order, B, Cc, h):
    """On the rows the host class builds for warm steps (all history terms and the corrector live) of a 20-step trailing schedule."""
    import mrisr
    cls = mrisr.UniPCMultistepScheduler if kind == UNIPC else mrisr.DPMSolverMultistepScheduler
    sch = cls(solver_order=order, timestep_spacing="trailing", final_sigmas_type="sigma_min")
    sch.set_timesteps(20)
    rows = sch.coefficient_rows()
    gen = torch.Generator().manual_seed(2750 + B * 100 + h + order)
    shape = (B, Cc, h, h)
    x = torch.randn(shape, generator=gen).cuda()
    eps3 = torch.randn((3 * B,) + shape[1:], generator=gen)
    eps3[B:2 * B] = 0.8 * eps3[B:2 * B] + 0.5 * eps3[2 * B:] + 0.05
    eps3[:B] = 0.6 * eps3[:B] + 0.7 * eps3[2 * B:] - 0.03
    eps3 = eps3.cuda()
    lr = (0.3 * torch.randn(shape, generator=gen)).cuda()
    hist = torch.randn((order,) + shape, generator=gen).cuda()
    xc = (x.cpu() + 0.05 * torch.randn(shape, generator=gen)).cuda()
    worst = 0.0
    for slot in (7, 8, 12):  # every ring position
        row = [float(np.float32(v)) for v in rows[slot]]
        assert any(row[8:14]) and (order == 1 or row[11] != 0.0)
        for anchor in (None, lr):
            for g in (1.0, 3.5):
                for phi in (0.0, 0.7):
                    for s in (0.0, 1.0, 3.0):
                        tag = (kind, order, slot, anchor is not None, g, s, phi)
                        out, h_out, xc_out, x3 = op_pag_multistep_step(kind, x, eps3, row, order, slot, hist, xc, g, s, phi, anchor)
                        ref, h_ref, xc_ref = ref_pag_multistep_step(kind, x, eps3, row, order, slot, hist, xc, g, s, phi, anchor)
                        errs = [rel(out, ref), maxrel(out, ref), rel(h_out, h_ref), maxrel(h_out, h_ref)]
                        if kind == UNIPC:
                            errs += [rel(xc_out, xc_ref), maxrel(xc_out, xc_ref)]
                        worst = max([worst] + errs)
                        assert max(errs) <= 1e-5, (tag, errs)
                        for k in range(order):  # only the slot of this step is written
                            if k != slot % order:
                                assert torch.equal(h_out[k], hist[k]), tag
                        assert torch.equal(x3[:B], out) and torch.equal(x3[B:2 * B], out) and torch.equal(x3[2 * B:], out), tag
                        if s == 0.0:  # the guided multistep step on [eps_u; eps_c], bit for bit: x, ring and corrected state
                            two = op_pag_multistep_step(kind, x, eps3[B:].contiguous(), row, order, slot, hist, xc, g, 0.0, phi, anchor, two_way=True)
                            assert torch.equal(out, two[0]) and torch.equal(h_out, two[1]), tag
                            assert kind != UNIPC or torch.equal(xc_out, two[2]), tag
    print(f"pag multistep step kernel kind {kind} order {order} B={B} C={Cc} h={h}: worst {worst:.3e}")


def test_pag_multistep_step_refusals():
    import mrisr
    x = torch.randn((1, 4, 16, 16)).cuda()
    eps3 = torch.randn((3, 4, 16, 16)).cuda()
    hist = torch.zeros((2, 1, 4, 16, 16)).cuda()
    row = [0.0] * 16
    with pytest.raises(mrisr.MrisrError, match="hist"):        # a ring of one slab for order 2
        op_pag_multistep_step(UNIPC, x, eps3, row, 2, 0, hist[:1].contiguous(), x, 3.0, 1.0, 0.0)
    with pytest.raises(mrisr.MrisrError, match="eps3"):        # [2B] where 3B are needed
        op_pag_multistep_step(UNIPC, x, eps3[:2].contiguous(), row, 2, 0, hist, x, 3.0, 1.0, 0.0)
    with pytest.raises(mrisr.MrisrError, match="pag_scale"):
        op_pag_multistep_step(DPMSOLVERPP, x, eps3, row, 2, 0, hist, x, 3.0, -1.0, 0.0)
    with pytest.raises(mrisr.MrisrError, match="UniPC or DPM-Solver"):
        op_pag_multistep_step(DDIM, x, eps3, row, 2, 0, hist, x, 3.0, 1.0, 0.0)
