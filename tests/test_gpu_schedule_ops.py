"""GPU: the kernels of the per-step schedule alone.

* the fused guided step reading {g, s, phi} from a schedule table (``mrisr_op_scheduled_step``): all five step kinds; the K = 2 step of
  classifier-free guidance, the K = 2 step of PAG alone (the kernel forms g = 1 + s) and the K = 3 step; 1,024, 4,096 and 20,736
  elements per sample (the last takes the re-reading kernel when a row has phi > 0); two tables of four distinct rows - one with
  phi = 0 everywhere (the grid-stride kernel), one with phi in {0.7, 0, 0.3, 0} (the rescale kernels, rows with phi == 0 included) -
  read at step counters 0, 2 and 3.
  - against the float64 formulae of include/mrisr.h on the same f32-valued inputs at 1e-5 relative L2 and max-relative: the bound
    test_gpu_multistep.py and test_gpu_pag_ops.py state for this arithmetic (a handful of f32 operations per element and two tree sums
    over <= 20,736 f32 terms);
  - bit for bit against the scalar entries (``mrisr_op_guided_step`` / ``mrisr_op_pag_step`` / ``mrisr_op_multistep_step`` /
    ``mrisr_op_pag_multistep_step``) called with the row's own scalars, whenever both take the same kernel: every row of the all-zero-phi
    table, and the rows with phi > 0 of the other;
  - all K parts of the staging buffer are the new x;
  - the neutral row {1, 0, 0, ...}: against the step formula on the conditional part ALONE in float64 at 1e-6.  Not bit-equal: the
    kernel still evaluates fma(1, eps_c - eps_0, eps_0), one rounding away from eps_c.
* one FreeU stage reading (b, s) from the table (``mrisr_op_freeu_scheduled``), f32 and bf16: bit for bit the by-value launch
  (``mrisr_op_freeu``) with the row's numbers, and the (1, 1) row leaves both tensors bit-identical.
* every refusal of ``mrisr_sampler_set_schedule`` and of the two entries, before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from pag_ref import pag_eps
from pag_testlib import DDIM, DDPM, DPMSOLVERPP, RESSHIFT, UNIPC, coef_row, kernel_cases, maxrel, rel
from schedule_ref import NEUTRAL

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# four distinct rows each; row 2 of the first and row 3 of the second are neutral.  Slots 0, 2 and 3 are read
TABLE_NOPHI = np.float32([(3.5, 1.0, 0.0, 1, 1, 1, 1, 0), (7.0, 2.0, 0.0, 1, 1, 1, 1, 0), NEUTRAL, (1.5, 0.5, 0.0, 1, 1, 1, 1, 0)])
TABLE_PHI = np.float32([(3.5, 1.0, 0.7, 1, 1, 1, 1, 0), (2.0, 2.0, 0.0, 1, 1, 1, 1, 0), (2.0, 3.0, 0.3, 1, 1, 1, 1, 0), NEUTRAL])
SLOTS = (0, 2, 3)
VARIANTS = {"cfg": (2, 0), "pag": (2, 1), "pag+cfg": (3, 0)}  # name -> (K, pag_alone)


def _lib():
    import mrisr
    return mrisr._lib


def _opt(t):
    return C.byref(t) if t is not None else None


def op_scheduled_step(kind, K, pag_alone, x, epsK, row, table, slot, lr=None, noise=None, clip=0.0, hist=None, xc=None, order=0):
    """mrisr_op_scheduled_step on copies: (new x, staging buffer [K B], history or None, corrected state or None).  ``noise``: the
    stack [slot + 1, B, C, h, w]."""
    L = _lib()
    x = x.clone()
    xk = torch.full((K * x.shape[0],) + tuple(x.shape[1:]), float("nan"), device=x.device)
    hist = hist.clone() if hist is not None else None
    xc = xc.clone() if xc is not None else None
    tx, txk, te = L.as_tensor(x), L.as_tensor(xk), L.as_tensor(epsK)
    tlr = L.as_tensor(lr) if lr is not None else None
    tnz = L.as_tensor(noise, shape=(noise.shape[0] * noise.shape[1],) + tuple(noise.shape[2:])) if noise is not None else None
    th = L.as_tensor(hist, shape=(hist.shape[0] * hist.shape[1],) + tuple(hist.shape[2:])) if hist is not None else None
    txc = L.as_tensor(xc) if xc is not None else None
    tbl = np.ascontiguousarray(table, dtype=np.float32)
    L.check(L.lib().mrisr_op_scheduled_step(kind, K, pag_alone, C.byref(tx), C.byref(txk), C.byref(te), _opt(tlr), _opt(tnz), _opt(th), _opt(txc),
                                            (C.c_float * 16)(*row), order, slot, clip, tbl.ctypes.data_as(C.c_void_p), len(tbl), L.stream_ptr()))
    return x, xk, hist, xc


def op_scalar_step(kind, K, x, epsK, row, g, s, phi, slot=0, lr=None, noise=None, clip=0.0, hist=None, xc=None, order=0):
    """The existing scalar entry of this (kind, K) on copies: (new x, history or None, corrected state or None)."""
    L = _lib()
    x = x.clone()
    xk = torch.empty((K * x.shape[0],) + tuple(x.shape[1:]), device=x.device)
    hist = hist.clone() if hist is not None else None
    xc = xc.clone() if xc is not None else None
    tx, txk, te = L.as_tensor(x), L.as_tensor(xk), L.as_tensor(epsK)
    tlr = L.as_tensor(lr) if lr is not None else None
    tnz = L.as_tensor(noise) if noise is not None else None
    if kind in (UNIPC, DPMSOLVERPP):
        th = L.as_tensor(hist, shape=(hist.shape[0] * hist.shape[1],) + tuple(hist.shape[2:]))
        txc = L.as_tensor(xc) if xc is not None else None
        args = [kind, C.byref(tx), C.byref(txk), C.byref(te), _opt(tlr), C.byref(th), _opt(txc), (C.c_float * 16)(*row), order, slot]
        if K == 2:
            L.check(L.lib().mrisr_op_multistep_step(*args, g, phi, L.stream_ptr()))
        else:
            L.check(L.lib().mrisr_op_pag_multistep_step(*args, g, s, phi, L.stream_ptr()))
    elif K == 2:
        L.check(L.lib().mrisr_op_guided_step(kind, C.byref(tx), C.byref(txk), C.byref(te), _opt(tlr), _opt(tnz), (C.c_float * 8)(*row), clip, g, phi,
                                             L.stream_ptr()))
    else:
        L.check(L.lib().mrisr_op_pag_step(kind, C.byref(tx), C.byref(txk), C.byref(te), _opt(tlr), _opt(tnz), (C.c_float * 8)(*row), clip, g, s, phi,
                                          L.stream_ptr()))
    return x, hist, xc


def ref_step(kind, x, e, row, slot, lr=None, noise=None, clip=0.0, hist=None, xc=None, order=0):
    """The step formulae of include/mrisr.h in float64 with the prediction ``e``: (new x, history or None, corrected state or None)."""
    x = x.double().cpu()
    lr = lr.double().cpu() if lr is not None else None
    if kind in (UNIPC, DPMSOLVERPP):
        hist = hist.double().cpu().clone()
        xcv = xc.double().cpu() if xc is not None else torch.zeros_like(x)
        anchor = lr if lr is not None else 0.0
        z = x - anchor
        h = [hist[(slot - k) % order] if k <= order else torch.zeros_like(x) for k in (1, 2, 3)]
        r = [float(v) for v in row]
        m = r[0] * z + r[1] * e
        zc = r[2] * z + r[3] * e + r[4] * xcv + r[5] * h[0] + r[6] * h[1] + r[7] * h[2]
        zn = r[8] * z + r[9] * e + r[10] * xcv + r[11] * h[0] + r[12] * h[1] + r[13] * h[2]
        hist[slot % order] = m
        return zn + anchor, hist, zc
    if kind == DDIM:
        return row[0] * x + row[1] * e, None, None
    if kind == RESSHIFT:
        sat, s1mat, sap, sig = row
        x0 = (x - (1 - sat) * lr - s1mat * e) / sat
        v = sap * x0 + (1 - sap) * lr
    else:
        ia, ie, c0, cx, sig = row
        x0 = ia * x - ie * e
        if clip > 0:
            x0 = x0.clamp(-clip, clip)
        v = c0 * x0 + cx * x
    return (v + sig * noise.double().cpu() if noise is not None else v), None, None


def all_cases():
    """(kind, with noise, clip, order) of the five step kinds."""
    for kind, with_noise, clip in kernel_cases():
        yield kind, with_noise, clip, 0
    yield UNIPC, False, 0.0, 2
    yield DPMSOLVERPP, False, 0.0, 2


# (2, 4, 72): 20,736 elements per sample, above the 16 Ki the registers hold: the re-reading kernel
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B,Cc,h", [(1, 4, 16), (3, 4, 32), (2, 4, 72)])
def test_scheduled_step_kernel(B, Cc, h, variant):
    import mrisr
    K, pag_alone = VARIANTS[variant]
    gen = torch.Generator().manual_seed(3500 + B * 100 + h + K * 7 + pag_alone)
    shape = (B, Cc, h, h)
    x = torch.randn(shape, generator=gen).cuda()
    eps3 = torch.randn((3 * B,) + shape[1:], generator=gen)
    # correlated parts with a mean, as three forwards of one network give: [perturbed; unconditional; conditional]
    eps3[B:2 * B] = 0.8 * eps3[B:2 * B] + 0.5 * eps3[2 * B:] + 0.05
    eps3[:B] = 0.6 * eps3[:B] + 0.7 * eps3[2 * B:] - 0.03
    eps_p, eps_u, eps_c = eps3[:B], eps3[B:2 * B], eps3[2 * B:]
    epsK = {"cfg": torch.cat([eps_u, eps_c]), "pag": torch.cat([eps_p, eps_c]), "pag+cfg": eps3}[variant].contiguous().cuda()
    lr = (0.3 * torch.randn(shape, generator=gen)).cuda()
    nz = torch.randn((max(SLOTS) + 1,) + shape, generator=gen).cuda()
    hist = torch.randn((2,) + shape, generator=gen).cuda()
    xc0 = (x.cpu() + 0.05 * torch.randn(shape, generator=gen)).cuda()
    ms_rows = {}
    for kind, cls in ((UNIPC, mrisr.UniPCMultistepScheduler), (DPMSOLVERPP, mrisr.DPMSolverMultistepScheduler)):
        sch = cls(solver_order=2, timestep_spacing="trailing", final_sigmas_type="sigma_min")
        sch.set_timesteps(20)
        ms_rows[kind] = [float(np.float32(v)) for v in sch.coefficient_rows()[8]]  # a warm step: history terms and the corrector live
        assert any(ms_rows[kind][8:14]) and ms_rows[kind][11] != 0.0
    worst, worst_neutral, n_bits = 0.0, 0.0, 0
    for kind, with_noise, clip, order in all_cases():
        multistep = order > 0
        row = ms_rows[kind] if multistep else coef_row(kind)
        for table in (TABLE_NOPHI, TABLE_PHI):
            for slot in SLOTS:
                tag = (variant, kind, with_noise, clip, "phi" if table is TABLE_PHI else "nophi", slot)
                g_row, s_row, phi = (float(v) for v in table[slot][:3])
                kw = dict(lr=lr if (kind == RESSHIFT or multistep) else None, clip=clip, hist=hist if multistep else None,
                          xc=xc0 if kind == UNIPC else None, order=order)
                out, xk, h_out, xc_out = op_scheduled_step(kind, K, pag_alone, x, epsK, row + [0.0] * (16 - len(row)), table, slot,
                                                           noise=nz[:slot + 1].contiguous() if with_noise else None, **kw)
                # the float64 formula with this row's scalars
                if variant == "cfg":
                    e = pag_eps(eps_c, eps_u, eps_c, g_row, 0.0, phi)
                    g_scalar, s_scalar = g_row, 0.0
                elif variant == "pag":
                    e = pag_eps(eps_p, None, eps_c, 1.0, s_row, phi)
                    g_scalar, s_scalar = float(np.float32(1.0) + np.float32(s_row)), 0.0
                else:
                    e = pag_eps(eps_p, eps_u, eps_c, g_row, s_row, phi)
                    g_scalar, s_scalar = g_row, s_row
                ref_kw = dict(kw, noise=nz[slot] if with_noise else None)
                ref, h_ref, xc_ref = ref_step(kind, x, e, row, slot, **ref_kw)
                errs = [rel(out, ref), maxrel(out, ref)]
                if multistep:
                    errs += [rel(h_out, h_ref), maxrel(h_out, h_ref)]
                    for k in range(order):  # only the slot of this step is written
                        if k != slot % order:
                            assert torch.equal(h_out[k], hist[k]), tag
                if kind == UNIPC:
                    errs += [rel(xc_out, xc_ref), maxrel(xc_out, xc_ref)]
                worst = max([worst] + errs)
                assert max(errs) <= 1e-5, (tag, errs)
                # the next forward's input: every part of the staging buffer is the new state, bit for bit
                for k in range(K):
                    assert torch.equal(xk[k * B:(k + 1) * B], out), (tag, k)
                # the scalar entry with the row's own scalars: the same kernel when the table has no phi, or this row has one
                if table is TABLE_NOPHI or phi > 0.0:
                    two = op_scalar_step(kind, K, x, epsK, row, g_scalar, s_scalar, phi, slot=slot if multistep else 0,
                                         noise=nz[slot].contiguous() if with_noise else None, **kw)
                    assert torch.equal(out, two[0]), tag
                    assert not multistep or torch.equal(h_out, two[1]), tag
                    assert kind != UNIPC or torch.equal(xc_out, two[2]), tag
                    n_bits += 1
                if tuple(table[slot]) == NEUTRAL:  # the conditional part alone through the plain step formula
                    ref1 = ref_step(kind, x, eps_c.double(), row, slot, **ref_kw)[0]
                    r1, m1 = rel(out, ref1), maxrel(out, ref1)
                    worst_neutral = max(worst_neutral, r1, m1)
                    print(f"scheduled step neutral row {tag}: rel {r1:.3e} maxrel {m1:.3e}")
                    assert r1 <= 1e-6 and m1 <= 1e-6, (tag, r1, m1)
    print(f"scheduled step kernel {variant} B={B} C={Cc} h={h}: worst {worst:.3e}; neutral rows worst {worst_neutral:.3e}; "
          f"{n_bits} bit comparisons with the scalar entries")
    assert n_bits == 9 * (3 + 2)


def test_scheduled_step_refusals():
    import mrisr
    x = torch.randn((1, 4, 16, 16)).cuda()
    eps2, eps3 = torch.randn((2, 4, 16, 16)).cuda(), torch.randn((3, 4, 16, 16)).cuda()
    row = coef_row(DDIM) + [0.0] * 14
    keep = x.clone()

    def call(table, slot=0, K=2, pag_alone=0, eps=eps2, kind=DDIM, **kw):
        return op_scheduled_step(kind, K, pag_alone, x, eps, row, table, slot, **kw)

    bad = TABLE_PHI.copy()
    for col, val, what in ((0, float("nan"), "guidance_scale"), (1, -1.0, "pag_scale"), (2, 1.5, "guidance_rescale"), (2, -0.5, "guidance_rescale"),
                           (4, -1.0, "freeu_s2"), (6, float("inf"), "freeu_b2")):
        t = bad.copy()
        t[1, col] = val
        with pytest.raises(mrisr.MrisrError, match=what):
            call(t)
    with pytest.raises(mrisr.MrisrError, match="slot"):
        call(TABLE_PHI, slot=4)
    with pytest.raises(mrisr.MrisrError, match="slot"):
        call(TABLE_PHI, slot=-1)
    with pytest.raises(mrisr.MrisrError, match="2 or 3 parts"):
        call(TABLE_PHI, K=4)
    with pytest.raises(mrisr.MrisrError, match="pag alone"):
        call(TABLE_PHI, K=3, pag_alone=1, eps=eps3)
    with pytest.raises(mrisr.MrisrError, match="eps3"):
        call(TABLE_PHI, K=3, eps=eps2)
    with pytest.raises(mrisr.MrisrError, match="noise"):  # slot 2 reads slab 2: one slab is not enough
        call(TABLE_PHI, slot=2, kind=DDPM, noise=torch.randn((1, 1, 4, 16, 16)).cuda())
    with pytest.raises(mrisr.MrisrError, match="multistep"):
        call(TABLE_PHI, hist=torch.zeros((2, 1, 4, 16, 16)).cuda(), order=2)
    with pytest.raises(mrisr.MrisrError, match="history"):
        call(TABLE_PHI, kind=DPMSOLVERPP)
    torch.cuda.synchronize()
    out = call(TABLE_PHI)[0]
    assert torch.equal(x, keep) and not torch.equal(out, keep)


# ------------------------------------------------------------------------------------------------ FreeU from the table
FREEU_TABLE = np.float32([(1, 0, 0, 0.9, 0.2, 1.5, 1.6, 0), (1, 0, 0, 0.5, 1.25, 1.1, 0.75, 0), NEUTRAL, (1, 0, 0, 0.0, 0.7, 2.0, 0.3, 0)])


def op_freeu(hid, skip, hid_out, skip_out, b, s):
    L = _lib()
    B, H, W, Ch = hid.shape
    L.check(L.lib().mrisr_op_freeu(L.dtype_id(hid.dtype), hid.data_ptr(), skip.data_ptr(), hid_out.data_ptr(), skip_out.data_ptr(), B, H, W, Ch,
                                   skip.shape[3], b, s, L.stream_ptr()))


def op_freeu_scheduled(hid, skip, hid_out, skip_out, stage, table, slot, dtype=None, geo=None):
    L = _lib()
    B, H, W, Ch = hid.shape
    geo = geo if geo is not None else (B, H, W, Ch, skip.shape[3])
    tbl = np.ascontiguousarray(table, dtype=np.float32)
    L.check(L.lib().mrisr_op_freeu_scheduled(L.dtype_id(hid.dtype) if dtype is None else dtype, hid.data_ptr(), skip.data_ptr(), hid_out.data_ptr(),
                                             skip_out.data_ptr(), *geo, stage, tbl.ctypes.data_as(C.c_void_p), len(tbl), slot, L.stream_ptr()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,W,Ch,Cs", [(2, 8, 8, 32, 16), (1, 5, 3, 32, 8), (2, 16, 16, 64, 64)])
def test_freeu_stage_from_the_table(B, H, W, Ch, Cs, dtype):
    gen = torch.Generator().manual_seed(3600 + H * 10 + W + Ch)
    hid = (2.0 * torch.randn((B, H, W, Ch), generator=gen)).to(dtype).cuda()
    skip = (torch.randn((B, H, W, Cs), generator=gen) + 1.5 + 0.3 * torch.arange(W).view(1, 1, W, 1)).to(dtype).cuda()
    hid0, skip0 = hid.clone(), skip.clone()
    for stage in (0, 1):
        for slot in range(4):
            s, b = float(FREEU_TABLE[slot][3 + stage]), float(FREEU_TABLE[slot][5 + stage])
            tag = (dtype, B, H, W, Ch, Cs, stage, slot)
            ho, so = torch.full_like(hid, float("nan")), torch.full_like(skip, float("nan"))
            op_freeu_scheduled(hid, skip, ho, so, stage, FREEU_TABLE, slot)
            hv, sv = torch.full_like(hid, float("nan")), torch.full_like(skip, float("nan"))
            op_freeu(hid, skip, hv, sv, b, s)
            hi, si = hid.clone(), skip.clone()
            op_freeu_scheduled(hi, si, hi, si, stage, FREEU_TABLE, slot)  # in place, as the UNet runs it
            torch.cuda.synchronize()
            assert torch.equal(hid, hid0) and torch.equal(skip, skip0), tag
            assert bool(torch.isfinite(ho).all()) and bool(torch.isfinite(so).all()), tag
            assert torch.equal(ho, hv) and torch.equal(so, sv), tag       # the row read from the table: the by-value launch, bit for bit
            assert torch.equal(hi, hv) and torch.equal(si, sv), tag
            if slot == 2:  # the (1, 1) row: both tensors bit-identical
                assert torch.equal(ho, hid) and torch.equal(so, skip), tag
            else:
                assert not torch.equal(ho, hid) and not torch.equal(so, skip), tag


def test_freeu_scheduled_refusals_launch_nothing():
    import mrisr
    L = _lib()
    B, H, W, Ch, Cs = 2, 4, 4, 32, 16
    hid, skip = torch.randn((B, H, W, Ch)).cuda(), torch.randn((B, H, W, Cs)).cuda()
    ho, so = torch.full_like(hid, float("nan")), torch.full_like(skip, float("nan"))
    for kw, what in ((dict(stage=2), "stage"), (dict(stage=-1), "stage"), (dict(slot=4), "slot"), (dict(slot=-1), "slot"),
                     (dict(geo=(B, H, W, 24, Cs)), "multiple of 16"), (dict(geo=(B, H, W, Ch, 12)), "multiple of 8"),
                     (dict(geo=(0, H, W, Ch, Cs)), "at least 1")):
        args = dict(stage=0, slot=0)
        args.update(kw)
        with pytest.raises(mrisr.MrisrError, match=what):
            op_freeu_scheduled(hid, skip, ho, so, args["stage"], FREEU_TABLE, args["slot"], geo=args.get("geo"))
    for col, val, what in ((3, -0.1, "freeu_s1"), (4, float("nan"), "freeu_s2"), (5, -2.0, "freeu_b1"), (6, float("inf"), "freeu_b2")):
        t = FREEU_TABLE.copy()
        t[3, col] = val
        with pytest.raises(mrisr.MrisrError, match=what):
            op_freeu_scheduled(hid, skip, ho, so, 0, t, 0)
    with pytest.raises(mrisr.MrisrError):
        op_freeu_scheduled(hid, skip, ho, so, 0, FREEU_TABLE, 0, dtype=L.MRISR_I64)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ho).all()) and bool(torch.isnan(so).all())  # nothing was launched
    op_freeu_scheduled(hid, skip, ho, so, 0, FREEU_TABLE, 0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ho).all()) and bool(torch.isfinite(so).all())


# ------------------------------------------------------------------------------------------------ mrisr_sampler_set_schedule
def test_set_schedule_refusals_name_the_field():
    """Refused before any device work: n_rows != n_steps, a non-finite value, s < 0, phi outside [0, 1], a FreeU value < 0."""
    import mrisr
    from oracle import unet as ou
    L = _lib()
    cfg = ou.TINY
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32")
    net.load_state_dict(ou.init_unet_params(cfg, seed=3701, perturb_norm=True))
    sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(4)
    smp = mrisr.Sampler(net, sp, kind="ddim")

    def set_rows(rows, n=None):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        L.check(L.lib().mrisr_sampler_set_schedule(smp._h, rows.ctypes.data_as(C.c_void_p), len(rows) if n is None else n))

    good = TABLE_PHI.copy()
    set_rows(good)
    for n in (3, 5):
        with pytest.raises(mrisr.MrisrError, match="n_rows"):
            set_rows(np.tile(good[0], (n, 1)))
    with pytest.raises(mrisr.MrisrError, match="n_rows"):
        set_rows(good, n=0)  # rows with a zero count: neither a table nor the clearing call
    nan, inf = float("nan"), float("inf")
    cases = [(0, nan, "guidance_scale"), (0, inf, "guidance_scale"), (1, nan, "pag_scale"), (2, nan, "guidance_rescale"), (7, inf, "padding"),
             (1, -1e-3, "pag_scale"), (2, -0.1, "guidance_rescale"), (2, 1.0001, "guidance_rescale")]
    cases += [(c, v, name) for c, name in ((3, "freeu_s1"), (4, "freeu_s2"), (5, "freeu_b1"), (6, "freeu_b2")) for v in (-0.5, nan, -inf)]
    for col, val, what in cases:
        rows = good.copy()
        rows[2, col] = val
        with pytest.raises(mrisr.MrisrError, match=what):
            set_rows(rows)
    L.check(L.lib().mrisr_sampler_set_schedule(smp._h, None, 0))  # NULL / 0 clears
    # and through Python: check_schedule refuses the same tables with a ValueError before the library is asked
    x = torch.randn((1, 4, 16, 16)).cuda()
    keep = x.clone()
    rows = good.copy()
    rows[1, 2] = 1.5
    with pytest.raises(ValueError, match="guidance_rescale"):
        smp.run(x, torch.randn((1, 77, cfg.cross_attention_dim)).cuda(), schedule=rows)
    with pytest.raises(ValueError, match="shape"):
        smp.run(x, torch.randn((1, 77, cfg.cross_attention_dim)).cuda(), schedule=good[:3])
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
