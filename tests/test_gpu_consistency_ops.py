"""GPU: the consistency kernel alone (``mrisr_op_consistency``) against tests/consistency_ref.py in float64.

Bound, per element:  |out - ref64| <= 1e-5 (|alpha| max|ref| + |beta| max|lr| + |sigma| max|z| + max|x|) - the project's f32 bound
(test_gpu_freeu_ops.py).  With N <= 8 a block sum has at most 64 terms, worst-case relative error 64 * 2^-24 = 3.8e-6 of the largest
term; the few roundings of d and of the interpolation stay under the rest.

Planes and factors (h, w, N): (6, 6, 3) takes the scalar path, (12, 20, 4) a 3 x 5 coarse grid, (16, 16, 8) a 2 x 2 grid where both edge
clamps meet, (128, 128, 2) the largest accepted LDS need; B in {1, 3}, C in {1, 4}, K in {1, 2, 3}, both filters, with and without lr
and noise, the step counter at the first and the last row (row and slab offsets).  Every part of xK equals x bit for bit; "nearest" at
w = 1 is a projection (pooled out == pooled target) within the same bound; w = 0 leaves every bit, NaN-filled ref and noise included;
two runs, and the 16-byte and scalar paths, give the same bits; sources are unchanged; every refusal raises and launches nothing."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import consistency_ref as kr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPES = ((2, 2, 2), (4, 8, 2), (8, 4, 4), (6, 6, 3), (12, 20, 4), (16, 16, 4), (16, 16, 8), (32, 32, 8), (64, 64, 2), (128, 128, 2))
ROWS = np.float32(((0.7, 0.9, 0.3, 0.5), (1.0, 0.0, 0.0, 0.0), (0.45, 0.6, 0.4, 0.8)))  # the middle row is never the one read
FILTERS = {"bilinear": 0, "nearest": 1}


def op(x, xK, K, ref, lr, noise, table, step, N, filter):
    import mrisr
    L = mrisr._lib
    B, Cc, h, w = x.shape
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    L.check(L.lib().mrisr_op_consistency(ptr(x), ptr(xK), K, ptr(ref), ptr(lr), ptr(noise), ptr(table), ptr(step), B, Cc, h, w, N,
                                         FILTERS[filter] if isinstance(filter, str) else filter, L.stream_ptr()))


def bound(row, ref, lr, z, x):
    _, al, be, sg = (abs(float(v)) for v in row)
    return 1e-5 * (al * float(ref.abs().max()) + (be * float(lr.abs().max()) if lr is not None else 0.0) +
                   (sg * float(z.abs().max()) if z is not None else 0.0) + float(x.abs().max()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_N{s[2]}")
def test_consistency_op(shape):
    h, w, N = shape
    gen = torch.Generator().manual_seed(5000 + 100 * h + w)
    table = torch.from_numpy(ROWS).cuda()
    worst = 0.0
    for B, Cc in itertools.product((1, 3), (1, 4)):
        # a plane with a mean and a slope, so that the low band carries most of it
        ramp = 0.2 * torch.arange(w).view(1, 1, 1, w) + 0.1 * torch.arange(h).view(1, 1, h, 1)
        x0 = torch.randn((B, Cc, h, w), generator=gen) + 1.0
        ref = 0.8 * torch.randn((B, Cc, h, w), generator=gen) + ramp
        lr0 = 0.5 * torch.randn((B, Cc, h, w), generator=gen) - 0.5
        nz0 = torch.randn((len(ROWS), B, Cc, h, w), generator=gen)
        d_ref, d_lr0, d_nz0 = ref.cuda(), lr0.cuda(), nz0.cuda()
        for filt, with_lr, with_nz, s in itertools.product(FILTERS, (False, True), (False, True), (0, len(ROWS) - 1)):
            tag = f"consistency op {h}x{w} N={N} B={B} C={Cc} {filt} lr={with_lr} noise={with_nz} step={s}"
            lr, nz = (lr0 if with_lr else None), (nz0 if with_nz else None)
            d_lr, d_nz = (d_lr0 if with_lr else None), (d_nz0 if with_nz else None)
            step = torch.tensor([s], dtype=torch.int32).cuda()
            want = kr.apply(x0, ref, lr, nz[s] if nz is not None else None, ROWS[s], N, filt)
            bnd = bound(ROWS[s], ref, lr, nz[s] if nz is not None else None, x0)
            first = None
            for K in (1, 2, 3):
                x, xK = x0.clone().cuda(), torch.full((K * B, Cc, h, w), float("nan")).cuda()
                op(x, xK, K, d_ref, d_lr, d_nz, table, step, N, filt)
                torch.cuda.synchronize()
                err = float((x.cpu().double() - want).abs().max())
                worst = max(worst, err / bnd)
                assert err <= bnd, (tag, K, err, bnd)
                for k in range(K):
                    assert torch.equal(xK[k * B:(k + 1) * B], x), (tag, K, k)
                if first is None:
                    first = x.clone()
                assert torch.equal(x, first), (tag, K)  # the same bits for every K, and from run to run
            assert torch.equal(d_ref, ref.cuda()) and torch.equal(d_lr0, lr0.cuda()) and torch.equal(d_nz0, nz0.cuda()), tag
    print(f"consistency op {h}x{w} N={N}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_N{s[2]}")
def test_nearest_at_weight_one_is_a_projection(shape):
    h, w, N = shape
    gen = torch.Generator().manual_seed(5100 + 100 * h + w)
    B, Cc = 3, 4
    row = np.float32((1.0, 0.9, 0.3, 0.5))
    x0, ref, lr = (torch.randn((B, Cc, h, w), generator=gen) + 0.5 for _ in range(3))
    nz = torch.randn((1, B, Cc, h, w), generator=gen)
    x, xK = x0.clone().cuda(), torch.full((2 * B, Cc, h, w), float("nan")).cuda()
    op(x, xK, 2, ref.cuda(), lr.cuda(), nz.cuda(), torch.from_numpy(row).cuda(), torch.zeros(1, dtype=torch.int32).cuda(), N, "nearest")
    torch.cuda.synchronize()
    y = kr.target(ref, lr, nz[0], row)
    gap = float((F.avg_pool2d(x.cpu().double(), N) - F.avg_pool2d(y, N)).abs().max())
    bnd = bound(row, ref, lr, nz[0], x0)
    print(f"nearest projection {h}x{w} N={N}: pooled gap {gap:.3e} (bound {bnd:.3e})")
    assert gap <= bnd
    # the detail of x - what the block means do not see - is what it was
    detail = lambda t: t - F.avg_pool2d(t, N).repeat_interleave(N, 2).repeat_interleave(N, 3)  # noqa: E731
    assert float((detail(x.cpu().double()) - detail(x0.double())).abs().max()) <= bnd


def test_weight_zero_leaves_every_bit():
    gen = torch.Generator().manual_seed(5200)
    for (h, w, N), K in itertools.product(((6, 6, 3), (16, 16, 4), (128, 128, 2)), (1, 2, 3)):
        B, Cc = 3, 4
        table = torch.from_numpy(np.float32(((1.0, 1.0, 1.0, 1.0), (0.0, 1.0, 1.0, 1.0), (-0.0, 1.0, 0.0, 1.0)))).cuda()
        x0, xK0 = torch.randn((B, Cc, h, w), generator=gen), torch.randn((K * B, Cc, h, w), generator=gen)
        nan = torch.full((B, Cc, h, w), float("nan")).cuda()
        nan_nz = torch.full((3, B, Cc, h, w), float("nan")).cuda()
        for s, filt in itertools.product((1, 2), FILTERS):
            x, xK = x0.clone().cuda(), xK0.clone().cuda()
            op(x, xK, K, nan, nan, nan_nz, table, torch.tensor([s], dtype=torch.int32).cuda(), N, filt)
            torch.cuda.synchronize()
            assert torch.equal(x.cpu(), x0) and torch.equal(xK.cpu(), xK0), (h, w, N, K, s, filt)
        x, xK = x0.clone().cuda(), xK0.clone().cuda()     # row 0 of the same table does run: the launch is live
        op(x, xK, K, nan, None, None, table, torch.zeros(1, dtype=torch.int32).cuda(), N, "bilinear")
        torch.cuda.synchronize()
        assert bool(torch.isnan(x).all()) and bool(torch.isnan(xK).all())


@pytest.mark.parametrize("shape", ((4, 8, 2), (12, 20, 4), (16, 16, 8), (24, 12, 3), (64, 64, 2)), ids=lambda s: f"{s[0]}x{s[1]}_N{s[2]}")
def test_scalar_path_has_the_bits_of_the_16_byte_path(shape):
    """w % 4 == 0 with every operand 16-byte aligned takes float4 loads and stores; one operand 4 bytes off sends the launch down the
    scalar path.  One summation order in both: the same bits."""
    h, w, N = shape
    gen = torch.Generator().manual_seed(5300 + h)
    B, Cc, n = 3, 4, 3 * 4 * h * w
    x0, ref, lr = (torch.randn((B, Cc, h, w), generator=gen) for _ in range(3))
    nz = torch.randn((2, B, Cc, h, w), generator=gen)
    table = torch.from_numpy(np.float32(((1.0, 0.0, 0.0, 0.0), (0.7, 0.9, 0.3, 0.5)))).cuda()
    step = torch.ones(1, dtype=torch.int32).cuda()
    for filt in FILTERS:
        x, xK = x0.clone().cuda(), torch.full((2 * B, Cc, h, w), float("nan")).cuda()
        op(x, xK, 2, ref.cuda(), lr.cuda(), nz.cuda(), table, step, N, filt)

        def shifted(t):  # the same values at an address 4 bytes past a 16-byte boundary
            buf = torch.empty(t.numel() + 4, dtype=torch.float32).cuda()
            v = buf[1:1 + t.numel()].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4
            return v
        for which in range(5):
            ops = [x0.clone().cuda(), torch.full((2 * B, Cc, h, w), float("nan")).cuda(), ref.cuda(), lr.cuda(), nz.cuda()]
            ops[which] = shifted(ops[which])
            op(ops[0], ops[1], 2, ops[2], ops[3], ops[4], table, step, N, filt)
            torch.cuda.synchronize()
            assert torch.equal(ops[0], x) and torch.equal(ops[1], xK), (shape, filt, which)


def test_refusals_launch_nothing():
    import mrisr
    gen = torch.Generator().manual_seed(5400)
    B, Cc, h, w = 1, 1, 256, 256
    x0 = torch.randn((B, Cc, h, w), generator=gen)
    x, ref = x0.clone().cuda(), torch.randn((B, Cc, h, w), generator=gen).cuda()
    xK = torch.full((3 * B, Cc, h, w), float("nan")).cuda()
    table = torch.from_numpy(np.float32(((1.0, 1.0, 0.0, 0.0),))).cuda()
    step = torch.zeros(1, dtype=torch.int32).cuda()

    def call(K=2, N=8, filt=0, hw=(h, w), xx=x, kk=xK, rr=ref, tt=table, ss=step):
        L = mrisr._lib
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        L.check(L.lib().mrisr_op_consistency(ptr(xx), ptr(kk), K, ptr(rr), None, None, ptr(tt), ptr(ss), B, Cc, hw[0], hw[1], N, filt,
                                             L.stream_ptr()))
    cases = [(dict(N=7), "must divide"), (dict(N=3, hw=(255, 256)), "must divide"), (dict(N=3, hw=(256, 255)), "must divide"),
             (dict(N=1), "2 .. 8"), (dict(N=0), "2 .. 8"), (dict(N=16), "2 .. 8"), (dict(N=-2), "2 .. 8"),
             (dict(filt=2), "filter"), (dict(filt=-1), "filter"),
             (dict(N=2), "LDS"), (dict(N=4), "LDS"),
             (dict(K=0), "K must lie"), (dict(K=4), "K must lie"), (dict(K=-1), "K must lie"), (dict(kk=None), "staging buffer"),
             (dict(xx=None), "null"), (dict(rr=None), "null"), (dict(tt=None), "null"), (dict(ss=None), "null")]
    for kw, word in cases:
        with pytest.raises(RuntimeError, match=word):
            call(**kw)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), x0) and bool(torch.isnan(xK).all())  # nothing was launched
    call()
    torch.cuda.synchronize()
    assert not torch.equal(x.cpu(), x0) and bool(torch.isfinite(xK[:2 * B]).all()) and bool(torch.isnan(xK[2 * B:]).all())
