"""GPU: the multi-tensor scaled add of the conditioning table alone, through ``mrisr_op_cond_add``:

    x_k[j] = round_T( fma(f_k, r_k[j], x_k[j]) )        f_k = w_k * table[4 * slot + col]   (f32, the product rounded once; no table: w_k)

f32 and bf16, over four pair lists - the 13 residuals of the TINY ControlNet at 16 x 16 latents and B = 2 (the 16-byte path, 13 pairs in
one launch), 324 elements (a multiple of 4 but not of 8: the bf16 scalar tail), an r pointer offset by one element (the unaligned route)
and 2B rows of x with the row range [B, 2B) and B rows of r (guess mode's range) - each with table slots 0 and 3, columns 0 and 1, the
weights 1 and the guess-mode weights, and without a table.

Bounds.  f32 against the float64 formula on the same inputs: max-relative 1e-5, what the step kernels meet for one fused multiply-add on
O(1) operands.  bf16: 2^-8 max-relative (inputs exact in bf16, the result rounded once: half an ulp is 2^-9 of the value).  At f = 1 the
result is x + r as ``launch_add_inplace`` forms it (one f32 add, one rounding to T), bit for bit; at f = 0 it is x, bit for bit (inputs
without -0); rows outside the range keep their bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from pag_testlib import maxrel

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

B = 2
TINY_RES = [(64, 16)] * 3 + [(64, 8)] + [(128, 8)] * 2 + [(128, 4)] + [(256, 4)] * 2 + [(256, 2)] * 3 + [(256, 2)]  # 12 down + mid: (C, H)
DTYPES = [torch.float32, torch.bfloat16]


def _lib():
    import mrisr
    return mrisr._lib


def cond_add(xs, rs, per_row, weights, table=None, slot=0, col=0, row_lo=0, row_hi=None, dtype=None, ptrs=None):
    """One launch.  xs / rs: CUDA tensors (x updated in place); per_row: elements per batch row of each pair."""
    L = _lib()
    n = len(xs)
    xp, rp = ptrs if ptrs is not None else ([x.data_ptr() for x in xs], [r.data_ptr() for r in rs])
    ax, ar = (C.c_void_p * n)(*xp), (C.c_void_p * n)(*rp)
    ap = (C.c_int64 * n)(*[int(p) for p in per_row])
    w = np.ascontiguousarray(weights, dtype=np.float32)
    tbl = None if table is None else np.ascontiguousarray(table, dtype=np.float32)
    L.check(L.lib().mrisr_op_cond_add(L.dtype_id(xs[0].dtype) if dtype is None else dtype, n, ax, ar, ap, w.ctypes.data_as(C.c_void_p),
                                      None if tbl is None else tbl.ctypes.data_as(C.c_void_p), 0 if tbl is None else len(tbl), slot, col,
                                      row_lo, xs[0].shape[0] if row_hi is None else row_hi, L.stream_ptr()))


def make(shape, dtype, seed):
    """Values exact in bf16 (so both dtypes see the same numbers), O(1), no zeros of either sign."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g).to(torch.bfloat16).float()
    v = torch.where(v == 0, torch.ones_like(v), v)
    return v.to(dtype).cuda().contiguous()


def pair_lists(dtype, which):
    """(xs, rs, per_row, row_lo, row_hi): NHWC tensors [rows, H, W, C]."""
    if which == "tiny13":
        xs = [make((B, h, h, c), dtype, 100 + k) for k, (c, h) in enumerate(TINY_RES)]
        rs = [make((B, h, h, c), dtype, 200 + k) for k, (c, h) in enumerate(TINY_RES)]
        return xs, rs, [h * h * c for c, h in TINY_RES], 0, B
    if which == "tail324":
        return [make((1, 3, 3, 36), dtype, 301)], [make((1, 3, 3, 36), dtype, 302)], [324], 0, 1
    if which == "unaligned":
        x = make((B, 5, 5, 24), dtype, 311)
        r = make((B * 5 * 5 * 24 + 1,), dtype, 312)[1:]  # one element past a 16-byte boundary
        assert r.data_ptr() % 16 != 0 and x.data_ptr() % 16 == 0
        return [x], [r], [5 * 5 * 24], 0, B
    assert which == "rowrange"
    return [make((2 * B, 4, 4, 64), dtype, 321)], [make((B, 4, 4, 64), dtype, 322)], [4 * 4 * 64], B, 2 * B


def reference(xs, rs, per_row, fs, row_lo, row_hi):
    """The float64 formula, rows outside the range unchanged."""
    out = []
    for x, r, p, f in zip(xs, rs, per_row, fs):
        y = x.double().cpu().reshape(x.shape[0], -1).clone()
        y[row_lo:row_hi] += float(f) * r.double().cpu().reshape(row_hi - row_lo, p)
        out.append(y.reshape(x.shape))
    return out


def weights_of(n, guess):
    import mrisr
    if not guess:
        return np.ones(n, dtype=np.float32)
    return mrisr.guess_mode_weights(n - 1) if n > 1 else np.float32([10.0 ** -0.5])


TABLE = np.float32([[0.5, 0.75, 0, 0], [9, 9, 0, 0], [9, 9, 0, 0], [1.25, -0.375, 0, 0], [9, 9, 0, 0]])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("which", ["tiny13", "tail324", "unaligned", "rowrange"])
def test_against_float64(which, dtype):
    bound = 1e-5 if dtype == torch.float32 else 2.0 ** -8
    for guess in (False, True):
        for slot, col in ((0, 0), (0, 1), (3, 0), (3, 1), (None, None)):
            xs, rs, per, lo, hi = pair_lists(dtype, which)
            w = weights_of(len(xs), guess)
            fs = w.astype(np.float64) * (1.0 if slot is None else float(TABLE[slot, col]))
            want = reference(xs, rs, per, fs, lo, hi)
            before = [x.clone() for x in xs]
            cond_add(xs, rs, per, w, None if slot is None else TABLE, slot or 0, col or 0, lo, hi)
            torch.cuda.synchronize()
            worst = max(maxrel(x, y) for x, y in zip(xs, want))
            print(f"cond_add {which} {dtype} guess={guess} slot={slot} col={col}: worst max-relative {worst:.3e} (bound {bound:.3e})")
            assert worst <= bound, (which, dtype, guess, slot, col, worst)
            for x, b in zip(xs, before):  # rows outside the range keep their bits
                assert torch.equal(x[:lo], b[:lo]) and torch.equal(x[hi:], b[hi:])
                assert not torch.equal(x[lo:hi], b[lo:hi])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("which", ["tiny13", "tail324", "unaligned", "rowrange"])
def test_factor_one_is_add_inplace_and_factor_zero_is_x(which, dtype):
    one = np.float32([[1, 1, 0, 0], [0, 0, 0, 0]])
    for table, slot in ((None, 0), (one, 0)):
        xs, rs, per, lo, hi = pair_lists(dtype, which)
        want = []
        for x, r in zip(xs, rs):  # add_inplace: from_f32<T>(to_f32(x) + to_f32(y))
            y = x.clone()
            y[lo:hi] = (x[lo:hi].float() + r.reshape(x[lo:hi].shape).float()).to(dtype)
            want.append(y)
        cond_add(xs, rs, per, np.ones(len(xs), np.float32), table, slot, 0, lo, hi)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(xs, want)), (which, dtype, "f = 1")
    for table, slot, w in ((one, 1, 1.0), (None, 0, 0.0)):  # f = 0 from the table's row, and from a zero weight
        xs, rs, per, lo, hi = pair_lists(dtype, which)
        before = [x.clone() for x in xs]
        cond_add(xs, rs, per, np.full(len(xs), w, np.float32), table, slot, 1, lo, hi)
        torch.cuda.synchronize()
        assert all(torch.equal(x, b) for x, b in zip(xs, before)), (which, dtype, "f = 0")


def test_refusals_before_any_launch():
    import mrisr
    L = _lib()
    xs, rs, per, lo, hi = pair_lists(torch.float32, "rowrange")
    before = xs[0].clone()
    ok = dict(weights=np.ones(1, np.float32), table=TABLE, slot=0, col=0, row_lo=lo, row_hi=hi)
    xp, rp = xs[0].data_ptr(), rs[0].data_ptr()
    nan = np.float32([[np.nan, 1, 0, 0]])
    cases = [(dict(ptrs=([None], [rp])), "null"), (dict(ptrs=([xp], [None])), "null"), (dict(ptrs=([xp + 2], [rp])), "aligned"),
             (dict(row_lo=2, row_hi=2), "row range"), (dict(row_lo=-1), "row range"), (dict(slot=5), "slot"), (dict(slot=-1), "slot"),
             (dict(col=2), "column"), (dict(table=nan), "not finite"), (dict(table=np.float32([[1, 1, 0.5, 0]])), "column 2"),
             (dict(weights=np.float32([np.inf])), "finite"), (dict(dtype=L.MRISR_F16), "f32 or bf16")]
    for kw, word in cases:
        with pytest.raises(mrisr.MrisrError, match=word):
            cond_add(xs, rs, per, **dict(ok, **kw))
    with pytest.raises(mrisr.MrisrError, match="empty"):
        cond_add(xs, rs, [0], **ok)
    with pytest.raises(mrisr.MrisrError, match="pairs"):
        cond_add(xs * 17, rs * 17, per * 17, **dict(ok, weights=np.ones(17, np.float32)))
    torch.cuda.synchronize()
    assert torch.equal(xs[0], before)
