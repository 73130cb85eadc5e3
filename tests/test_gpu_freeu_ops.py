"""GPU: the FreeU kernel alone (``mrisr_op_freeu``), f32 and bf16, on NHWC operands.

* backbone half: a single multiply in the activation dtype - bit-equal to torch's ``x * b`` in that dtype (torch multiplies bf16 by
  a scalar in f32 and rounds once, as the kernel does); the other channels bit-equal to the input.
* skip: against diffusers' ``fourier_filter`` (tests/freeu_ref.py) in float64.  f32: |out - ref64| <= 1e-5 max|x| - the project's
  bound for an f32 tree sum plus a handful of f32 operations (test_gpu_pag_ops.py).  bf16: |out - ref64| <= 2^-8 |ref64| + 1e-5 max|x|
  with ref64 computed from the bf16 input: one rounding to bf16 on top.
* s = 1 within the same bound of the input; out of place: sources unchanged, NaN-filled outputs fully finite; in place: the same bits;
  two runs: the same bits; every refusal raises and launches nothing."""
import pytest
import torch

import freeu_ref as fr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HW = ((1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (4, 4), (4, 6), (8, 8), (16, 16))
CHANNELS = ((256, 128), (256, 256), (1280, 640), (1280, 1280), (16, 8))
B_SCALE, S_SCALE = 1.6, 0.2  # (1.6 is not a bf16 / f32 number: the product rounds)


def op_freeu(hid, skip, hid_out, skip_out, b, s):
    import mrisr
    L = mrisr._lib
    B, H, W, Ch = hid.shape
    L.check(L.lib().mrisr_op_freeu(L.dtype_id(hid.dtype), hid.data_ptr(), skip.data_ptr(), hid_out.data_ptr(), skip_out.data_ptr(), B, H, W, Ch,
                                   skip.shape[3], b, s, L.stream_ptr()))


def skip_bound(ref64, xmax, dtype):
    return (2.0 ** -8 * ref64.abs() if dtype == torch.bfloat16 else 0.0) + 1e-5 * xmax


@pytest.mark.parametrize("chs", CHANNELS, ids=lambda c: f"{c[0]}+{c[1]}")
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_freeu_op(dtype, chs):
    Ch, Cs = chs
    gen = torch.Generator().manual_seed(3200 + Ch + Cs)
    for B in (1, 3):
        for H, W in HW:
            tag = f"freeu op {dtype} B={B} {H}x{W} Ch={Ch} Cs={Cs}"
            hid = (2.0 * torch.randn((B, H, W, Ch), generator=gen)).to(dtype).cuda()
            # a plane with a mean and a slope: the filtered frequencies carry most of it
            skip = (torch.randn((B, H, W, Cs), generator=gen) + 1.5 + 0.3 * torch.arange(W).view(1, 1, W, 1)).to(dtype).cuda()
            hid0, skip0 = hid.clone(), skip.clone()
            ref64 = fr.fourier_filter(skip.cpu().double().permute(0, 3, 1, 2), 1, S_SCALE).permute(0, 2, 3, 1)
            xmax = float(skip.abs().max())
            # out of place, outputs pre-filled with NaN
            ho, so = torch.full_like(hid, float("nan")), torch.full_like(skip, float("nan"))
            op_freeu(hid, skip, ho, so, B_SCALE, S_SCALE)
            torch.cuda.synchronize()
            assert torch.equal(hid, hid0) and torch.equal(skip, skip0), tag
            assert bool(torch.isfinite(ho).all()) and bool(torch.isfinite(so).all()), tag
            assert torch.equal(ho[..., :Ch // 2], hid[..., :Ch // 2] * B_SCALE), tag
            assert torch.equal(ho[..., Ch // 2:], hid[..., Ch // 2:]), tag
            err = (so.cpu().double() - ref64).abs()
            excess = float((err - skip_bound(ref64, xmax, dtype)).max())
            print(f"{tag}: skip max abs err {float(err.max()):.3e} (max|x| {xmax:.2f}), over the bound by {excess:.3e}")
            assert excess <= 0.0, tag
            # twice: the same bits
            ho2, so2 = torch.full_like(hid, float("nan")), torch.full_like(skip, float("nan"))
            op_freeu(hid, skip, ho2, so2, B_SCALE, S_SCALE)
            # in place: the same bits
            hi, si = hid.clone(), skip.clone()
            op_freeu(hi, si, hi, si, B_SCALE, S_SCALE)
            # mixed: one operand in place, the other out of place
            hm, sm = hid.clone(), torch.full_like(skip, float("nan"))
            op_freeu(hm, skip, hm, sm, B_SCALE, S_SCALE)
            torch.cuda.synchronize()
            assert torch.equal(ho2, ho) and torch.equal(so2, so), tag
            assert torch.equal(hi, ho) and torch.equal(si, so), tag
            assert torch.equal(hm, ho) and torch.equal(sm, so) and torch.equal(skip, skip0), tag
            # s = 1 (and b = 1): the input, within the same bound
            h1, s1 = torch.full_like(hid, float("nan")), torch.full_like(skip, float("nan"))
            op_freeu(hid, skip, h1, s1, 1.0, 1.0)
            torch.cuda.synchronize()
            x64 = skip.cpu().double()
            assert float(((s1.cpu().double() - x64).abs() - skip_bound(x64, xmax, dtype)).max()) <= 0.0, tag
            assert torch.equal(h1, hid), tag


def test_freeu_op_refusals_launch_nothing():
    import mrisr
    L = mrisr._lib
    B, H, W, Ch, Cs = 2, 4, 4, 32, 16
    hid, skip = torch.randn((B, H, W, Ch)).cuda(), torch.randn((B, H, W, Cs)).cuda()
    ho, so = torch.full_like(hid, float("nan")), torch.full_like(skip, float("nan"))
    hp, sp, hop, sop = hid.data_ptr(), skip.data_ptr(), ho.data_ptr(), so.data_ptr()

    def call(ptrs, geo, b=1.5, s=0.2, dtype=None):
        L.check(L.lib().mrisr_op_freeu(L.MRISR_F32 if dtype is None else dtype, *ptrs, *geo, b, s, L.stream_ptr()))

    good_p, good_g = (hp, sp, hop, sop), (B, H, W, Ch, Cs)
    nan, inf = float("nan"), float("inf")
    cases = [((None, sp, hop, sop), good_g, {}, "null"), ((hp, None, hop, sop), good_g, {}, "null"),
             ((hp, sp, None, sop), good_g, {}, "null"), ((hp, sp, hop, None), good_g, {}, "null"),
             ((hp + 4, sp, hop, sop), good_g, {}, "aligned"), ((hp, sp + 8, hop, sop), good_g, {}, "aligned"),
             ((hp, sp, hop + 4, sop), good_g, {}, "aligned"), ((hp, sp, hop, sop + 4), good_g, {}, "aligned"),
             (good_p, (0, H, W, Ch, Cs), {}, "at least 1"), (good_p, (B, 0, W, Ch, Cs), {}, "at least 1"),
             (good_p, (B, H, -1, Ch, Cs), {}, "at least 1"),
             (good_p, (B, H, W, 24, Cs), {}, "multiple of 16"), (good_p, (B, H, W, 0, Cs), {}, "multiple of 16"),
             (good_p, (B, H, W, Ch, 12), {}, "multiple of 8"), (good_p, (B, H, W, Ch, 0), {}, "multiple of 8")]
    for bad in (-0.5, nan, inf):
        cases.append((good_p, good_g, dict(b=bad), "finite"))
        cases.append((good_p, good_g, dict(s=bad), "finite"))
    for ptrs, geo, kw, what in cases:
        with pytest.raises(RuntimeError, match=what):
            call(ptrs, geo, **kw)
    with pytest.raises(RuntimeError):
        call(good_p, good_g, dtype=L.MRISR_I64)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ho).all()) and bool(torch.isnan(so).all())  # nothing was launched
    call(good_p, good_g)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ho).all()) and bool(torch.isfinite(so).all())
