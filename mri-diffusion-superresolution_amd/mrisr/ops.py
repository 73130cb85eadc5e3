"""Single-op entry points of the C ABI (``mrisr_op_*``): the same kernels the models launch, exposed so the parity
tests can check each one against a plain PyTorch reference of the op."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L


def _nhwc(x: torch.Tensor):
    """torch NCHW tensor -> (contiguous NHWC buffer, descriptor with logical NCHW shape)."""
    buf = x.permute(0, 2, 3, 1).contiguous()
    return buf, L.as_tensor(buf, L.MRISR_NHWC, shape=x.shape)


def _f32(x: Optional[torch.Tensor]):
    return None if x is None else C.c_void_p(x.detach().to(torch.float32).contiguous().data_ptr())


def conv3x3(x, weight, bias=None, x2=None, stride=1, upsample=False, act=L.ACT_NONE, splitk=0, tile=0, subpix=False):
    """x [B,C,H,W] (bf16/f32, cuda), weight [Cout,Cin,3,3] f32.  Returns NCHW tensor of x.dtype.  ``upsample``: nearest x2 first
    (diffusers Upsample2D); with ``subpix`` in its sub-pixel form (four 2 x 2 parity convs on the low-resolution input, bf16)."""
    xb, tx = _nhwc(x)
    t2 = None
    if x2 is not None:
        x2b, t2 = _nhwc(x2)
    w = weight.detach().to(torch.float32).contiguous()
    b = bias.detach().to(torch.float32).contiguous() if bias is not None else None
    B, _, H, W = x.shape
    Hc, Wc = (H * 2, W * 2) if upsample else (H, W)
    Ho, Wo = (Hc - 1) // stride + 1, (Wc - 1) // stride + 1
    cout = w.shape[0]
    yb = torch.empty((B, Ho, Wo, cout), dtype=x.dtype, device=x.device)
    ty = L.as_tensor(yb, L.MRISR_NHWC, shape=(B, cout, Ho, Wo))
    L.check(L.lib().mrisr_op_conv3x3(C.byref(tx), C.byref(t2) if t2 else None, C.c_void_p(w.data_ptr()),
                                     C.c_void_p(b.data_ptr()) if b is not None else None, cout, stride,
                                     (2 if subpix else 1) if upsample else 0, act, splitk, tile, C.byref(ty), L.stream_ptr()))
    return yb.permute(0, 3, 1, 2)


def conv3x3_sc(x, weight, bias, xs, weight_sc, bias_sc, x2=None, xs2=None, splitk=0, tile=0, fused=True):
    """A resnet's conv2 with its 1x1 shortcut (bf16): conv3x3([x | x2]) + bias + weight_sc [xs | xs2] + bias_sc.  ``fused``: one launch with
    the shortcut as the 1x1 tail of the conv's K loop; otherwise the shortcut GEMM followed by the conv with it as residual."""
    bufs = [_nhwc(t) if t is not None else (None, None) for t in (x, x2, xs, xs2)]
    w = weight.detach().to(torch.float32).contiguous()
    ws = weight_sc.detach().to(torch.float32).reshape(weight_sc.shape[0], -1).contiguous()
    b, bs = (t.detach().to(torch.float32).contiguous() for t in (bias, bias_sc))
    B, _, H, W = x.shape
    cout = w.shape[0]
    yb = torch.empty((B, H, W, cout), dtype=x.dtype, device=x.device)
    ty = L.as_tensor(yb, L.MRISR_NHWC, shape=(B, cout, H, W))
    ref = lambda d: C.byref(d) if d is not None else None
    L.check(L.lib().mrisr_op_conv3x3_sc(ref(bufs[0][1]), ref(bufs[1][1]), C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()),
                                        ref(bufs[2][1]), ref(bufs[3][1]), C.c_void_p(ws.data_ptr()), C.c_void_p(bs.data_ptr()), cout,
                                        splitk, tile, 1 if fused else 0, C.byref(ty), L.stream_ptr()))
    return yb.permute(0, 3, 1, 2)


def ff_proj(h, t, x, w2, b2, wp, bp, tile=0, fused=True):
    """A transformer block's ff.net.2 followed by the transformer's proj_out (bf16 rows): (h w2^T + b2 + t) wp^T + bp + x with h [M,K4],
    t / x [M,C], w2 [C,K4], wp [C,C].  ``fused``: one launch over K = [K4 | C] on the composed weight [wp w2 | wp]; otherwise the two launches."""
    h, t, x = h.contiguous(), t.contiguous(), x.contiguous()
    f = lambda a: a.detach().to(torch.float32).contiguous() if a is not None else None
    w2f, b2f, wpf, bpf = (f(a) for a in (w2, b2, wp.reshape(wp.shape[0], -1), bp))
    y = torch.empty_like(x)
    th, tt, tx, ty = (L.as_tensor(a) for a in (h, t, x, y))
    p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None
    L.check(L.lib().mrisr_op_ff_proj(C.byref(th), C.byref(tt), C.byref(tx), p(w2f), p(b2f), p(wpf), p(bpf), tile, 1 if fused else 0,
                                     C.byref(ty), L.stream_ptr()))
    return y


def linear(x, weight, bias=None, act=L.ACT_NONE, splitk=0, tile=0):
    """x [M,K], weight [N,K] f32 -> [M,N] (GEGLU: [M,N/2])."""
    x = x.contiguous()
    w = weight.detach().to(torch.float32).contiguous()
    b = bias.detach().to(torch.float32).contiguous() if bias is not None else None
    n = w.shape[0]
    y = torch.empty((x.shape[0], n // 2 if act == L.ACT_GEGLU else n), dtype=x.dtype, device=x.device)
    tx, ty = L.as_tensor(x), L.as_tensor(y)
    L.check(L.lib().mrisr_op_linear(C.byref(tx), C.c_void_p(w.data_ptr()),
                                    C.c_void_p(b.data_ptr()) if b is not None else None, n, act, splitk, tile,
                                    C.byref(ty), L.stream_ptr()))
    return y


def linear_resid(x, weight, bias=None, rowvec=None, lora_a=None, lora_b=None, lora_scale=1.0, resid=None, out=None, splitk=0, tile=0):
    """x [M,K] bf16, weight [N,K] -> x weight^T + bias + rowvec[m // (M // R)] + lora_scale * lora_b (lora_a x) + resid: a projection with all
    its epilogue operands.  rowvec [R,N] f32 (R divides M; R = 1: one row for every output row), lora_a [r,K], lora_b [N,r], resid [M,N]
    bf16.  ``out``: the output tensor; passing ``resid`` itself runs the projection in place."""
    x = x.contiguous()
    f = lambda a: a.detach().to(torch.float32).contiguous() if a is not None else None
    w, b, rv, la, lb = (f(a) for a in (weight, bias, rowvec, lora_a, lora_b))
    n = w.shape[0]
    y = out if out is not None else torch.empty((x.shape[0], n), dtype=x.dtype, device=x.device)
    tx, ty = L.as_tensor(x), L.as_tensor(y)
    tr = L.as_tensor(resid) if resid is not None else None
    p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None
    L.check(L.lib().mrisr_op_linear_resid(C.byref(tx), p(w), p(b), n, p(rv), rv.shape[0] if rv is not None else 0, p(la), p(lb),
                                          la.shape[0] if la is not None else 0, C.c_float(lora_scale), C.byref(tr) if tr is not None else None,
                                          splitk, tile, C.byref(ty), L.stream_ptr()))
    return y


def ln_linear(x, gamma, beta, weight, bias=None, act=L.ACT_NONE):
    """LayerNorm(x) W^T + bias, the normalisation fused into the row-panel GEMM (bf16, K = 320 / 640)."""
    x = x.contiguous()
    w = weight.detach().to(torch.float32).contiguous()
    b = bias.detach().to(torch.float32).contiguous() if bias is not None else None
    ga, be = (t.detach().to(torch.float32).contiguous() for t in (gamma, beta))
    n = w.shape[0]
    y = torch.empty((x.shape[0], n // 2 if act == L.ACT_GEGLU else n), dtype=x.dtype, device=x.device)
    tx, ty = L.as_tensor(x), L.as_tensor(y)
    L.check(L.lib().mrisr_op_ln_linear(C.byref(tx), C.c_void_p(ga.data_ptr()), C.c_void_p(be.data_ptr()), C.c_void_p(w.data_ptr()),
                                       C.c_void_p(b.data_ptr()) if b is not None else None, n, act, C.byref(ty), L.stream_ptr()))
    return y


def mlp(x, gamma, beta, w1, b1, w2, b2, residual=True, wp=None, bp=None, xres=None):
    """x + FF2(GEGLU(FF1(LayerNorm(x)))) in one kernel (bf16 rows of width 320; the hidden activation stays on-chip):
    w1 [2H][320] = diffusers ff.net.0.proj.weight (value half then gate half), w2 [320][H] = ff.net.2.weight.
    With ``wp`` [320][320] (and ``xres`` [M][320], optionally ``bp``) the kernel's continuation runs as well and ITS result is
    returned: (the above) wp^T + bp + xres, the transformer's proj_out and outer residual (whole 128-row panels only)."""
    x = x.contiguous()
    f = lambda t: t.detach().to(torch.float32).contiguous() if t is not None else None
    ga, be, w1f, b1f, w2f, b2f, wpf, bpf = (f(t) for t in (gamma, beta, w1, b1, w2, b2, wp, bp))
    hidden = w2f.shape[1]
    y = torch.empty((x.shape[0], w2f.shape[0]), dtype=x.dtype, device=x.device)
    tx, ty = L.as_tensor(x), L.as_tensor(y)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    if wp is not None or bp is not None or xres is not None:
        if wp is None or xres is None:
            raise L.MrisrError("mlp: the proj_out continuation needs wp and xres")
        if wpf.shape != (y.shape[1], y.shape[1]) or (bpf is not None and bpf.shape != (y.shape[1],)):
            raise L.MrisrError("mlp: wp [320][320], bp [320]")
        xr = xres.contiguous()
        txr = L.as_tensor(xr)
        L.check(L.lib().mrisr_op_mlp_proj(C.byref(tx), p(ga), p(be), p(w1f), p(b1f), p(w2f), p(b2f), hidden, 1 if residual else 0,
                                          p(wpf), p(bpf), C.byref(txr), C.byref(ty), L.stream_ptr()))
        return y
    L.check(L.lib().mrisr_op_mlp(C.byref(tx), p(ga), p(be), p(w1f), p(b1f), p(w2f), p(b2f), hidden, 1 if residual else 0,
                                 C.byref(ty), L.stream_ptr()))
    return y


def xattn_tail(ao, t, ntok, w1, b1, gamma, beta, wq, bq, w2, b2, k, v, nk=None, lora=None, lora_scale=1.0):
    """The row-local middle of a C = 320 transformer block in one kernel (csrc/xtail.hip):
    x1 = ao w1^T + b1 + t;  q = LayerNorm(x1; gamma, beta) wq^T + bq;  o = softmax(q k^T / sqrt(40)) v over 8 heads;
    returns o w2^T + b2 + x1.  ao [M][ldao], t [M][ldt] bf16 rows whose second extent is the row pitch (>= 320, columns beyond 320
    are padding); the kernel works in place on ``t``, so a clone of it is passed and returned, padding included.  ``ntok`` tokens
    per image; k, v the projected prompt rows, bf16 [M / ntok][keys][320], of which the first ``nk`` (default: all) are attended
    to.  ``lora``: three rank-4 adapters ((A1, B1), (Aq, Bq), (A2, B2)), A [4][320], B [320][4], all scaled by ``lora_scale``;
    a pair may be None, which the library refuses unless all three are."""
    ao, k, v = ao.contiguous(), k.contiguous(), v.contiguous()
    out = t.contiguous().clone()
    f = lambda a: a.detach().to(torch.float32).contiguous() if a is not None else None
    w1f, b1f, gaf, bef, wqf, bqf, w2f, b2f = (f(a) for a in (w1, b1, gamma, beta, wq, bq, w2, b2))
    if lora is not None and len(lora) != 3:
        raise L.MrisrError("xattn_tail: lora is three (A, B) pairs, for attn1.to_out, attn2.to_q and attn2.to_out")
    ad = [f(a) for pair in (lora or ()) for a in (pair if pair is not None else (None, None))] or [None] * 6
    rank = next((int(a.shape[0]) for a in ad[0::2] if a is not None), 0)
    # (the library sees pointers only: what it will read through them is checked here)
    if any(a.shape != (320, 320) for a in (w1f, wqf, w2f)) or any(a.shape != (320,) for a in (b1f, gaf, bef, bqf, b2f) if a is not None):
        raise L.MrisrError("xattn_tail: weights [320][320], vectors [320]")
    if any(a is not None and a.shape != s for pair in zip(ad[0::2], ad[1::2]) for a, s in zip(pair, ((rank, 320), (320, rank)))):
        raise L.MrisrError("xattn_tail: adapters A [r][320], B [320][r], one rank")
    tao, tt, tk, tv = (L.as_tensor(a) for a in (ao, out, k, v))
    p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None
    L.check(L.lib().mrisr_op_xattn_tail(C.byref(tao), C.byref(tt), int(ntok), p(w1f), p(b1f), p(gaf), p(bef), p(wqf), p(bqf), p(w2f), p(b2f),
                                        C.byref(tk), C.byref(tv), int(k.shape[1] if nk is None else nk), *(p(a) for a in ad), rank,
                                        float(lora_scale), L.stream_ptr()))
    return out


def linear_fp8(x, weight, bias=None, act=L.ACT_NONE, gamma=None, beta=None):
    """[LayerNorm(x)] W^T + bias with OCP e4m3 operands on the fp8 MFMA (row-panel kernel; bf16 in / out, K = 320 / 640)."""
    x = x.contiguous()
    w = weight.detach().to(torch.float32).contiguous()
    b = bias.detach().to(torch.float32).contiguous() if bias is not None else None
    ga = gamma.detach().to(torch.float32).contiguous() if gamma is not None else None
    be = beta.detach().to(torch.float32).contiguous() if beta is not None else None
    n = w.shape[0]
    y = torch.empty((x.shape[0], n // 2 if act == L.ACT_GEGLU else n), dtype=x.dtype, device=x.device)
    tx, ty = L.as_tensor(x), L.as_tensor(y)
    L.check(L.lib().mrisr_op_linear_fp8(C.byref(tx), C.c_void_p(ga.data_ptr()) if ga is not None else None,
                                        C.c_void_p(be.data_ptr()) if be is not None else None, C.c_void_p(w.data_ptr()),
                                        C.c_void_p(b.data_ptr()) if b is not None else None, n, act, C.byref(ty), L.stream_ptr()))
    return y


def groupnorm(x, gamma, beta, groups=32, eps=1e-5, silu=False, x2=None):
    xb, tx = _nhwc(x)
    t2 = None
    ctot = x.shape[1]
    if x2 is not None:
        x2b, t2 = _nhwc(x2)
        ctot += x2.shape[1]
    g = gamma.detach().to(torch.float32).contiguous()
    b = beta.detach().to(torch.float32).contiguous()
    B, _, H, W = x.shape
    yb = torch.empty((B, H, W, ctot), dtype=x.dtype, device=x.device)
    ty = L.as_tensor(yb, L.MRISR_NHWC, shape=(B, ctot, H, W))
    L.check(L.lib().mrisr_op_groupnorm(C.byref(tx), C.byref(t2) if t2 else None, C.c_void_p(g.data_ptr()),
                                       C.c_void_p(b.data_ptr()), groups, C.c_float(eps), 1 if silu else 0,
                                       C.byref(ty), L.stream_ptr()))
    return yb.permute(0, 3, 1, 2)


def layernorm(x, gamma, beta, eps=1e-5):
    x = x.contiguous()
    g = gamma.detach().to(torch.float32).contiguous()
    b = beta.detach().to(torch.float32).contiguous()
    y = torch.empty_like(x)
    tx, ty = L.as_tensor(x), L.as_tensor(y)
    L.check(L.lib().mrisr_op_layernorm(C.byref(tx), C.c_void_p(g.data_ptr()), C.c_void_p(b.data_ptr()), C.c_float(eps),
                                       C.byref(ty), L.stream_ptr()))
    torch.cuda.current_stream().synchronize()
    return y


def attention(q, k, v, heads, flash=True, fp8=False):
    """q [B,N,C], k/v [B,Nk,C] -> [B,N,C]  (softmax(q k^T / sqrt(d)) v per head).  ``fp8``: Q K^T and P V with OCP e4m3 operands
    (per-head scales, f32 softmax) - BASELINE configs[4]."""
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    out = torch.empty_like(q)
    tq, tk, tv, to = (L.as_tensor(t) for t in (q, k, v, out))
    L.check(L.lib().mrisr_op_attention(C.byref(tq), C.byref(tk), C.byref(tv), heads, 2 if fp8 else (1 if flash else 0), C.byref(to),
                                       L.stream_ptr()))
    return out


def attention_backward(q, k, v, dout, heads):
    """Gradients (dq, dk, dv) of ``attention`` w.r.t. its bf16 inputs for an upstream ``dout`` [B,N,C]: the flash
    forward (keeping the log-sum-exp) followed by the two backward kernels the fine-tuning step uses."""
    q, k, v, dout = (t.contiguous() for t in (q, k, v, dout))
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ts = [L.as_tensor(t) for t in (q, k, v, dout, dq, dk, dv)]
    L.check(L.lib().mrisr_op_attention_bwd(C.byref(ts[0]), C.byref(ts[1]), C.byref(ts[2]), C.byref(ts[3]), heads,
                                           C.byref(ts[4]), C.byref(ts[5]), C.byref(ts[6]), L.stream_ptr()))
    return dq, dk, dv


# ---- the backward (mrisr_op_*_bwd and friends): thin wrappers over raw device pointers.  Tensors are used as they are (contiguous, on
# the GPU, already in the kernels' layouts: NHWC activations, token rows); outputs that a kernel adds into are passed in by the caller.
def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous():
        raise L.MrisrError("backward ops take contiguous GPU tensors")
    return t.data_ptr()


def _dt(t: torch.Tensor) -> int:
    return L.dtype_id(t.dtype)


def groupnorm_backward(x, dy, gamma, beta, groups=32, eps=1e-5, silu=False, x2=None, dx=None, dx2=None, acc=False, acc2=False,
                       g_gamma=None, g_beta=None):
    """x [B,HW,c0] (and x2 [B,HW,c1]) NHWC rows, dy [B,HW,c0+c1]; returns (dx, dx2).  ``dx`` / ``dx2`` given with ``acc`` / ``acc2``: the
    gradient is added into them.  ``g_gamma`` / ``g_beta`` (f32 [c0], x2 None): the affine gradients are added into them."""
    B, HW, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[2]
    dx = torch.empty_like(x) if dx is None else dx
    if x2 is not None and dx2 is None:
        dx2 = torch.empty_like(x2)
    L.check(L.lib().mrisr_op_groupnorm_bwd(_dt(x), _p(x), c0, _p(x2), c1, B, HW, _p(gamma), _p(beta), groups, eps, 1 if silu else 0, _p(dy),
                                           _p(dx), 1 if acc else 0, _p(dx2), 1 if acc2 else 0, _p(g_gamma), _p(g_beta), L.stream_ptr()))
    return dx, dx2


def layernorm_backward(x, dy, gamma, eps=1e-5, dx=None, acc=False, g_gamma=None, g_beta=None, need_dx=True):
    """rows x, dy [M,C] -> dx (added into a given ``dx`` with ``acc``); g_gamma / g_beta f32 [C] are added into.  ``need_dx`` False: the
    affine gradients alone (rows wider than the dx kernel takes, up to 1536 channels)."""
    M, Cc = x.shape
    dx = (torch.empty_like(x) if dx is None else dx) if need_dx else None
    L.check(L.lib().mrisr_op_layernorm_bwd(_dt(x), _p(x), _p(dy), _p(dx), _p(gamma), M, Cc, eps, 1 if acc else 0, _p(g_gamma), _p(g_beta),
                                           L.stream_ptr()))
    return dx


def geglu(pre, dout=None):
    """pre [M, 2*half] in the projection's 16-wide interleave.  Without ``dout``: u * gelu(g) [M, half]; with it: d pre [M, 2*half]."""
    M, two = pre.shape
    half = two // 2
    out = torch.empty((M, half) if dout is None else (M, two), dtype=pre.dtype, device=pre.device)
    L.check(L.lib().mrisr_op_geglu(_dt(pre), 0 if dout is None else 1, _p(pre), _p(dout), _p(out), M, half, L.stream_ptr()))
    return out


PW_SILU_BWD, PW_RELU_BWD, PW_SUMPOOL2, PW_MSE_GRAD, PW_ROWVEC_GRAD, PW_COLSUM = range(6)


def pointwise_backward(kind, a, b=None, out=None, out_f32=None, n=0, B=0, H=0, W=0, Cc=0, flag=0, ld_out=0, off=0):
    """mrisr_op_pointwise_bwd as declared in include/mrisr.h (kind = one of the PW_* constants)."""
    L.check(L.lib().mrisr_op_pointwise_bwd(kind, _dt(a), _p(a), _p(b), _p(out), _p(out_f32), n, B, H, W, Cc, flag, ld_out, off, L.stream_ptr()))


def lora_wgrad(P, Q, M, Cc, mode, r, nmod, secN, outs, scale=1.0, ldp=None, ldq=None):
    """P [M, ldp] (T), Q [M, ldq] f32; ``outs``: up to three f32 tensors (None: no adapter on that module), added into."""
    outs = list(outs) + [None] * (3 - len(outs))
    L.check(L.lib().mrisr_op_lora_wgrad(_dt(P), _p(P), P.shape[1] if ldp is None else ldp, _p(Q), Q.shape[1] if ldq is None else ldq, M, Cc,
                                        mode, r, nmod, secN, _p(outs[0]), _p(outs[1]), _p(outs[2]), scale, L.stream_ptr()))


def lora_wgrad_hr(P, Q, M, Cc, mode, r, nmod, secN, outs, scale=1.0, ldp=None, ldq=None, geglu_half=0):
    """``lora_wgrad`` at rank 32 .. 128 (multiples of 16): P [M, ldp] (T), Q [M, ldq] of the same type with module j's ``r`` columns at
    ``j * rp``, ``rp`` = ``r`` rounded up to 64 (bf16) / 32 (f32); ``outs`` as there.  ``geglu_half``: dB of ``ff.net.0.proj`` (P's columns
    in the 16-wide interleave, ``outs[0]`` [2*half, r] in raw row order)."""
    outs = list(outs) + [None] * (3 - len(outs))
    L.check(L.lib().mrisr_op_lora_wgrad_hr(_dt(P), _p(P), P.shape[1] if ldp is None else ldp, _p(Q), Q.shape[1] if ldq is None else ldq, M, Cc,
                                           mode, r, nmod, secN, _p(outs[0]), _p(outs[1]), _p(outs[2]), scale, geglu_half, L.stream_ptr()))


def dora_scale(W, A, B, mag, scale, dtype, ld=None, geglu_half=0, merged=False):
    """``mrisr_op_dora_scale``: W [n, k], A [r, k], B [n, r], mag [n] f32 (raw row order) -> (g f32 [n], rows [n, ld] of ``dtype``), both in
    the row order of the packed weight (``geglu_half``: the 16-wide interleave, ``geglu_packed_rows``).  Row ``dst(j)`` holds ``g W[j]`` or,
    ``merged``, ``g (W + scale B A)[j]`` in its first k columns; the columns beyond k keep what ``rows`` was filled with (NaN)."""
    n, k = W.shape
    ld = k if ld is None else ld
    g = torch.full((n,), float("nan"), dtype=torch.float32, device=W.device)
    rows = torch.full((n, ld), float("nan"), dtype=dtype, device=W.device)
    L.check(L.lib().mrisr_op_dora_scale(L.dtype_id(dtype), _p(W), _p(A), _p(B), _p(mag), scale, _p(g), _p(rows), ld, n, k, A.shape[0], geglu_half,
                                        1 if merged else 0, L.stream_ptr()))
    return g, rows


def dora_mag_grad(P, Y, mag, gm, M, Cc, R=None, bias=None, ldp=None, ldy=None, ldr=None, geglu_half=0):
    """``mrisr_op_dora_mag_grad``: adds ``(sum_m P (Y - R) - bias sum_m P) / mag`` into ``gm`` (f32 [C]).  P, Y, R: [M, ld*] of one dtype."""
    L.check(L.lib().mrisr_op_dora_mag_grad(_dt(P), _p(P), P.shape[1] if ldp is None else ldp, _p(Y), Y.shape[1] if ldy is None else ldy, _p(R),
                                           0 if R is None else (R.shape[1] if ldr is None else ldr), _p(bias), _p(mag), _p(gm), M, Cc, geglu_half,
                                           L.stream_ptr()))
    return gm


def geglu_packed_rows(half: int) -> torch.Tensor:
    """Packed row of every raw row of ``ff.net.0.proj`` ([2*half] rows: value half, then gate half): raw row ``g * half + j`` is stored at
    ``(j >> 4) * 32 + (j & 15) + 16 g`` - (value, gate) interleaved in blocks of 16.  ``packed[perm] = raw`` packs, ``packed[perm]`` unpacks."""
    if half <= 0 or half % 16:
        raise ValueError("half must be a positive multiple of 16")
    j = torch.arange(half, dtype=torch.int64)
    p = (j >> 4) * 32 + (j & 15)
    return torch.cat([p, p + 16])


def lora_wgrad_geglu(dpre, z, out, scale=1.0, M=None, ldp=None, ldq=None, r=None):
    """dB of an adapter on ``ff.net.0.proj``: dpre [M, 2*half] (T) in the 16-wide (value, gate) interleave, z [M, r] f32; ``out`` f32
    [2*half, r] in lora_B's raw row order (value rows, then gate rows) is added into."""
    L.check(L.lib().mrisr_op_lora_wgrad_geglu(_dt(dpre), _p(dpre), dpre.shape[1] if ldp is None else ldp, _p(z), z.shape[1] if ldq is None else ldq,
                                              dpre.shape[0] if M is None else M, out.shape[0] // 2, out.shape[1] if r is None else r, _p(out),
                                              scale, L.stream_ptr()))


def transpose(src, dst, R, Cc, ld_src, ld_dst, bs_src=0, bs_dst=0, batch=1, r_valid=None):
    L.check(L.lib().mrisr_op_transpose(_dt(src), _p(src), _p(dst), R, Cc, ld_src, ld_dst, bs_src, bs_dst, batch, R if r_valid is None else r_valid,
                                       L.stream_ptr()))


def softmax_backward(p, dp, nk, scale):
    """p [rows, ld] (T), dp [rows, ld] f32 -> dS [rows, ld] (T)."""
    rows, ld = p.shape
    ds = torch.empty_like(p)
    L.check(L.lib().mrisr_op_softmax_bwd(_dt(p), _p(p), _p(dp), _p(ds), ld, rows, nk, scale, L.stream_ptr()))
    return ds


def small_wgrad(dY, X, N, K, gW, gB=None, silu_in=False, rows=None):
    """gW [N,K] += dY^T act(X), gB [N] += colsum(dY): f32 rows dY [rows, ldy], X [rows, ldx]."""
    L.check(L.lib().mrisr_op_small_dense_bwd(L.MRISR_F32, 0, _p(dY), dY.shape[1], _p(X), X.shape[1], dY.shape[0] if rows is None else rows, N, K,
                                             1 if silu_in else 0, None, 0, _p(gW), _p(gB), 0, L.stream_ptr()))


def small_dgrad(dY, Wt, N, K, pre=None, rows=None):
    """dX [rows,K] = (dY W) * silu'(pre): dY f32 [rows, ldy], W [N,K] f32 or bf16, pre f32 [rows, ldpre] or None."""
    rows = dY.shape[0] if rows is None else rows
    dX = torch.empty((max(rows, 1), K), dtype=torch.float32, device=dY.device)
    L.check(L.lib().mrisr_op_small_dense_bwd(_dt(Wt), 1, _p(dY), dY.shape[1], _p(Wt), 0, rows, N, K, 0, _p(pre), 0 if pre is None else pre.shape[1],
                                             _p(dX), None, K, L.stream_ptr()))
    return dX


def conv_wgrad(x, dY, gW, gB=None, ks=3, stride=1, col0=0, cout_src=None, cout=None, cin=None, geglu_half=0):
    """x NHWC [B,H,W,cin_src] (a linear: [1,M,1,K]), dY rows [M, ldy]; gW f32 [cout,cin,ks,ks] and gB f32 [cout] are added into."""
    B, H, W, cin_src = x.shape
    cout_src = dY.shape[1] - col0 if cout_src is None else cout_src
    L.check(L.lib().mrisr_op_conv_wgrad(_dt(x), _p(x), B, H, W, cin_src, _p(dY), dY.shape[1], col0, cout_src, ks, stride, _p(gW), _p(gB),
                                        gW.shape[0] if cout is None else cout, gW.shape[1] if cin is None else cin, geglu_half, L.stream_ptr()))


def conv_dgrad(dy, weight, stride=1, dx=None, acc=False):
    """dy NHWC [B,H,W,cout], weight f32 [cout,cin,3,3] -> dx NHWC [B,H*stride,W*stride,cin] (added into a given ``dx`` with ``acc``)."""
    B, H, W, cout = dy.shape
    cin = weight.shape[1]
    mode = stride - 1
    if dx is None:
        dx = torch.empty((B, H << max(mode, 0), W << max(mode, 0), cin), dtype=dy.dtype, device=dy.device)
    L.check(L.lib().mrisr_op_conv_dgrad(_dt(dy), _p(dy), B, H, W, cout, _p(weight), cin, mode, _p(dx), 1 if acc else 0, L.stream_ptr()))
    return dx


def conv_lora_down(x, A, route=0):
    """x NHWC [B,H,W,cin] (f32 / bf16), A = lora_A [r,cin,3,3] -> z [B*H*W, r] f32 = conv3x3(x, A) (stride 1, pad 1).  ``route``: 0 planned,
    else 100 * (waves per pixel group: 1 or 4) + K slabs."""
    B, H, W, cin = x.shape
    a = A.detach().to(torch.float32).contiguous()
    z = torch.empty((B * H * W, a.shape[0]), dtype=torch.float32, device=x.device)
    L.check(L.lib().mrisr_op_conv_lora_down(_dt(x), _p(x), B, H, W, cin, _p(a), a.shape[0], _p(z), route, L.stream_ptr()))
    return z


def conv_lora_dgrad(dz, A, B, H, W, dtype=torch.float32, dx=None, acc=False):
    """dz [B*H*W, r] f32, A = lora_A [r,cin,3,3] -> dx NHWC [B,H,W,cin]: the transposed conv of dz (added into a given ``dx`` with ``acc``)."""
    a = A.detach().to(torch.float32).contiguous()
    r, cin = a.shape[0], a.shape[1]
    if dx is None:
        dx = torch.empty((B, H, W, cin), dtype=dtype, device=dz.device)
    L.check(L.lib().mrisr_op_conv_lora_dgrad(_dt(dx), _p(dz), B, H, W, r, _p(a), cin, _p(dx), 1 if acc else 0, L.stream_ptr()))
    return dx


def conv3x3_lora(x, weight, bias, A, Bm, scale, rowvec=None, resid=None, splitk=0, tile=0):
    """conv3x3(x, weight) + bias + rowvec[b, :, None, None] + scale * lora_B(lora_A(x)) + resid on NCHW x (f32 / bf16): the conv with the
    adapter's rank-r term in its epilogue.  A [r,cin,3,3], Bm [cout,r,1,1], rowvec [B,cout] f32.  A = Bm = None: no adapter."""
    xb, tx = _nhwc(x)
    tr = None
    if resid is not None:
        rb, tr = _nhwc(resid)
    f = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    w, b, a, bm, rv = f(weight), f(bias), f(A), f(Bm), f(rowvec)
    Bn, _, H, W = x.shape
    cout = w.shape[0]
    yb = torch.empty((Bn, H, W, cout), dtype=x.dtype, device=x.device)
    ty = L.as_tensor(yb, L.MRISR_NHWC, shape=(Bn, cout, H, W))
    L.check(L.lib().mrisr_op_conv3x3_lora(C.byref(tx), _p(w), _p(b), _p(a), _p(bm), a.shape[0] if a is not None else 0, float(scale), _p(rv),
                                          C.byref(tr) if tr is not None else None, cout, splitk, tile, C.byref(ty), L.stream_ptr()))
    return yb.permute(0, 3, 1, 2)
