"""The cases of tests/test_gpu_gemm_head.py and the script that records their output bits.

Every case is one launch (or one small op) on the tiled (gemm_bl_kernel) or halo (gemm_halo_kernel) GEMM with operands from a closed-form
integer pattern that is exact in bf16 - no random generator - and returns (output, float64 reference of the bf16-rounded operands).

    python tests/gemm_head_cases.py --record tests/golden/gemm_head/bits.json

runs every case on the library in the tree and writes the SHA-256 of each output's bytes.  The committed file was recorded this way from the
library of the commit BEFORE the launch head existed: the test holds the kernels to those bits from then on."""
import hashlib
import json
import os
import sys

import torch
import torch.nn.functional as F

T64x64, T64x160, T128x128, T128x160 = 17, 26, 14, 25  # csrc/gemm.hip: TILES
HALO128x160, HALO64x160 = 41, 43
POISON = 2048  # mrisr_debug_gemm_flags: LDS poisoned before the first DMA


def pat(shape, salt, scale=1.0, dt=torch.float32):
    """((7919 i + 104729 j + 613 salt) % 251 - 125) / 64 over the flattened (row, column) index: multiples of 1/64 below 2 in magnitude, exact in
    bf16 (seven significant bits); `scale` is a power of two."""
    n = 1
    for s in shape:
        n *= s
    cols = shape[-1]
    idx = torch.arange(n, dtype=torch.int64)
    i, j = idx // cols, idx % cols
    v = ((7919 * i + 104729 * j + 613 * salt) % 251 - 125).double() / 64.0 * scale
    out = v.reshape(shape).to(dt)
    assert torch.equal(out.double(), out.to(torch.bfloat16).double())
    return out


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _lib():
    from mrisr import _lib as L
    return L.lib()


def _group_m(gm):
    lib = _lib()
    if hasattr(lib, "mrisr_debug_group_m"):  # (the library the bits were recorded from has no such hook: the tile order changes no output bit)
        lib.mrisr_debug_group_m(gm)


# ---- tiled, plain ----
def linear_case(tile, M, N, K, lora=False, resid=True, splitk=0, group_m=0, sk_inkernel=None):
    def run():
        from mrisr import ops
        x, w = pat((M, K), 1, dt=torch.bfloat16), pat((N, K), 2, 1 / 8)
        b, rv = pat((N,), 3), pat((1, N), 4)
        A, Bm = (pat((4, K), 5, 1 / 8), pat((N, 4), 6, 1 / 4)) if lora else (None, None)
        pitch = (N + 7) // 8 * 8
        r = pat((M, pitch), 7, dt=torch.bfloat16) if resid else None
        ref = x.double() @ w.double().T + b.double() + rv.double()
        if lora:
            ref = ref + 0.5 * (x.double() @ A.double().T) @ Bm.double().T
        if resid:
            ref = ref + r.double()[:, :N]
        cu = lambda t: None if t is None else t.cuda()
        out = torch.zeros((M, pitch), dtype=torch.bfloat16, device="cuda")
        lib = _lib()
        try:
            _group_m(group_m)
            if sk_inkernel is not None:
                lib.mrisr_debug_sk_inkernel(sk_inkernel)
            y = ops.linear_resid(cu(x), cu(w), cu(b), rowvec=cu(rv), lora_a=cu(A), lora_b=cu(Bm), lora_scale=0.5, resid=cu(r), out=out, splitk=splitk, tile=tile)
            torch.cuda.synchronize()
        finally:
            _group_m(0)
            lib.mrisr_debug_sk_inkernel(-1)
        return y[:, :N].clone(), ref
    return run


def two_source_case(tile):
    """ff.net.2 + proj_out as one GEMM over K = [64 | 128]: the two plain row sources (c0 = 64, c1 = 128)"""
    def run():
        from mrisr import ops
        M, K4, C = 272, 64, 128
        h, t, x = pat((M, K4), 11, dt=torch.bfloat16), pat((M, C), 12, 1 / 4, dt=torch.bfloat16), pat((M, C), 13, dt=torch.bfloat16)
        w2, b2, wp, bp = pat((C, K4), 14, 1 / 8), pat((C,), 15), pat((C, C), 16, 1 / 16), pat((C,), 17)
        ref = (h.double() @ w2.double().T + b2.double() + t.double()) @ wp.double().T + bp.double() + x.double()
        y = ops.ff_proj(h.cuda(), t.cuda(), x.cuda(), w2.cuda(), b2.cuda(), wp.cuda(), bp.cuda(), tile=tile, fused=True)
        return y, ref
    return run


def attention_case():
    """the unfused bf16 attention: batched Q K^T and P V launches (blockIdx.z, non-zero a_bs / w_bs) on head-major operands"""
    def run():
        from mrisr import ops
        B, N, C, heads = 2, 64, 128, 2
        q, k, v = (pat((B, N, C), s, 1 / 4, dt=torch.bfloat16) for s in (21, 22, 23))
        hd = C // heads
        sp = lambda t: t.double().reshape(B, N, heads, hd).transpose(1, 2)
        ref = F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(B, N, C)
        return ops.attention(q.cuda(), k.cuda(), v.cuda(), heads, flash=False), ref
    return run


# ---- tiled and halo, conv: NCHW operands, B x C x H x W ----
def _conv_ops(B, C, H, W, cout, salt):
    return pat((B, C, H, W), salt, dt=torch.bfloat16), pat((cout, C, 3, 3), salt + 1, 1 / 32), pat((cout,), salt + 2)


def conv_case(tile, form, B=3, H=6, W=10, C=64, cout=64, splitk=0):
    def run():
        from mrisr import ops
        x, w, b = _conv_ops(B, C, H, W, cout, 31)
        kw = dict(tile=tile, splitk=splitk)
        if form == "stride1":
            return ops.conv3x3(x.cuda(), w.cuda(), b.cuda(), **kw), F.conv2d(x.double(), w.double(), b.double(), padding=1)
        if form == "stride2":
            return ops.conv3x3(x.cuda(), w.cuda(), b.cuda(), stride=2, **kw), F.conv2d(x.double(), w.double(), b.double(), padding=1, stride=2)
        if form == "stride2pad0":
            # Downsample2D(padding=0): zero pad (0, 1, 0, 1), then stride 2 - output (oy, ox) reads rows 2 oy .. 2 oy + 2, which is the window of
            # output (2 oy + 1, 2 ox + 1) of the stride-1 pad-1 conv: the same K order over the same values, so the same bits.  The library
            # the bits were recorded from has no op that reaches pad 0 (no hook): there the case IS that sub-sampled stride-1 launch, and the
            # digest holds the pad-0 launch of today's library to it
            ref = F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), w.double(), b.double(), stride=2, padding=0)
            lib = _lib()
            if not hasattr(lib, "mrisr_debug_op_conv_pad0"):
                return ops.conv3x3(x.cuda(), w.cuda(), b.cuda(), **kw)[:, :, 1::2, 1::2].contiguous(), ref
            try:
                lib.mrisr_debug_op_conv_pad0(1)
                y = ops.conv3x3(x.cuda(), w.cuda(), b.cuda(), stride=2, **kw).contiguous()
                torch.cuda.synchronize()
            finally:
                lib.mrisr_debug_op_conv_pad0(0)
            return y, ref
        if form in ("nearest", "subpix"):
            ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)
            return ops.conv3x3(x.cuda(), w.cuda(), b.cuda(), upsample=True, subpix=form == "subpix", **kw), ref
        if form == "two_sources":
            x2 = pat((B, C, H, W), 35, dt=torch.bfloat16)
            w2 = pat((cout, 2 * C, 3, 3), 36, 1 / 32)
            return ops.conv3x3(x.cuda(), w2.cuda(), b.cuda(), x2=x2.cuda(), **kw), F.conv2d(torch.cat([x, x2], 1).double(), w2.double(), b.double(), padding=1)
        if form in ("tail1", "tail2"):
            xs, ws, bs = pat((B, C, H, W), 37, dt=torch.bfloat16), pat((cout, C if form == "tail1" else 2 * C, 1, 1), 38, 1 / 8), pat((cout,), 39)
            xs2 = pat((B, C, H, W), 40, dt=torch.bfloat16) if form == "tail2" else None
            src = xs if xs2 is None else torch.cat([xs, xs2], 1)
            ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) + F.conv2d(src.double(), ws.double(), bs.double())
            y = ops.conv3x3_sc(x.cuda(), w.cuda(), b.cuda(), xs.cuda(), ws.cuda(), bs.cuda(), xs2=None if xs2 is None else xs2.cuda(), fused=True, **kw)
            return y, ref
        if form == "zstuff":  # the data gradient of a stride-2 conv: a stride-1 conv over the zero-stuffed x2 image
            dy, wz = pat((B, H, W, cout), 41, dt=torch.bfloat16), pat((cout, C, 3, 3), 42, 1 / 32, dt=torch.bfloat16)
            with torch.enable_grad():
                xi = torch.zeros((B, C, 2 * H, 2 * W), dtype=torch.float64, requires_grad=True)
                (g,) = torch.autograd.grad(F.conv2d(xi, wz.double(), padding=1, stride=2), xi, dy.double().permute(0, 3, 1, 2))
            lib = _lib()
            try:
                lib.mrisr_debug_force_tile(tile)
                y = ops.conv_dgrad(dy.cuda(), wz.float().cuda(), stride=2)
                torch.cuda.synchronize()
            finally:
                lib.mrisr_debug_force_tile(0)
            return y, g.permute(0, 2, 3, 1)
        raise ValueError(form)
    return run


def unet_case():
    def run():
        import mrisr
        from oracle import unet as ou
        cfg = ou.TINY
        params = ou.init_unet_params(cfg, seed=7, perturb_norm=True)
        params.update(ou.init_lora_params(params, rank=4, seed=8))
        x, ctx, t = pat((2, 4, 16, 16), 51), pat((2, 77, cfg.cross_attention_dim), 52, 1 / 2), torch.tensor(601)
        with torch.no_grad():
            ref = ou.unet_forward(params, cfg, x, t, ctx)
        lib = _lib()
        try:
            # one tile for every GEMM of the model: TINY's shapes are in no tile table, and the plan-time tuner's pick - by timing, per process -
            # decides the summation order and with it the bits
            lib.mrisr_debug_force_tile(T64x64)
            net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4)
            net.load_state_dict(params)
            y = net(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample.clone()
            torch.cuda.synchronize()
        finally:
            lib.mrisr_debug_force_tile(0)
        return y, ref
    return run


def cases():
    """name -> (run, relative-L2 bound against the float64 reference)"""
    c = {}
    for tile in (T64x64, T64x160, T128x128, T128x160):
        for N in (68, 160, 192):  # 68 in rows of pitch 72; on 64 x 64 N = 160 gives 15 workgroups: the `nblk & 7 = 7` remainder of the XCD remap
            for K in (128, 192):
                c[f"linear t{tile} M272 N{N} K{K}"] = linear_case(tile, 272, N, K)
        c[f"linear t{tile} M8 N160 K128"] = linear_case(tile, 8, 160, 128)  # one tile, 8 live rows
        c[f"linear t{tile} lora"] = linear_case(tile, 272, 160, 128, lora=True)
        c[f"linear t{tile} split2 reduce kernel"] = linear_case(tile, 272, 160, 192, splitk=2, sk_inkernel=0)  # three K tiles: shares of 2 and 1
        c[f"linear t{tile} split2 in kernel"] = linear_case(tile, 272, 160, 192, splitk=2, sk_inkernel=1)
        c[f"two sources t{tile}"] = two_source_case(tile)
        for form in ("stride1", "stride2", "stride2pad0", "nearest", "subpix", "zstuff", "tail1", "tail2", "two_sources"):
            c[f"conv t{tile} {form}"] = conv_case(tile, form)
    for tile in (T64x64, T64x160):  # five M tiles: groups of 1, 2 (short last group of 1), 3 (of 2) and 8 (larger than the grid)
        for gm in (1, 2, 3, 8):
            c[f"linear t{tile} group_m {gm}"] = linear_case(tile, 272, 160, 128, group_m=gm)
    # weights of 512 KiB and more: the launch pre-touches them (pretouch_weights_head runs, its pieces land in the second stage buffer)
    c["linear t26 pretouch N640 K448"] = linear_case(T64x160, 272, 640, 448)
    c["halo t41 pretouch C192"] = conv_case(HALO128x160, "stride1", B=2, H=16, W=16, C=192, cout=160)
    c["attention unfused bf16"] = attention_case()
    for tile, sizes in ((HALO128x160, (16, 32)), (HALO64x160, (8, 16, 32))):  # whole tiles per image: 128 rows need 16 x 16 and up
        for s in sizes:
            c[f"halo t{tile} {s}x{s}"] = conv_case(tile, "stride1", B=2, H=s, W=s, cout=160)
        c[f"halo t{tile} two sources"] = conv_case(tile, "two_sources", B=2, H=16, W=16, cout=160)
        c[f"halo t{tile} tail1"] = conv_case(tile, "tail1", B=2, H=16, W=16, cout=160)
        c[f"halo t{tile} tail2"] = conv_case(tile, "tail2", B=2, H=16, W=16, cout=160)
        c[f"halo t{tile} split2"] = conv_case(tile, "two_sources", B=2, H=16, W=16, cout=160, splitk=2)
    for tile in (HALO128x160, HALO64x160):
        inner = conv_case(tile, "stride1", B=2, H=16, W=16, cout=160)

        def run(inner=inner):
            try:
                _group_m(3)
                y, ref = inner()
                torch.cuda.synchronize()
            finally:
                _group_m(0)
            return y, ref
        c[f"halo t{tile} group_m 3"] = run
    c["unet tiny forward"] = unet_case()
    return c


def run_both(run):
    """the case plain and with the LDS poisoned before the first DMA -> (output, poisoned output, reference)"""
    lib = _lib()
    try:
        lib.mrisr_debug_gemm_flags(0)
        y, ref = run()
        lib.mrisr_debug_gemm_flags(POISON)
        yp, _ = run()
    finally:
        lib.mrisr_debug_gemm_flags(0)
    return y, yp, ref


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "mri-diffusion-superresolution_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.setdefault("MRISR_TUNE_CACHE", os.path.join(root, "profiles", "r03_tune_cache.tsv"))
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    bits = {}
    for name, run in cases().items():
        y, yp, ref = run_both(run)
        bits[name] = digest(y)
        print(f"{name}: rel-l2 vs float64 {rel(y, ref):.3e}  poisoned equal {torch.equal(y, yp)}  {bits[name][:16]}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    with open(sys.argv[2], "w") as f:
        json.dump(bits, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(bits)} cases -> {sys.argv[2]}")


if __name__ == "__main__":
    main()
