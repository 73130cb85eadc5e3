"""GPU: the tiled (gemm_bl_kernel) and halo (gemm_halo_kernel) GEMMs run their plain staged epilogue - alpha * acc + bias [+ time row] into the
LDS tile, the residual added on the way out - on its own few lines; mrisr_debug_gemm_flags(64) sends it through the generic epilogue4 again,
as before.  It is the same loads and the same operations in the same order, so every case must give the SAME BITS with the flag clear and
set (torch.equal, no tolerance), plain and with the LDS poisoned before the first DMA (flag 2048: a read that ran ahead of its DMA would return NaN).  One case per kernel is also
held against a float64 reference of the bf16-rounded operands at the relative-L2 bound tests/test_gpu_ops.py uses for bf16 linears and convs.

Shapes are the smallest that reach every path the change touches: M = 272 on 64- and 128-row tiles (the last tile has 16 live rows),
N = 68 in rows of pitch 72 (a staged output needs a pitch that is a multiple of 8: the plain path's 8-byte stores into the LDS tile meet the
N % 8 == 4 tail of the copy-out pass), N = 160 / 192 (more than one column tile on the narrow tiles, a ragged one on 128 x 128), K = 128 / 192
(two / three K steps).  The plain path takes the folded time row and the per-image one; cases with an epilogue-side adapter term (z from
global memory), GEGLU or a separate split-K reduce take the generic epilogue either way and pin it.  test_cases_reach_the_staged_path checks
with the phase stamps that the N = 68 and the halo cases really leave through the staged copy-out pass."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL_BF16 = 1.2e-2  # tests/test_gpu_ops.py: TOL["bf16"]
GENERIC, POISON = 64, 2048  # mrisr_debug_gemm_flags: plain staged epilogue through epilogue4; poisoned LDS
T64x64, T64x160, T128x128, T128x160, T128x192 = 17, 26, 14, 25, 28  # csrc/gemm.hip: TILES
HALO128x160, HALO64x160 = 41, 43


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def _rnd(shape, seed, scale=1.0, dt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


def _both_orders(run):
    """run() -> output tensor.  The plain epilogue (flags 0) and the generic one (64: the kernels as they were), each plain and with poisoned
    LDS: all bit-equal.  Returns the new code's output."""
    from mrisr import _lib as L
    lib = L.lib()
    outs = {}
    try:
        for flags in (0, GENERIC):
            for poison in (0, POISON):
                lib.mrisr_debug_gemm_flags(flags | poison)
                outs[flags | poison] = run().clone()
    finally:
        lib.mrisr_debug_gemm_flags(0)
    assert torch.isfinite(outs[0].float()).all()
    for flags in (GENERIC,):
        assert torch.equal(outs[0], outs[flags]), f"flags 0 vs {flags}"
        assert torch.equal(outs[POISON], outs[flags | POISON]), f"flags 0 vs {flags}, poisoned LDS"
    assert torch.equal(outs[0], outs[POISON]), "poisoned LDS changed the result"
    return outs[0]


def _linear_case(M, N, K, bias, rv_rows, lora, resid):
    """Operands of one projection (CPU), seeded by the shape; resid: None, 'out' (its own tensor) or 'inplace' (the output aliases it)."""
    s = 1000 * M + 10 * N + K
    c = {"x": _rnd((M, K), s + 1, dt=torch.bfloat16), "w": _rnd((N, K), s + 2, K ** -0.5)}
    c["b"] = _rnd((N,), s + 3) if bias else None
    c["rv"] = _rnd((rv_rows, N), s + 4) if rv_rows else None
    c["A"] = _rnd((4, K), s + 5, K ** -0.5) if lora else None
    c["B"] = _rnd((N, 4), s + 6, 0.25) if lora else None
    c["r"] = _rnd((M, _pitch(N)), s + 7, dt=torch.bfloat16) if resid else None  # (columns N .. pitch - 1 are never read or written)
    return c


def _pitch(N):
    return (N + 7) // 8 * 8


def _linear_ref64(c, scale):
    q = lambda t: t.to(torch.bfloat16).double()
    y = c["x"].double() @ q(c["w"]).T
    if c["b"] is not None:
        y = y + c["b"].double()
    if c["rv"] is not None:
        y = y + c["rv"].double().repeat_interleave(y.shape[0] // c["rv"].shape[0], dim=0)
    if c["A"] is not None:
        y = y + scale * (c["x"].double() @ q(c["A"]).T) @ c["B"].double().T
    if c["r"] is not None:
        y = y + c["r"].double()[:, :y.shape[1]]
    return y


LINEAR_CASES = [
    # tile, M, N, K, bias, rowvec rows (0 none, 1 scalar timestep: folded into the preload, 2 per image: per-row loads), rank-4 LoRA, residual, float64 check
    (T64x64, 272, 64, 128, True, 1, True, "out", True),
    (T64x64, 272, 68, 192, True, 2, False, "inplace", False),
    (T64x64, 272, 160, 128, False, 0, False, "out", False),
    (T64x160, 272, 160, 128, False, 1, True, "inplace", False),
    (T64x160, 272, 68, 192, True, 0, False, "out", False),
    (T64x160, 272, 192, 192, True, 2, False, None, False),
    (T128x128, 272, 192, 192, True, 2, True, "out", False),
    (T128x128, 256, 160, 128, False, 0, False, "inplace", False),
    (T128x160, 272, 160, 192, True, 1, True, "inplace", False),
    (T128x160, 272, 192, 128, True, 0, False, "out", False),
    (T128x160, 272, 68, 128, False, 1, False, "inplace", False),
]


def _linear_run(d, N, resid, scale, tile, **kw):
    """one launch of the case; the output in rows of pitch _pitch(N), its first N columns returned"""
    from mrisr import ops

    def run():
        r = d["r"].clone() if d["r"] is not None else None  # (in place: a fresh copy of the residual every run)
        out = r if resid == "inplace" else torch.zeros((d["x"].shape[0], _pitch(N)), dtype=torch.bfloat16, device="cuda")
        y = ops.linear_resid(d["x"], d["w"], d["b"], rowvec=d["rv"], lora_a=d["A"], lora_b=d["B"], lora_scale=scale, resid=r, out=out, tile=tile, **kw)
        return y[:, :N]
    return run


@pytest.mark.parametrize("tile,M,N,K,bias,rv_rows,lora,resid,check64", LINEAR_CASES)
def test_linear_epilogue_orders_are_bit_equal(tile, M, N, K, bias, rv_rows, lora, resid, check64):
    from mrisr import ops
    c = _linear_case(M, N, K, bias, rv_rows, lora, resid)
    d = {k: (v.cuda() if v is not None else None) for k, v in c.items()}
    scale = 0.5

    run = _linear_run(d, N, resid, scale, tile)
    y = _both_orders(run)
    assert y.shape == (M, N)
    if check64:
        e = rel(y, _linear_ref64(c, scale))
        print(f"linear tile {tile} M={M} N={N} K={K}: rel-l2 vs float64 {e:.3e}")
        assert e < TOL_BF16, e


@pytest.mark.parametrize("tile,bias", [(T128x192, True), (T128x192, False), (T64x64, True), (T128x128, False)])
def test_geglu_epilogue_orders_are_bit_equal(tile, bias):
    """The GEGLU epilogue takes the preloaded (u, gate) bias pairs: 128 x 192 is the tile the projection runs on in the models; two narrower tiles."""
    from mrisr import _lib as L
    from mrisr import ops
    M, N, K = 272, 192, 128
    x, w = _rnd((M, K), 11, dt=torch.bfloat16).cuda(), _rnd((N, K), 12, K ** -0.5).cuda()
    b = _rnd((N,), 13).cuda() if bias else None
    y = _both_orders(lambda: ops.linear(x, w, b, act=L.ACT_GEGLU, tile=tile))
    assert y.shape == (M, N // 2)


def _conv_case(cout):
    B, C, H = 2, 64, 16
    return {"x": _rnd((B, C, H, H), 21 + cout, dt=torch.bfloat16), "w": _rnd((cout, C, 3, 3), 22 + cout, (9 * C) ** -0.5), "b": _rnd((cout,), 23 + cout),
            "A": _rnd((4, C, 3, 3), 24 + cout, (9 * C) ** -0.5), "B": _rnd((cout, 4, 1, 1), 25 + cout, 0.25), "rv": _rnd((B, cout), 26 + cout),
            "r": _rnd((B, cout, H, H), 27 + cout, dt=torch.bfloat16), "xs": _rnd((B, C, H, H), 28 + cout, dt=torch.bfloat16),
            "ws": _rnd((cout, C, 1, 1), 29 + cout, C ** -0.5), "bs": _rnd((cout,), 30 + cout)}


@pytest.mark.parametrize("tile", [HALO128x160, HALO64x160])
@pytest.mark.parametrize("cout", [64, 160])
def test_halo_conv_epilogue_orders_are_bit_equal(tile, cout):
    """16 x 16 images, 64 -> cout channels, with a residual.  Plain path: bias + the time row per image + an out-of-place residual (held to
    float64 at cout = 160), and bias + an in-place residual (the shortcut GEMM's output is the conv's residual and its output).  Generic
    epilogue under either flag: the same conv with a rank-4 adapter's term from global z."""
    from mrisr import ops
    c = _conv_case(cout)
    d = {k: v.cuda() for k, v in c.items()}
    scale = 0.5
    y = _both_orders(lambda: ops.conv3x3_lora(d["x"], d["w"], d["b"], None, None, 1.0, rowvec=d["rv"], resid=d["r"], tile=tile))
    ya = _both_orders(lambda: ops.conv3x3_lora(d["x"], d["w"], d["b"], d["A"], d["B"], scale, rowvec=d["rv"], resid=d["r"], tile=tile))
    if cout == 160:
        q = lambda t: t.to(torch.bfloat16).double()
        ref = F.conv2d(c["x"].double(), q(c["w"]), c["b"].double(), padding=1) + c["rv"].double()[:, :, None, None] + c["r"].double()
        e = rel(y, ref)
        ea = rel(ya, ref + scale * F.conv2d(F.conv2d(c["x"].double(), q(c["A"]), padding=1), c["B"].double()))
        print(f"halo tile {tile} 64 -> {cout}: rel-l2 vs float64 {e:.3e}, with the adapter {ea:.3e}")
        assert e < TOL_BF16 and ea < TOL_BF16, (e, ea)
    _both_orders(lambda: ops.conv3x3_sc(d["x"], d["w"], d["b"], d["xs"], d["ws"], d["bs"], tile=tile, fused=False))


def _staged_launches(tile, run):
    """run() under the phase stamps of `tile`: [(M, N, K, the launch left through the staged copy-out pass)] for its launches on that tile.
    Stamp 6 (first residual batch in registers) is written only inside copy_out_tile."""
    import ctypes as C
    from mrisr import _lib as L
    HDR, WGS, SLOTS = 8, 1024, 256  # include/mrisr_debug.h
    buf = torch.zeros((SLOTS, HDR + 8 * WGS), dtype=torch.int64, device="cuda")
    lib = L.lib()
    lib.mrisr_debug_gemm_stamps.argtypes = [C.c_void_p, C.c_int]
    try:
        lib.mrisr_debug_gemm_stamps(C.c_void_p(buf.data_ptr()), tile)
        run()
        torch.cuda.synchronize()
    finally:
        lib.mrisr_debug_gemm_stamps(C.c_void_p(0), 0)
    s = buf.cpu()
    return [(int(h[0]), int(h[1]), int(h[2]), bool(h[HDR + 6] != 0 and h[HDR + 7] != 0)) for h in s if int(h[7]) == 1]


def test_cases_reach_the_staged_path():
    """The N = 68 linears (rows of pitch 72) and the adapter-free halo conv leave through the LDS tile and copy_out_tile, i.e. the bit-equality
    above compares the plain epilogue with the generic one there, not one path with itself; rows of pitch 68 cannot be staged."""
    from mrisr import ops
    for tile, M, N, K, bias, rv_rows, lora, resid, _ in LINEAR_CASES:
        if N != 68:
            continue
        c = _linear_case(M, N, K, bias, rv_rows, lora, resid)
        d = {k: (v.cuda() if v is not None else None) for k, v in c.items()}
        got = _staged_launches(tile, _linear_run(d, N, resid, 0.5, tile))
        assert got == [(M, N, K, True)], (tile, got)
    x, w = _rnd((272, 128), 71, dt=torch.bfloat16).cuda(), _rnd((68, 128), 72, 128 ** -0.5).cuda()
    assert _staged_launches(T64x64, lambda: ops.linear_resid(x, w, tile=T64x64)) == [(272, 68, 128, False)]
    for tile in (HALO128x160, HALO64x160):
        d = {k: v.cuda() for k, v in _conv_case(160).items()}
        got = _staged_launches(tile, lambda: ops.conv3x3_lora(d["x"], d["w"], d["b"], None, None, 1.0, rowvec=d["rv"], resid=d["r"], tile=tile))
        assert got == [(512, 160, 576, True)], (tile, got)


def test_split_k_paths_are_bit_equal():
    """Split launches: the reduce kernel finishes them (generic epilogue), or, with the reduction inside the kernel, the last arriver runs the
    kernel's own epilogue - the plain one where the form allows."""
    from mrisr import _lib as L
    from mrisr import ops
    lib = L.lib()
    c = _linear_case(272, 160, 192, True, 1, False, "out")
    d = {k: (v.cuda() if v is not None else None) for k, v in c.items()}
    cv = {k: v.cuda() for k, v in _conv_case(160).items()}
    x2 = torch.cat([cv["x"], cv["xs"]], 1)  # 128 input channels: two 64-channel chunks, one per split
    w2 = torch.cat([cv["w"], cv["w"].flip(0)], 1)
    lin = lambda **kw: ops.linear_resid(d["x"], d["w"], d["b"], rowvec=d["rv"], resid=d["r"], **kw)
    try:
        lib.mrisr_debug_force_split(2)
        y_plan = _both_orders(lambda: lin())  # the planner's tile, split by the hook
        y_tile = _both_orders(lambda: lin(tile=T64x160, splitk=2))
        _both_orders(lambda: ops.conv3x3_sc(x2, w2, cv["b"], cv["xs"], cv["ws"], cv["bs"], tile=HALO128x160, splitk=2, fused=False))
        _both_orders(lambda: ops.conv3x3_lora(x2, w2, cv["b"], torch.cat([cv["A"], cv["A"]], 1), cv["B"], 0.5, resid=cv["r"], tile=HALO64x160, splitk=2))
        lib.mrisr_debug_sk_inkernel(1)
        y_in = _both_orders(lambda: lin(tile=T64x64, splitk=2))
    finally:
        lib.mrisr_debug_force_split(0)
        lib.mrisr_debug_sk_inkernel(-1)
    ref = _linear_ref64(c, 0.0)
    for y in (y_plan, y_tile, y_in):
        assert rel(y, ref) < TOL_BF16


def test_unet_forward_is_bit_equal_with_either_epilogue():
    """A whole bf16 denoiser forward (rank-4 LoRA; head-major Q / K / V sections, conv1 with its per-image time row, conv2 + residual, the planner's
    tiles): the same bits with the plain staged epilogue and with the generic one."""
    import mrisr
    from mrisr import _lib as L
    from oracle import unet as ou
    cfg = ou.TINY
    params = ou.init_unet_params(cfg, seed=7, perturb_norm=True)
    params.update(ou.init_lora_params(params, rank=4, seed=8))
    x, ctx, t = _rnd((2, 4, 16, 16), 41).cuda(), _rnd((2, 77, cfg.cross_attention_dim), 42).cuda(), torch.tensor(601).cuda()
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4)
    net.load_state_dict(params)
    lib = L.lib()
    outs = []
    try:
        for flags in (0, GENERIC):
            lib.mrisr_debug_gemm_flags(flags)
            outs.append(net(x, t, encoder_hidden_states=ctx).sample.clone())
    finally:
        lib.mrisr_debug_gemm_flags(0)
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("tile", [T64x64, T64x160, HALO128x160, HALO64x160])
def test_conv_dgrad_accumulates_with_one_rounding_on_staged_tiles(tile):
    """dX += conv_dgrad(dY) on an un-split staged tile: the residual joins the f32 value ahead of the one rounding (GemmArgs::resid_exact), so
    the result meets |got - ref| <= 2^-8 |ref| + floor whichever tile the tuner picks (the element-wise bound and floor of
    tests/test_gpu_bwd_ops.py for conv.dgrad).  Rounded to bf16 before the add, as inference tiles do, cancelling elements miss it by 7e-3."""
    from mrisr import _lib as L
    from mrisr import ops
    B, cin, cout, H = 2, 64, 64, 16
    dy, w = _rnd((B, H, H, cout), 1001, dt=torch.bfloat16), _rnd((cout, cin, 3, 3), 1002, (9 * cin) ** -0.5, dt=torch.bfloat16)
    prior = _rnd((B, H, H, cin), 1003, dt=torch.bfloat16)
    with torch.enable_grad():
        x = torch.zeros((B, cin, H, H), dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv2d(x, w.double(), padding=1), x, dy.double().permute(0, 3, 1, 2))
    ref = (g.permute(0, 2, 3, 1) + prior.double()).cuda()
    lib = L.lib()
    try:
        lib.mrisr_debug_force_tile(tile)
        got = ops.conv_dgrad(dy.cuda(), w.float().cuda(), stride=1, dx=prior.cuda().clone(), acc=1).double()
    finally:
        lib.mrisr_debug_force_tile(0)
    excess = float(((got - ref).abs() - 2.0 ** -8 * ref.abs()).max())
    print(f"conv_dgrad acc=1 tile {tile}: max(|d| - 2^-8 |ref|) = {excess:.3e}")
    assert excess <= 8 * 2.425e-06, excess
