"""GPU: a resnet's 1x1 conv_shortcut run as the last K steps of its conv2 (one launch on the concatenated filter bank
[cout][9 cout | cin], summed bias, no residual) against the float64 reference and against the two launches it replaces.

Op level (`ops.conv3x3_sc`, bf16): the bound is the one tests/test_gpu_ops.py applies to conv3x3 in bf16 (1.2e-2 relative L2 against
the reference on the bf16-rounded operands); the fused form keeps the shortcut in the f32 accumulator, so it must be no further from
the reference than shortcut GEMM -> conv + residual.  Model level (TINY config): the bounds of tests/test_gpu_unet.py."""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_BF16 = 1.2e-2          # tests/test_gpu_ops.py TOL["bf16"]
TOL_UNET_BF16 = 5e-2       # tests/test_gpu_unet.py, bf16 engine against oracle.unet
HALO_TILES = (41, 42, 43, 44, 45)
TILED_TILES = (14, 15, 16, 17, 18, 25, 26, 27, 28, 29, 30, 31)   # gemm_bl_kernel, 2-stage form
SOURCES = ((64, 0), (128, 64), (64, 128))
LDS_POISON = 2048


def rel64(a, ref):
    a = a.double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def _rnd(shape, seed, scale=1.0, dt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


_CASES = {}


def case(B, H, cin, cout, s0, s1):
    """Operands, the float64 reference and the two-launch result of one configuration: built once, shared, never modified."""
    key = (B, H, cin, cout, s0, s1)
    if key in _CASES:
        return _CASES[key]
    from mrisr import ops
    bf = torch.bfloat16
    h = _rnd((B, cin, H, H), 901, dt=bf)
    xs = _rnd((B, s0, H, H), 902, dt=bf)
    xs2 = _rnd((B, s1, H, H), 903, dt=bf) if s1 else None
    w, b = _rnd((cout, cin, 3, 3), 904, (9 * cin) ** -0.5), _rnd((cout,), 905)
    ws, bs = _rnd((cout, s0 + s1), 906, (s0 + s1) ** -0.5), _rnd((cout,), 907)
    xcat = xs.double() if xs2 is None else torch.cat([xs.double(), xs2.double()], 1)
    ref = F.conv2d(h.double(), w.to(bf).double(), b.double(), padding=1) + \
        F.conv2d(xcat, ws.to(bf).double()[:, :, None, None], bs.double())
    dev = dict(x=h.cuda(), weight=w.cuda(), bias=b.cuda(), xs=xs.cuda(), weight_sc=ws.cuda(), bias_sc=bs.cuda(),
               xs2=xs2.cuda() if xs2 is not None else None)
    two = ops.conv3x3_sc(**dev, fused=False)
    e_two = rel64(two, ref)
    assert e_two < TOL_BF16, e_two
    _CASES[key] = (dev, ref, e_two)
    return _CASES[key]


def check(B, H, cin, cout, s0, s1, tile, splitk=0):
    """fused launch: bound, not worse than the two-launch form, same bits twice, same bits with poisoned LDS."""
    from mrisr import _lib as L
    from mrisr import ops
    dev, ref, e_two = case(B, H, cin, cout, s0, s1)
    y = ops.conv3x3_sc(**dev, tile=tile, splitk=splitk).clone()
    e = rel64(y, ref)
    print(f"B={B} H={H} cin={cin} cout={cout} sc=({s0},{s1}) tile={tile} splitk={splitk}: fused {e:.3e}  two launches {e_two:.3e}")
    assert e < TOL_BF16, (tile, splitk, e)
    assert e <= e_two, (tile, splitk, e, e_two)
    assert torch.equal(y, ops.conv3x3_sc(**dev, tile=tile, splitk=splitk)), "not repeatable"
    lib = L.lib()
    try:
        lib.mrisr_debug_gemm_flags(C.c_int(LDS_POISON))
        yp = ops.conv3x3_sc(**dev, tile=tile, splitk=splitk)
    finally:
        lib.mrisr_debug_gemm_flags(C.c_int(0))
    assert torch.isfinite(yp.float()).all() and torch.equal(y, yp), "LDS poison changed the result: a read ran ahead of its DMA"


# ---- halo path: B = 2 (an M tile must not reach the neighbouring image through the shortcut source), 16 x 16, every halo tile ----
@pytest.mark.parametrize("cout", [64, 192])   # a single ragged N tile; two N tiles, the second ragged against BN = 160
@pytest.mark.parametrize("s0,s1", SOURCES)
def test_halo_kernels_carry_the_shortcut_tail(cout, s0, s1):
    for tile in HALO_TILES:
        check(2, 16, cout, cout, s0, s1, tile)


@pytest.mark.parametrize("cout,splitk", [(192, 2), (192, 4), (64, 3)])
def test_halo_kernels_split_over_chunks_with_a_tail(cout, splitk):
    """The halo kernels split K over 64-channel chunks, the tail's chunks dealt out the same way: (192, 2) both kinds in every split,
    (192, 4) a split with nothing at all, (64, 3) splits that hold tail chunks only (one 3x3 chunk, three tail chunks)."""
    nch, nsc = cout // 64, 3
    per, per_sc = -(-nch // splitk), -(-nsc // splitk)
    kinds = set()
    for s in range(splitk):
        conv = max(0, min(nch, (s + 1) * per) - s * per)
        tail = max(0, min(nsc, (s + 1) * per_sc) - min(nsc, s * per_sc))
        kinds.add((conv > 0, tail > 0))
    want = {(192, 2): {(True, True)}, (192, 4): {(True, True), (False, False)}, (64, 3): {(True, True), (False, True)}}[(cout, splitk)]
    assert kinds == want, kinds
    for tile in HALO_TILES:
        check(2, 16, cout, cout, 128, 64, tile, splitk)


# ---- tiled conv path: 8 x 8 (B = 2, M = 128) and 4 x 4 (B = 5, M = 80: one full 64-row tile over four images + a ragged one) ----
@pytest.mark.parametrize("B,H", [(2, 8), (5, 4)])
@pytest.mark.parametrize("cout", [64, 192])
@pytest.mark.parametrize("s0,s1", SOURCES)
def test_tiled_kernels_carry_the_shortcut_tail(B, H, cout, s0, s1):
    for tile in TILED_TILES:
        check(B, H, cout, cout, s0, s1, tile)


def _boundary_kinds(cin, s0, s1, splitk):
    """Where gemm_bl_kernel's split rule (64-wide K tiles, ceil(nkt / splitk) per split) cuts the fused K axis [9 cin | s0 | s1]."""
    taps, a, b = 9 * cin // 64, s0 // 64, s1 // 64
    nkt = taps + a + b
    per = -(-nkt // splitk)
    kinds = set()
    for k in range(per, nkt, per):
        if k < taps:
            kinds.add("inside the taps")
        elif k == taps:
            kinds.add("taps | shortcut")
        elif k == taps + a and b:
            kinds.add("between the sources")
        else:
            kinds.add("inside the shortcut")
    return kinds


SPLITS = (1, 2, 3, 4, 7)


def test_split_boundaries_cover_every_kind():
    """The arithmetic behind the split cases below, asserted so that a change of the split rule cannot silently drop one.  cout = conv
    input = 64: nine tap tiles, then the tail.  Sources (128, 64): splits 2 / 3 cut inside the taps, 4 exactly between taps and
    shortcut, 7 inside the first source.  No split of this set can cut between the sources of (128, 64) (the cut would have to be K tile
    11 of 12); the same splits on sources (64, 128) put one there (split 7, K tile 10), so both orders run."""
    k = {s: _boundary_kinds(64, 128, 64, s) for s in SPLITS}
    assert k[1] == set() and "inside the taps" in k[2] and "inside the taps" in k[3]
    assert "taps | shortcut" in k[4] and "inside the shortcut" in k[7]
    assert "between the sources" in _boundary_kinds(64, 64, 128, 7)
    union = set().union(*k.values(), *(_boundary_kinds(64, 64, 128, s) for s in SPLITS))
    assert union == {"inside the taps", "taps | shortcut", "inside the shortcut", "between the sources"}


@pytest.mark.parametrize("B,H", [(2, 8), (5, 4)])
@pytest.mark.parametrize("s0,s1", [(128, 64), (64, 128)])
@pytest.mark.parametrize("splitk", SPLITS)
def test_tiled_kernels_split_k_with_a_tail(B, H, s0, s1, splitk):
    """Every split with the separate reduce kernel (a launch that carries a tail never takes the in-kernel finisher)."""
    for tile in (14, 17, 26):
        check(B, H, 64, 64, s0, s1, tile, splitk)


def test_kernels_without_the_tail_are_refused():
    """Counted rings, the eight-wave halo kernel and the f32 / small-kernel configurations do not know the tail: a forced one is
    not taken for a launch that has a tail (the planner picks an eligible kernel), the result stays right."""
    from mrisr import ops
    dev, ref, _ = case(2, 16, 64, 64, 128, 64)
    for tile in (1, 4, 33, 37, 46, 50, 60):
        assert rel64(ops.conv3x3_sc(**dev, tile=tile), ref) < TOL_BF16


# =================================================================================================
# model level (TINY)
# =================================================================================================
def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


@pytest.fixture(scope="module")
def tiny():
    from oracle import unet as ou
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=101, perturb_norm=True)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 4, 16, 16), generator=g)
    ctx = torch.randn((2, 77, cfg.cross_attention_dim), generator=g)
    t = torch.tensor([10, 990])
    ref = ou.unet_forward(up, cfg, x, t, ctx)
    return cfg, up, x.cuda(), t.cuda(), ctx.cuda(), ref


def profiled(lib, fn):
    """fn() once un-profiled (planning, tuning), then once under the launch profiler: (result, {class: launches})."""
    fn()
    lib.mrisr_prof_reset(); lib.mrisr_prof_enable(1)
    out = fn()
    torch.cuda.synchronize(); lib.mrisr_prof_enable(0)
    buf = C.create_string_buffer(1 << 20)
    n = lib.mrisr_prof_report(buf, len(buf))
    cls = {k: v["launches"] for k, v in json.loads(buf.value[:n].decode()).items()}
    lib.mrisr_prof_reset()
    return out, cls


N_SHORTCUTS_TINY = 14   # down level 1 / 2 first resnets + the twelve decoder resnets (skip concatenation)


def test_unet_bf16_fused_and_two_launch_forms(tiny):
    import mrisr
    from mrisr import _lib as L
    cfg, up, x, t, ctx, ref = tiny
    lib = L.lib()
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
    net.load_state_dict(up)
    fwd = lambda: net(x, t, encoder_hidden_states=ctx).sample.float().clone()
    try:
        lib.mrisr_debug_sc_fused(C.c_int(1))
        on, c_on = profiled(lib, fwd)
        lib.mrisr_debug_sc_fused(C.c_int(0))
        off, c_off = profiled(lib, fwd)
    finally:
        lib.mrisr_debug_sc_fused(C.c_int(-1))
    e_on, e_off, e_between = rel(on, ref), rel(off, ref), rel(on, off)
    print(f"bf16 vs oracle: fused {e_on:.3e}, two launches {e_off:.3e}, between them {e_between:.3e}")
    assert e_on < TOL_UNET_BF16 and e_off < TOL_UNET_BF16 and e_between < TOL_UNET_BF16
    # every shortcut GEMM is gone (and whatever reduce launch followed one)
    assert sum(c_off.values()) - sum(c_on.values()) >= N_SHORTCUTS_TINY, (c_on, c_off)
    assert torch.equal(on, profiled(lib, fwd)[0])   # the default is the fused form


@pytest.mark.parametrize("split", [2, 4])
def test_groupnorm_sums_the_slabs_of_a_conv2_with_a_tail_and_changes_no_bit(tiny, split):
    """The invariant of test_groupnorm_sums_the_split_k_slabs_itself_and_changes_no_bit with the shortcut in conv2's K loop: the
    resnets in front of a transformer (down level 1 / 2 first resnets and the decoder's: all with a shortcut) hand their slabs to the
    transformer's GroupNorm, summed bias, no residual - the same bits as fused slabs -> splitk_reduce -> GroupNorm."""
    import mrisr
    from mrisr import _lib as L
    cfg, up, x, t, ctx, ref = tiny
    lib = L.lib()
    try:
        lib.mrisr_debug_sc_fused(C.c_int(1))
        lib.mrisr_debug_force_split(C.c_int(split))
        net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
        net.load_state_dict(up)
        fwd = lambda: net(x, t, encoder_hidden_states=ctx).sample.float().clone()
        lib.mrisr_debug_gn_slabs(C.c_int(0))
        two, c0 = profiled(lib, fwd)
        lib.mrisr_debug_gn_slabs(C.c_int(1))
        one, c1 = profiled(lib, fwd)
        n_slab = c1.get("groupnorm_from_slabs", 0)
        # 22 resnets: at most 22 conv1 -> norm2 pairs; 16 resnets stand in front of a transformer norm, 5 of them without a shortcut
        # (down level 0 twice, the second of down levels 1 / 2, mid 0) - any count above 27 proves a conv2 with a tail among them
        print("groupnorm_from_slabs launches:", n_slab)
        assert "groupnorm_from_slabs" not in c0 and n_slab > 22 + 5, (n_slab, sorted(c1))
        assert c0["splitk_reduce"] - c1["splitk_reduce"] == n_slab
        assert torch.equal(one, two), float((one - two).abs().max())
        assert rel(one, ref) < TOL_UNET_BF16
        # the same launches without the tail: as many slab-summing GroupNorms, 14 more GEMMs (+ their reduces)
        lib.mrisr_debug_sc_fused(C.c_int(0))
        _, c2 = profiled(lib, fwd)
        assert c2.get("groupnorm_from_slabs", 0) == n_slab
        assert sum(c2.values()) - sum(c1.values()) >= N_SHORTCUTS_TINY
    finally:
        lib.mrisr_debug_force_split(C.c_int(0))
        lib.mrisr_debug_gn_slabs(C.c_int(-1))
        lib.mrisr_debug_sc_fused(C.c_int(-1))


def test_reloaded_shortcut_weights_reach_the_fused_bank(tiny):
    import mrisr
    cfg, up, x, t, ctx, _ = tiny
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
    net.load_state_dict(up)
    fwd = lambda n: n(x, t, encoder_hidden_states=ctx).sample.float().clone()
    before = fwd(net)
    changed = dict(up)
    keys = [k for k in up if ".conv_shortcut." in k]
    assert len(keys) == 2 * N_SHORTCUTS_TINY
    g = torch.Generator().manual_seed(77)
    for k in keys:
        changed[k] = up[k] + 0.5 * up[k].abs().mean() * torch.randn(up[k].shape, generator=g)
    net.load_state_dict(changed)   # on the live model: finalize runs again and must rebuild every bank
    after = fwd(net)
    fresh = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
    fresh.load_state_dict(changed)
    assert torch.equal(after, fwd(fresh))
    assert rel(after, before) > 1e-2


def test_f32_engine_and_training_step_keep_their_launch_sequences(tiny):
    import mrisr
    from mrisr import _lib as L
    from oracle import unet as ou
    cfg, up, x, t, ctx, ref = tiny
    lib = L.lib()
    lora = ou.init_lora_params(up, rank=4, seed=103)
    tgt = torch.randn(x.shape, generator=torch.Generator().manual_seed(9)).cuda()
    counts = {}
    try:
        for on in (1, 0):
            lib.mrisr_debug_sc_fused(C.c_int(on))
            f32 = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32")
            f32.load_state_dict(up)
            out, c_f32 = profiled(lib, lambda: f32(x, t, encoder_hidden_states=ctx).sample.float().clone())
            assert rel(out, ref) < 1e-3
            net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4, lora_fused=True)
            net.load_state_dict({**up, **lora})
            tr = mrisr.LoRATrainer(net)

            def step():
                tr.zero_grad()
                return tr.forward_backward(x, t, ctx, tgt)
            _, c_tr = profiled(lib, step)
            counts[on] = (c_f32, c_tr)
    finally:
        lib.mrisr_debug_sc_fused(C.c_int(-1))
    assert counts[1][0] == counts[0][0]
    assert counts[1][1] == counts[0][1]
