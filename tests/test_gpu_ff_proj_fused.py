"""GPU: a transformer block's ``ff.net.2`` and the transformer's ``proj_out`` run as ONE GEMM over the concatenated K axis [4C | C]
(sources: the GEGLU output h and the residual stream t; weight [Wp W2 | Wp] composed at finalize in f32 and rounded once; bias
Wp b2 + bp; residual x) against the float64 reference and against the two launches it replaces.

Op level (`ops.ff_proj`, bf16).  The reference is the two-step formula o = (h W2^T + b2 + t) Wp^T + bp + x in float64 on the f32 master
weights (the model the bf16 engine approximates: each form then carries its own weight roundings - W2 and Wp for the two launches, Wp W2
rounded once and Wp for the composed one) and the bf16 activations as given.  The bound is the one tests/test_gpu_ops.py applies to
bf16 linears (1.2e-2 relative L2).  "Not worse than the two launches": the error figures are root-mean-squares over n = M C roughly
independent rounding errors, so two evaluations of the same arithmetic in a different summation order (another tile, another split)
differ by about 1 / sqrt(2 n) of the figure - 1.1 % at the smallest case (M = C = 64); the margin is 5 %, a little over four of those.
Model level (TINY config, all 16 transformer blocks at C = 64 / 128 / 256 qualify): the bounds of tests/test_gpu_unet.py.

Measured on an MI355X (relative L2 against the reference; composed un-split, composed with forced split 2 / 4, the two launches):
M = 64, C = 64: 2.62e-3, 2.11e-3, 3.38e-3; M = 192, C = 64: 2.58e-3, 2.09e-3, 3.31e-3; M = 64, C = 128: 2.04e-3, 2.04e-3, 3.03e-3;
M = 192, C = 128: 2.06e-3, 2.06e-3, 3.04e-3.  TINY forward against the oracle: composed 1.13e-2, two launches 1.15e-2."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lora_ff_ref as lref  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_BF16 = 1.2e-2          # tests/test_gpu_ops.py TOL["bf16"]
TOL_UNET_BF16 = 5e-2       # tests/test_gpu_unet.py, bf16 engine against oracle.unet
NOISE = 1.05               # see the module docstring
LDS_POISON = 2048
SPLITS = (0, 2, 4)
SHAPES = [(64, 64), (192, 64), (64, 128), (192, 128)]   # (M, C): one M tile / ragged multi-tile M; one / two K tiles of t


def rel64(a, ref):
    a = a.double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def _rnd(shape, seed, scale=1.0, dt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


_CASES = {}


def case(M, Cw):
    """Operands, the float64 reference and the two-launch result of one shape: built once, shared, never modified.  h W2^T and t are
    both of unit variance, so both K sources weigh the same in the sum."""
    if (M, Cw) in _CASES:
        return _CASES[(M, Cw)]
    from mrisr import ops
    bf = torch.bfloat16
    h, t, x = _rnd((M, 4 * Cw), 701, dt=bf), _rnd((M, Cw), 702, dt=bf), _rnd((M, Cw), 703, dt=bf)
    w2, b2 = _rnd((Cw, 4 * Cw), 704, (4 * Cw) ** -0.5), _rnd((Cw,), 705, 0.5)
    wp, bp = _rnd((Cw, Cw), 706, Cw ** -0.5), _rnd((Cw,), 707, 0.5)
    mid = h.double() @ w2.double().T + b2.double() + t.double()
    ref = mid @ wp.double().T + bp.double() + x.double()
    dev = dict(h=h.cuda(), t=t.cuda(), x=x.cuda(), w2=w2.cuda(), b2=b2.cuda(), wp=wp.cuda(), bp=bp.cuda())
    two = ops.ff_proj(**dev, fused=False)
    e_two = rel64(two, ref)
    assert e_two < TOL_BF16, e_two
    _CASES[(M, Cw)] = (dev, ref, e_two)
    return _CASES[(M, Cw)]


def _boundary_kinds(Cw, splitk):
    """Where gemm_bl_kernel's split rule (64-wide K tiles, ceil(nkt / splitk) per split) cuts the composed K axis [4C | C]."""
    nh, nkt = 4 * Cw // 64, 5 * Cw // 64
    if splitk < 2:
        return set()
    per = -(-nkt // splitk)
    return {"inside h" if k < nh else ("h | t" if k == nh else "inside t") for k in range(per, nkt, per)}


def test_split_boundaries_cover_every_kind():
    """The arithmetic behind the split cases below, asserted so that a change of the split rule or of the shapes cannot silently drop one:
    C = 64 (K tiles 4 | 1): split 2 cuts inside h, split 4 inside h and exactly between h and t; C = 128 (8 | 2): split 4 cuts at K tiles
    3, 6 and 9 - the last one inside t."""
    assert _boundary_kinds(64, 2) == {"inside h"}
    assert _boundary_kinds(64, 4) == {"inside h", "h | t"}
    assert "inside t" in _boundary_kinds(128, 4) and "inside h" in _boundary_kinds(128, 2)
    union = set().union(*(_boundary_kinds(c, s) for _, c in SHAPES for s in SPLITS))
    assert union == {"inside h", "h | t", "inside t"}


@pytest.mark.parametrize("M,Cw", SHAPES)
def test_composed_launch_against_float64_and_the_two_launches(M, Cw):
    from mrisr import _lib as L
    from mrisr import ops
    dev, ref, e_two = case(M, Cw)
    lib = L.lib()
    try:
        for split in SPLITS:
            lib.mrisr_debug_force_split(C.c_int(split))
            y = ops.ff_proj(**dev).clone()
            e = rel64(y, ref)
            print(f"M={M} C={Cw} force_split={split} {sorted(_boundary_kinds(Cw, split))}: composed {e:.3e}  two launches {e_two:.3e}")
            assert e < TOL_BF16, (split, e)
            assert e <= NOISE * e_two, (split, e, e_two)
            assert torch.equal(y, ops.ff_proj(**dev)), "not repeatable"
            try:
                lib.mrisr_debug_gemm_flags(C.c_int(LDS_POISON))
                yp = ops.ff_proj(**dev)
            finally:
                lib.mrisr_debug_gemm_flags(C.c_int(0))
            assert torch.isfinite(yp.float()).all() and torch.equal(y, yp), "LDS poison changed the result: a read ran ahead of its DMA"
    finally:
        lib.mrisr_debug_force_split(C.c_int(0))


# =================================================================================================
# model level (TINY)
# =================================================================================================
N_BLOCKS_TINY = 16   # 2 + 2 + 2 down, mid, 3 + 3 + 3 up: channels 64 / 128 / 256, none takes the C = 320 feed-forward kernel


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


def test_unet_bf16_composed_and_two_launch_forms(tiny):
    import mrisr
    from mrisr import _lib as L
    cfg, up, x, t, ctx, ref = tiny
    lib = L.lib()
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
    net.load_state_dict(up)
    fwd = lambda: net(x, t, encoder_hidden_states=ctx).sample.float().clone()
    try:
        lib.mrisr_debug_ff_proj_fused(C.c_int(1))
        on, c_on = profiled(lib, fwd)
        lib.mrisr_debug_ff_proj_fused(C.c_int(0))
        off, c_off = profiled(lib, fwd)
    finally:
        lib.mrisr_debug_ff_proj_fused(C.c_int(-1))
    e_on, e_off, e_between = rel(on, ref), rel(off, ref), rel(on, off)
    print(f"bf16 vs oracle: composed {e_on:.3e}, two launches {e_off:.3e}, between them {e_between:.3e}")
    print(f"launches: composed {sum(c_on.values())}, two launches {sum(c_off.values())}")
    assert e_on < TOL_UNET_BF16 and e_off < TOL_UNET_BF16 and e_between < TOL_UNET_BF16
    # every stand-alone proj_out GEMM is gone (and whatever reduce launch followed one)
    assert sum(c_off.values()) - sum(c_on.values()) >= N_BLOCKS_TINY, (c_on, c_off)
    assert torch.equal(on, profiled(lib, fwd)[0])   # the default is the composed form


def test_reloaded_weights_reach_the_composed_bank(tiny):
    import mrisr
    cfg, up, x, t, ctx, _ = tiny
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
    net.load_state_dict(up)
    fwd = lambda n: n(x, t, encoder_hidden_states=ctx).sample.float().clone()
    before = fwd(net)
    changed = dict(up)
    keys = [k for k in up if ".ff.net.2." in k or ".proj_out." in k]
    assert len(keys) == 4 * N_BLOCKS_TINY
    g = torch.Generator().manual_seed(77)
    for k in keys:
        changed[k] = up[k] + 0.5 * up[k].abs().mean() * torch.randn(up[k].shape, generator=g)
    net.load_state_dict(changed)   # on the live model: finalize runs again and must rebuild every bank
    after = fwd(net)
    fresh = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
    fresh.load_state_dict(changed)
    assert torch.equal(after, fwd(fresh))
    assert rel(after, before) > 1e-2


def test_merged_adapter_on_ff2_is_composed_from_the_merged_weight(tiny):
    """lora_fused = False folds the adapters into the packed weights at load; the bank must be built from W2 + s B A, not from W2."""
    import mrisr
    from mrisr import _lib as L
    from oracle import unet as ou
    cfg, up, x, t, ctx, _ = tiny
    lib = L.lib()
    mods = lref.block_modules(up, [lref.FF2, "proj_out"])
    lora = lref.init_adapters(up, mods, 4, seed=131)
    for k in lora:   # adapters strong enough to show (B as large as the weight's own entries)
        if ".lora_B." in k:
            lora[k] = lora[k] * 10
    scale = 2.0
    ref = ou.unet_forward(lref.merged(up, lora, scale, torch.float32), cfg, x.cpu(), t.cpu(), ctx.cpu())
    plain = ou.unet_forward(up, cfg, x.cpu(), t.cpu(), ctx.cpu())
    assert rel(plain, ref) > 2 * TOL_UNET_BF16   # (the adapters matter: a bank without them cannot pass)
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4 * scale, lora_fused=False)
    net.load_state_dict({**up, **lora})
    fwd = lambda: net(x, t, encoder_hidden_states=ctx).sample.float().clone()
    try:
        lib.mrisr_debug_ff_proj_fused(C.c_int(1))
        on, c_on = profiled(lib, fwd)
        lib.mrisr_debug_ff_proj_fused(C.c_int(0))
        off, c_off = profiled(lib, fwd)
    finally:
        lib.mrisr_debug_ff_proj_fused(C.c_int(-1))
    print(f"merged adapters, bf16 vs oracle: composed {rel(on, ref):.3e}, two launches {rel(off, ref):.3e}")
    assert rel(on, ref) < TOL_UNET_BF16 and rel(off, ref) < TOL_UNET_BF16
    assert sum(c_off.values()) - sum(c_on.values()) >= N_BLOCKS_TINY


def test_f32_engine_training_step_and_unmerged_adapters_keep_their_launches_and_bits(tiny):
    """None of the three takes the composed launch: the same launches by profiler class and the same bits with the switch on and off.
    Of the training step the bits compared are those of its forward (the prediction).  Its loss and gradients are accumulated with
    float atomics across workgroups (csrc/bwd.hip), so two steps of ONE build already differ in the last bits; for them the difference
    between the two settings must be f32 summation-order noise (below 1e-5 relative; a changed forward would move them at the bf16
    level, 1e-3 and more), and the difference between two steps of one setting is printed next to it."""
    import mrisr
    from mrisr import _lib as L
    from oracle import unet as ou
    cfg, up, x, t, ctx, ref = tiny
    lib = L.lib()
    lora = ou.init_lora_params(up, rank=4, seed=103)
    lora_ff2 = lref.init_adapters(up, lref.block_modules(up, [lref.FF2]), 4, seed=104)
    tgt = torch.randn(x.shape, generator=torch.Generator().manual_seed(9)).cuda()
    seen, grads = {}, {}
    try:
        for on in (1, 0):
            lib.mrisr_debug_ff_proj_fused(C.c_int(on))
            f32 = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32")
            f32.load_state_dict(up)
            o_f32, c_f32 = profiled(lib, lambda: f32(x, t, encoder_hidden_states=ctx).sample.float().clone())
            assert rel(o_f32, ref) < 1e-3
            net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4, lora_fused=True)
            net.load_state_dict({**up, **lora})
            tr = mrisr.LoRATrainer(net)

            def step():
                tr.zero_grad()
                loss, pred = tr.forward_backward(x, t, ctx, tgt, return_pred=True)
                return pred.float().cpu().clone(), (float(loss), tr.grad.detach().float().cpu().reshape(-1).clone())
            (o_tr, g_tr), c_tr = profiled(lib, step)
            grads.setdefault(on, []).extend([g_tr, step()[1]])
            ada = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4, lora_fused=True)
            ada.load_state_dict({**up, **lora_ff2})
            o_ada, c_ada = profiled(lib, lambda: ada(x, t, encoder_hidden_states=ctx).sample.float().clone())
            assert rel(o_ada, ref) < TOL_UNET_BF16 * 2   # (sanity only: the adapters move the output a little)
            seen[on] = ((o_f32, c_f32), (o_tr, c_tr), (o_ada, c_ada))
    finally:
        lib.mrisr_debug_ff_proj_fused(C.c_int(-1))
    for what, (a, ca), (b, cb) in zip(("f32 engine", "training step", "un-merged ff.net.2 adapter"), seen[1], seen[0]):
        assert ca == cb, (what, ca, cb)
        assert torch.equal(a, b), what
    # the step's loss and gradients: float atomics, bits not repeatable (see the docstring) - f32 summation-order noise only
    same = rel(grads[1][0][1], grads[1][1][1])
    across = max(rel(a[1], b[1]) for a in grads[1] for b in grads[0])
    d_loss = max(abs(a[0] - b[0]) / abs(b[0]) for a in grads[1] for b in grads[0])
    print(f"training step: flat gradient, two steps of one setting {same:.3e}, switch on against off {across:.3e}; loss on against off {d_loss:.3e}")
    assert across < 1e-5 and d_loss < 1e-5, (across, d_loss)


def test_three_ddim_steps_graph_equals_eager(tiny):
    import mrisr
    from mrisr import _lib as L
    cfg, up, x, t, ctx, _ = tiny
    lib = L.lib()
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
    net.load_state_dict(up)
    sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(3)

    def run(graph):
        lat = x.clone().contiguous()
        mrisr.Sampler(net, sp, kind="ddim").run(lat, ctx, use_graph=graph)
        torch.cuda.synchronize()
        return lat.cpu()
    try:
        lib.mrisr_debug_ff_proj_fused(C.c_int(1))
        g, e = run(True), run(False)
    finally:
        lib.mrisr_debug_ff_proj_fused(C.c_int(-1))
    assert torch.isfinite(g).all() and torch.equal(g, e)
