"""CPU: tiled sampling's grid and window - the reference (tests/tiles_ref.py) on the cases worked out by hand, the library's
host routine ``mrisr_tile_tables`` (through ``mrisr.tile_tables``; no GPU call) against it, partition of unity of the f32 tables,
every refusal of ``mrisr.check_tiles``, and the reference wrappers' own properties."""
import os

import pytest
import torch

import tiles_ref as tr

GRID_CASES = [  # extent, tile, overlap, origins, t_eff
    (24, 16, 8, [0, 8], 16),
    (32, 16, 8, [0, 8, 16], 16),
    (40, 16, 0, [0, 16, 24], 16),
    (64, 32, 8, [0, 24, 32], 32),
    (48, 32, 16, [0, 16], 32),
    (16, 32, 0, [0], 16),
]
WINDOWS = ("uniform", "gaussian")


@pytest.fixture(scope="module")
def mrisr_mod():
    import mrisr
    if not os.path.exists(mrisr.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return mrisr


@pytest.mark.parametrize("n,t,o,origins,te", GRID_CASES)
def test_grid_rule_reference(n, t, o, origins, te):
    got, got_te = tr.grid(n, t, o)
    assert got == origins and got_te == te
    assert got[0] == 0 and got[-1] + te == n and all(b > a and b - a <= te for a, b in zip(got, got[1:]))


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n,t,o,origins,te", GRID_CASES)
def test_library_tables_equal_the_reference(mrisr_mod, n, t, o, origins, te, window):
    got_o, got_w = mrisr_mod.tile_tables(n, t, o, window)
    ref_o, ref_w = tr.norm_tables(n, t, o, window)
    assert got_o == origins == ref_o  # exact
    assert got_w.dtype == torch.float32 and tuple(got_w.shape) == (len(origins), te)
    err = float(((got_w.double() - ref_w) / ref_w).abs().max())
    print(f"tile tables n={n} t={t} o={o} {window}: worst relative error {err:.3e}, smallest weight {float(ref_w.min()):.3e}")
    assert err <= 1e-6  # both sides compute in float64; one rounding to f32 is 6e-8
    assert torch.equal(got_w, ref_w.float())


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n,t,o,origins,te", GRID_CASES)
def test_partition_of_unity_and_single_cover(mrisr_mod, n, t, o, origins, te, window):
    _, w = mrisr_mod.tile_tables(n, t, o, window)
    total = torch.zeros(n, dtype=torch.float64)
    cover = torch.zeros(n, dtype=torch.int64)
    for q, org in enumerate(origins):
        total[org:org + te] += w[q].double()
        cover[org:org + te] += 1
    assert int(cover.min()) >= 1
    dev = float((total - 1.0).abs().max())
    print(f"partition of unity n={n} t={t} o={o} {window}: max |sum - 1| = {dev:.3e}")
    assert dev <= 1e-6
    for q, org in enumerate(origins):  # a pixel one tile covers: exactly 1.0f
        single = cover[org:org + te] == 1
        assert bool((w[q][single] == 1.0).all())
    if window == "uniform" and o == 0 and n % t == 0:
        assert bool((w == 1.0).all())


def test_check_tiles(mrisr_mod):
    ct = mrisr_mod.check_tiles
    assert ct(16, 8, "gaussian", 8) == (16, 16, 8, 8, "gaussian")
    assert ct((16, 32), (0, 8), "uniform", 8) == (16, 32, 0, 8, "uniform")
    assert ct(4, 2, "gaussian", 2) == (4, 4, 2, 2, "gaussian")
    bad = [
        (dict(tile=4, overlap=0, window="gaussian", divisor=8), "tile"),            # below the divisor
        (dict(tile=12, overlap=0, window="gaussian", divisor=8), "tile"),           # not a multiple
        (dict(tile=(16, 20), overlap=0, window="gaussian", divisor=8), "tile"),
        (dict(tile=0, overlap=0, window="gaussian", divisor=8), "tile"),
        (dict(tile=16.0, overlap=0, window="gaussian", divisor=8), "tile"),
        (dict(tile=(16, 16, 16), overlap=0, window="gaussian", divisor=8), "tile"),
        (dict(tile=16, overlap=-8, window="gaussian", divisor=8), "overlap"),       # negative
        (dict(tile=16, overlap=16, window="gaussian", divisor=8), "overlap"),       # >= tile
        (dict(tile=16, overlap=24, window="gaussian", divisor=8), "overlap"),
        (dict(tile=16, overlap=4, window="gaussian", divisor=8), "overlap"),        # not a multiple
        (dict(tile=(32, 16), overlap=(8, 16), window="gaussian", divisor=8), "overlap"),
        (dict(tile=16, overlap=True, window="gaussian", divisor=8), "overlap"),
        (dict(tile=16, overlap=8, window="hann", divisor=8), "window"),
        (dict(tile=16, overlap=8, window=None, divisor=8), "window"),
        (dict(tile=16, overlap=8, window="gaussian", divisor=8, has_cache=True), "cache"),
    ]
    for kw, name in bad:
        with pytest.raises(ValueError, match=name):
            ct(**kw)
    with pytest.raises(ValueError, match="window"):
        mrisr_mod.tile_tables(32, 16, 8, "hann")
    for args in ((0, 16, 8), (32, 0, 0), (32, 16, 16), (32, 16, -1)):  # the C routine refuses what it cannot grid
        with pytest.raises(RuntimeError):
            mrisr_mod.tile_tables(*args, "gaussian")


@pytest.mark.parametrize("window", WINDOWS)
def test_reference_blend_of_gather_is_the_identity(window):
    g = torch.Generator().manual_seed(5101)
    for (H, W, t, o) in ((24, 32, 16, 8), (40, 40, 16, 0), (12, 8, 4, 2), (64, 64, 32, 8), (16, 16, 16, 0)):
        x = torch.randn((2, 3, H, W), generator=g)
        oy, nwy = tr.norm_tables(H, t, o, window)
        ox, nwx = tr.norm_tables(W, t, o, window)
        th, tw = min(t, H), min(t, W)
        xt = tr.gather(x, oy, ox, th, tw)
        assert tuple(xt.shape) == (2 * len(oy) * len(ox), 3, th, tw)
        T = len(oy) * len(ox)
        for iy, y in enumerate(oy):  # row b * T + ty * k_x + tx is sample b's tile (ty, tx)
            for ix, xx in enumerate(ox):
                assert torch.equal(xt[T + iy * len(ox) + ix], x[1, :, y:y + th, xx:xx + tw])
        back = tr.blend(xt, oy, ox, nwy.float(), nwx.float(), H, W)
        err = float((back - x.double()).abs().max() / x.abs().max())
        print(f"blend(gather(x)) {H}x{W} t={t} o={o} {window}: max error {err:.3e}")
        assert err <= 1e-6


def test_tiled_wrappers_pointwise_network_and_one_tile():
    """A network that acts per pixel commutes with tiling (partition of unity end to end); with one tile the wrapper IS the wrapped
    network, bit for bit, on the real oracle UNet."""
    from oracle import unet as ou

    class Pointwise:
        def __call__(self, sample, timestep, encoder_hidden_states=None, **kw):
            return type("O", (), {"sample": 2.0 * sample + encoder_hidden_states[:, 0, 0, None, None, None]})

    g = torch.Generator().manual_seed(5102)
    x = torch.randn((2, 4, 24, 32), generator=g)
    ctx = torch.randn((2, 5, 7), generator=g)
    w = tr.TiledUNet(Pointwise(), 24, 32, 16, 8)
    assert w.T == 6
    out = w(x, torch.tensor(3), encoder_hidden_states=ctx).sample
    ref = 2.0 * x + ctx[:, 0, 0, None, None, None]
    assert float((out - ref).abs().max() / ref.abs().max()) <= 1e-6
    assert tuple(w.last[0].shape) == (12, 4, 16, 16)

    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=5103, perturb_norm=True)
    net = ou.OracleUNet(p, cfg)
    x = torch.randn((2, 4, 8, 16), generator=g)
    ctx = torch.randn((2, 9, cfg.cross_attention_dim), generator=g)
    with torch.no_grad():
        plain = net(x, torch.tensor(401), encoder_hidden_states=ctx).sample
        for tile, overlap in ((16, 8), ((8, 16), 0), (32, 0)):
            one = tr.TiledUNet(net, 8, 16, tile, overlap)
            assert one.T == 1
            assert torch.equal(one(x, torch.tensor(401), encoder_hidden_states=ctx).sample, plain)
