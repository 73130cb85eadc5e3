"""Reference for tiled sampling, shared by test_tiles_cpu.py (which checks THIS file on the CPU) and test_gpu_tiles.py (which checks
the device kernels and the tiled sampler against it).  Pure torch, float64 where it computes.  No new oracle code: the oracle's
sampler loops (and tests/multistep_ref.py) take the UNet and the ControlNet as callables, so tiling is two wrappers around
``oracle.unet.OracleUNet`` / ``OracleControlNet`` that take the loop's canvas call, run the wrapped network on the tile batch and
hand back the blended canvas prediction.

Contract (include/mrisr.h, "tiled sampling"), per axis with extent n, tile t, overlap o:

    t_eff = min(t, n);  one tile at 0 if n <= t;  else s = t - o, k = ceil((n - t) / s) + 1, origin_i = min(i s, n - t)
    window: uniform 1, or gaussian w[i] = exp(-((i - (t_eff - 1) / 2) / t_eff)^2 / (2 * 0.01))
    nw[tile][i] = w[i] / sum over the tiles covering origin + i of w[their local index]      float64, rounded once to f32
    row of the tile batch r = b * T + ty * k_x + tx;   blend: sum over covering (ty, tx), ty then tx ascending,
    of (nwy[ty][.] * nwx[tx][.]) * et[r]"""
import torch


def grid(n, t, o):
    """(origins, t_eff) of one axis."""
    assert n > 0 and t > 0 and 0 <= o < t
    if n <= t:
        return [0], n
    s = t - o
    k = -(-(n - t) // s) + 1
    return [min(i * s, n - t) for i in range(k)], t


def window(t_eff, kind):
    if kind == "uniform":
        return torch.ones(t_eff, dtype=torch.float64)
    assert kind == "gaussian"
    i = torch.arange(t_eff, dtype=torch.float64)
    return torch.exp(-(((i - (t_eff - 1) / 2.0) / t_eff) ** 2) / (2.0 * 0.01))


def norm_tables(n, t, o, kind):
    """(origins, nw float64 [k, t_eff]); ``.float()`` of it is the table the device reads."""
    origins, te = grid(n, t, o)
    w = window(te, kind)
    total = torch.zeros(n, dtype=torch.float64)
    for q in origins:
        total[q:q + te] += w
    return origins, torch.stack([w / total[q:q + te] for q in origins])


def gather(x, oy, ox, th, tw):
    """[B, C, H, W] -> [B * T, C, th, tw], sample-major, ty-major inside a sample: a copy."""
    return torch.stack([x[:, :, y:y + th, xx:xx + tw] for y in oy for xx in ox], dim=1).flatten(0, 1)


def blend(et, oy, ox, nwy, nwx, H, W):
    """[B * T, C, th, tw] -> [B, C, H, W] in float64, on the tables as given (pass the f32-rounded ones to mirror the device)."""
    T = len(oy) * len(ox)
    th, tw = et.shape[2], et.shape[3]
    e = et.double().unflatten(0, (et.shape[0] // T, T))
    out = torch.zeros((e.shape[0], et.shape[1], H, W), dtype=torch.float64)
    for iy, y in enumerate(oy):
        for ix, xx in enumerate(ox):
            w2 = (nwy[iy].float()[:, None] * nwx[ix].float()[None, :]).double()  # the device multiplies the two f32 weights in f32
            out[:, :, y:y + th, xx:xx + tw] += w2 * e[:, iy * len(ox) + ix]
    return out


class _Out:
    def __init__(self, sample):
        self.sample = sample


class _Tiling:
    def __init__(self, H, W, tile, overlap, window_kind="gaussian"):
        t_h, t_w = tile if isinstance(tile, (tuple, list)) else (tile, tile)
        o_h, o_w = overlap if isinstance(overlap, (tuple, list)) else (overlap, overlap)
        self.H, self.W = H, W
        self.oy, nwy = norm_tables(H, t_h, o_h, window_kind)
        self.ox, nwx = norm_tables(W, t_w, o_w, window_kind)
        self.nwy, self.nwx = nwy.float(), nwx.float()  # rounded once to f32, as the device table
        self.th, self.tw = min(t_h, H), min(t_w, W)
        self.T = len(self.oy) * len(self.ox)

    def tiles(self, x, scale_num=1, scale_den=1):
        """Crop a canvas-shaped tensor whose pixels are scale_num / scale_den latent pixels wide (condition image: 8 / 1; adapter
        feature i: 1 / 2^i)."""
        f = lambda v: v * scale_num // scale_den  # noqa: E731
        return gather(x, [f(y) for y in self.oy], [f(xx) for xx in self.ox], f(self.th), f(self.tw))

    def rows(self, ctx):
        return None if ctx is None else ctx.repeat_interleave(self.T, dim=0)


class TiledControlNet(_Tiling):
    """The ControlNet on the tile batch: returns (down, mid) of the TILE batch, which only ``TiledUNet`` understands; the loops hand
    them through untouched."""

    def __init__(self, controlnet, H, W, tile, overlap, window_kind="gaussian"):
        super().__init__(H, W, tile, overlap, window_kind)
        self.controlnet = controlnet

    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, return_dict=False):
        assert tuple(sample.shape[2:]) == (self.H, self.W)
        return self.controlnet(self.tiles(sample), timestep, encoder_hidden_states=self.rows(encoder_hidden_states),
                               controlnet_cond=self.tiles(controlnet_cond, 8), return_dict=False)


class TiledUNet(_Tiling):
    """``unet`` on the tile batch of the canvas call: per-tile context rows, adapter features cropped per tile (feature i at
    origin / 2^i, from its own size), ControlNet residuals as ``TiledControlNet`` made them; ``.sample`` is the blended canvas
    prediction in the sample's dtype.  ``last`` keeps (tile batch in, tile predictions) of the latest call."""

    def __init__(self, unet, H, W, tile, overlap, window_kind="gaussian"):
        super().__init__(H, W, tile, overlap, window_kind)
        self.unet = unet
        self.last = None

    def __call__(self, sample, timestep, encoder_hidden_states=None, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, down_intrablock_additional_residuals=None):
        assert tuple(sample.shape[2:]) == (self.H, self.W)
        kw = {}
        if down_intrablock_additional_residuals is not None:
            feats = []
            for f in down_intrablock_additional_residuals:
                r = self.H // f.shape[2]
                assert f.shape[2] * r == self.H and f.shape[3] * r == self.W and r & (r - 1) == 0
                feats.append(self.tiles(f, 1, r).clone())
            kw["down_intrablock_additional_residuals"] = feats
        xt = self.tiles(sample)
        et = self.unet(xt, timestep, encoder_hidden_states=self.rows(encoder_hidden_states),
                       down_block_additional_residuals=down_block_additional_residuals,
                       mid_block_additional_residual=mid_block_additional_residual, **kw).sample
        self.last = (xt, et)
        return _Out(blend(et, self.oy, self.ox, self.nwy, self.nwx, self.H, self.W).to(sample.dtype))

