"""Reference for the two row-local fused kernels of a C = 320 transformer block, shared by test_xtail_ref_cpu.py (which checks
THIS file on the CPU) and test_gpu_xtail_op.py (which checks the kernels against it).  Plain torch, nothing from ``mrisr``.

The operations are diffusers' ``BasicTransformerBlock`` between ``attn1`` and ``norm3`` ("middle": csrc/xtail.hip) and its
feed-forward followed by the transformer's ``proj_out`` and outer residual ("ff": the continuation of mlp_fused_kernel in
csrc/gemm.hip), as oracle/unet.py restates them.  Each comes as a pair:

  ``*_exact``     float64 on the operands the kernel is given (bf16 rows, weights rounded to bf16 as the packers round them, f32
                  vectors), no rounding in between;
  ``*_emulated``  the same chain in float64 with the kernel's rounding points inserted (listed at each function), exact
                  accumulation otherwise.  Its distance from ``*_exact`` is the yardstick a kernel's error is held against.

An operand set is a dict (see ``middle_random``); the recipes below build every set the GPU tests use, so that the CPU test can
show the yardstick is sane for each of them before a GPU sees it.  Everything runs on the device its operands live on."""
import math

import torch

C, HEADS, HD = 320, 8, 40
BF = torch.bfloat16


def bf(x):
    """Round to bf16 (through f32, as a kernel's f32 accumulator is rounded), back in float64."""
    return x.to(torch.float32).to(BF).to(torch.float64)


def _d(x):
    return None if x is None else x.to(torch.float64)


def _wq(w):
    """A weight as the packers hand it to the MFMA: f32 -> bf16."""
    return w.to(torch.float32).to(BF).to(torch.float64)


def _lin(x, w, b):
    y = x @ w.t()
    return y if b is None else y + _d(b)


def _adapter(op, i):
    """(A as bf16, scale * B as the f32 product the packer forms) of projection i, or None."""
    if not op.get("lora"):
        return None
    a, b = op["lora"][i]
    sb = (b.to(torch.float32) * torch.tensor(op["lora_scale"], dtype=torch.float32)).to(torch.float64)
    return _wq(a), sb


def _layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * _d(g) + _d(b)


def _heads(x, n):
    return x.reshape(-1, n, HEADS, HD).permute(0, 2, 1, 3)


def _attention(q, op, round_p):
    """softmax(q k^T / sqrt(40)) v per head over the first nk prompt rows; ``round_p``: P normalised, then rounded to bf16."""
    nk, ntok = op["nk"], op["ntok"]
    qh = _heads(q, ntok)
    kh, vh = _heads(_d(op["k"][:, :nk]), nk), _heads(_d(op["v"][:, :nk]), nk)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(HD)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    if round_p:
        p = bf(p)
    return (p @ vh).permute(0, 2, 1, 3).reshape(-1, C)


def _rows(op):
    return _d(op["ao"][:, :C]), _d(op["t"][:, :C])


def middle_exact(op):
    """x2 [M][320] in float64."""
    ao, x0 = _rows(op)

    def proj(x, w, b, i):
        y = _lin(x, _wq(op[w]), op[b])
        ad = _adapter(op, i)
        return y if ad is None else y + (x @ ad[0].t()) @ ad[1].t()

    x1 = proj(ao, "w1", "b1", 0) + x0
    q = proj(_layer_norm(x1, op["gamma"], op["beta"]), "wq", "bq", 1)
    o = _attention(q, op, False)
    return proj(o, "w2", "b2", 2) + x1


def middle_emulated(op):
    """The rounding points of xattn_tail_kernel (csrc/xtail.hip), in the order the kernel meets them:
    z = bf16(x A^T) and bf16(scale * B) at the adapter's MFMA K step (gemm_chunk: ``lbf[r] = (bf16)lb[i][r]``);
    x1 = bf16(bf16(acc) + x0): the projection's output is rounded, then the sum again; LayerNorm output to bf16; q to bf16;
    P normalised, then bf16; o to bf16; x2 = bf16(bf16(acc) + x1).  The LayerNorm statistics themselves are taken exactly (the
    kernel's are f32 with the variance shifted by the row's element 0: no rounding POINT, and what the LayerNorm cases probe)."""
    ao, x0 = _rows(op)

    def proj(x, w, b, i):
        y = _lin(x, _wq(op[w]), op[b])
        ad = _adapter(op, i)
        return bf(y if ad is None else y + bf(x @ ad[0].t()) @ bf(ad[1]).t())

    x1 = bf(proj(ao, "w1", "b1", 0) + x0)
    xn = bf(_layer_norm(x1, op["gamma"], op["beta"]))
    q = proj(xn, "wq", "bq", 1)
    o = bf(_attention(q, op, True))
    return bf(proj(o, "w2", "b2", 2) + x1)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _ff(op, r):
    x = _d(op["x"])
    xn = r(_layer_norm(x, op["gamma"], op["beta"]))
    u, g = _lin(xn, _wq(op["w1"]), op["b1"]).chunk(2, dim=-1)
    f = r(_lin(r(u * _gelu(g)), _wq(op["w2"]), op["b2"]))
    t2 = r(f + x) if op["residual"] else f
    return r(r(_lin(t2, _wq(op["wp"]), op["bp"])) + _d(op["xres"]))


def ff_exact(op):
    """([x +] FF2(GEGLU(FF1(LayerNorm(x))))) Wp^T + bp + xres in float64."""
    return _ff(op, lambda v: v)


def ff_emulated(op):
    """The rounding points of mlp_fused_kernel with its continuation (csrc/gemm.hip): bf16 LayerNorm output, bf16 hidden activation
    (the two test_fused_feed_forward_kernel already uses), then bf16 after FF2, after + x, after the projection and after + xres."""
    return _ff(op, bf)


def measures(y, exact):
    """(max |y - exact| / max |exact|, relative L2, the worst row's relative L2) of a result [M][320] against ``exact``."""
    y, e = y.to(torch.float64), exact.to(torch.float64)
    d = y - e
    rows = d.norm(dim=-1) / e.norm(dim=-1).clamp_min(1e-300)
    return float(d.abs().max() / e.abs().max()), float(d.norm() / e.norm()), float(rows.max())


# ------------------------------------------------------------------------------------------------------------------------------
# operand recipes
# ------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pad(x, ld, fill):
    out = torch.full((x.shape[0], ld), fill, dtype=x.dtype)
    out[:, : x.shape[1]] = x
    return out


PAD = 768.0   # sentinel of the padding columns (exact in bf16)


def middle_random(M=256, ntok=128, nk=77, lora=False, bias=True, seed=0, ldao=C, ldt=C, nkbuf=None):
    """N(0, 1) rows and prompt rows, N(0, 1 / 320) weights (so x1, q and the scores are O(1)), LayerNorm near the identity;
    adapters as large as the projections they sit on (A ~ N(0, 1 / 320), scale * B ~ 0.6 N(0, 1)), so that a fault in that branch
    is not hidden below the rounding noise.  ``ldao`` / ``ldt``: row pitches (the padding holds PAD); ``nkbuf``: rows of the k / v
    buffers (rows >= nk random as well)."""
    g = _gen(1000 + seed)
    n = lambda *s: torch.randn(s, generator=g)
    B = M // ntok
    w = lambda: n(C, C) / math.sqrt(C)
    b = lambda: (0.1 * n(C)) if bias else None
    op = {"ao": _pad(n(M, C).to(BF), ldao, PAD), "t": _pad(n(M, C).to(BF), ldt, PAD), "ntok": ntok, "nk": nk,
          "w1": w(), "b1": b(), "gamma": 1 + 0.1 * n(C), "beta": 0.1 * n(C), "wq": w(), "bq": b(), "w2": w(), "b2": b(),
          "k": n(B, nkbuf or nk, C).to(BF), "v": n(B, nkbuf or nk, C).to(BF), "lora": None, "lora_scale": 2.0}
    if lora:
        op["lora"] = [(n(4, C) / math.sqrt(C), 0.3 * n(C, 4)) for _ in range(3)]
    return op


def middle_one_hot(M=256, ntok=128, nk=77, seed=0):
    """Every head of every row attends to ONE key, a different one per head: keys of +-1 entries, head h of token i selects key
    perm_h[i mod nk].  attn1.to_out is zero, so x1 = x0 = the selected keys side by side; LayerNorm is the plain normalisation
    (rows of +-1: mean ~ 0, variance ~ 1) and Wq = 6 I, so q is 6 times the selected key up to the row's mean and deviation: its
    score is 6 sqrt(40) ~ 38 against N(0, 6) for the others.  W2 = I, b2 = 0 and V holds multiples of 1/4 in [-2, 2] (x1 + V exact
    in bf16): x2 - x1 is row perm_h[i] of V in head h's 40 columns, bit for bit.  Returns (operands, sel [B][8][ntok])."""
    g = _gen(2000 + seed)
    B = M // ntok
    k = torch.sign(torch.randn((B, nk, C), generator=g))
    v = torch.randint(-8, 9, (B, nk, C), generator=g).float() / 4
    sel = torch.stack([torch.stack([torch.randperm(nk, generator=g)[torch.arange(ntok) % nk] for _ in range(HEADS)]) for _ in range(B)])
    x0 = torch.empty((B, ntok, C))
    for h in range(HEADS):
        cs = slice(HD * h, HD * h + HD)
        x0[:, :, cs] = torch.gather(k[:, :, cs], 1, sel[:, h, :, None].expand(-1, -1, HD))
    eye = torch.eye(C)
    op = {"ao": torch.randn((M, C), generator=g).to(BF), "t": x0.reshape(M, C).to(BF), "ntok": ntok, "nk": nk,
          "w1": torch.zeros(C, C), "b1": None, "gamma": torch.ones(C), "beta": torch.zeros(C), "wq": 6 * eye, "bq": None,
          "w2": eye, "b2": None, "k": k.to(BF), "v": v.to(BF), "lora": None, "lora_scale": 1.0}
    return op, sel


def middle_uniform(nk, M=256, ntok=128, seed=0, big=1000.0):
    """Wq = 0, bq = 0: every score is 0, attention is the mean over the first nk rows of V; W2 = I, b2 = 0, so x2 - x1 is that mean
    to bf16 rounding.  The k / v buffers have 80 rows; rows >= nk hold +-``big``: only the masks of the pack and of the kernel
    keep them out."""
    op = middle_random(M, ntok, nk, seed=3000 + seed, nkbuf=80)
    op["wq"], op["bq"], op["w2"], op["b2"] = torch.zeros(C, C), None, torch.eye(C), None
    sg = torch.sign(torch.randn((M // ntok, 80 - nk, C), generator=_gen(3500 + seed)))
    for name in ("k", "v"):
        op[name][:, nk:] = (big * sg).to(BF)
    return op


def middle_softmax_range(kind, M=256, ntok=128, nk=77, seed=0):
    """Scores of magnitude 150 (q k / sqrt(40), before the kernel's factor log2 e).  Rows are +-p_b, one +-1 pattern per image
    (attn1.to_out zero, plain LayerNorm), Wq = (150 / sqrt(40)) I.  ``last``: the LAST key is p_b, the others random +-1: its
    score is +150 in the rows +p_b (the maximum, in the last key) and -150 in the rows -p_b (where the maximum is some other key);
    ``equal``: every key is p_b, all scores of a row are equal (+150 or -150)."""
    g = _gen(4000 + seed)
    B = M // ntok
    p = torch.sign(torch.randn((B, 1, C), generator=g))
    sgn = torch.sign(torch.randn((B, ntok, 1), generator=g))
    k = torch.sign(torch.randn((B, nk, C), generator=g))
    if kind == "last":
        k[:, nk - 1] = p[:, 0]
    else:
        k[:] = p
    op = middle_random(M, ntok, nk, seed=4500 + seed)
    op.update({"t": (sgn * p).reshape(M, C).to(BF), "w1": torch.zeros(C, C), "b1": None, "gamma": torch.ones(C), "beta": torch.zeros(C),
               "wq": (150.0 / math.sqrt(HD)) * torch.eye(C), "bq": None, "k": k.to(BF)})
    return op


def middle_layernorm(kind, M=256, ntok=128, nk=77, seed=0):
    """Rows that strain the statistics (the kernel's variance is E[(x - x[0])^2] - E[x - x[0]]^2 in f32), attn1.to_out zero so that
    x1 = x0 is exactly the row described: ``offset`` mean 30, deviation 0.5; ``spike`` element 0 is 100, the rest N(0, 0.05^2);
    ``constant`` every element of a row equal (variance 0: the output is beta); ``affine`` ordinary rows (attn1.to_out live) with
    gamma ~ 5 N(0, 1), beta ~ 3 N(0, 1)."""
    g = _gen(5000 + seed)
    op = middle_random(M, ntok, nk, seed=5500 + seed)
    if kind == "affine":
        op["gamma"], op["beta"] = 5 * torch.randn(C, generator=g), 3 * torch.randn(C, generator=g)
        return op
    if kind == "offset":
        x = 30 + 0.5 * torch.randn((M, C), generator=g)
    elif kind == "spike":
        x = 0.05 * torch.randn((M, C), generator=g)
        x[:, 0] = 100.0
    elif kind == "constant":
        x = (3 * torch.randn((M, 1), generator=g)).expand(M, C).clone()
    else:
        raise ValueError(kind)
    op.update({"t": x.to(BF), "w1": torch.zeros(C, C), "b1": None})
    return op


def ff_random(M=128, H=1280, bias=True, residual=True, seed=0):
    """The operands of test_fused_feed_forward_kernel (rows 0.7 N(0, 1) + 0.5, N(0, 1 / fan-in) weights) plus proj_out and xres;
    ``bias``: proj_out's (the feed-forward's own are always there)."""
    g = _gen(6000 + seed)
    n = lambda *s: torch.randn(s, generator=g)
    return {"x": (0.7 * n(M, C) + 0.5).to(BF), "gamma": 1 + 0.1 * n(C), "beta": 0.1 * n(C),
            "w1": n(2 * H, C) / math.sqrt(C), "b1": n(2 * H), "w2": n(C, H) / math.sqrt(H), "b2": n(C),
            "wp": n(C, C) / math.sqrt(C), "bp": n(C) if bias else None, "xres": n(M, C).to(BF), "residual": residual}


def to(op, device):
    """The operand set on ``device`` (tensors moved, adapters included)."""
    mv = lambda v: v.to(device) if torch.is_tensor(v) else v
    out = {k: mv(v) for k, v in op.items()}
    if out.get("lora"):
        out["lora"] = [None if p is None else (p[0].to(device), p[1].to(device)) for p in out["lora"]]
    return out
