"""Reference for LoRA on every linear of a transformer block, ``ff.net.0.proj`` included, shared by test_lora_ff_cpu.py (which checks
THIS file on the CPU) and test_gpu_lora_ff.py (which checks the device trainer against it).  No new oracle code: the oracle's
forward applies adapters to the attention projections only, so an adapter enters as the weight it stands for,

    W_eff = W + s B A          (y = x W^T + s (x A^T) B^T = x W_eff^T: the same function)

with ``A`` / ``B`` float64 leaf tensors; autograd through ``oracle.unet.unet_forward`` + MSE then gives d(loss)/dA and d(loss)/dB.
``lora_B`` of ``ff.net.0.proj`` is [8C, r] in PyTorch's row order: value half first, then gate half."""
import torch

# the nine adapted linears of a block (fused Q/K/V and K/V count once each), as peft module suffixes
ATTN = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0")
FF1, FF2 = "ff.net.0.proj", "ff.net.2"


def block_modules(params, which="all"):
    """Module names, per transformer block in the library's flat-vector order: proj_in, attn1 q/k/v, attn1 out, attn2 q, attn2 k/v,
    attn2 out, ff.net.0.proj, ff.net.2, proj_out.  ``which``: "all", "existing" (all but ``ff.net.0.proj``: what the trainer took
    before) or an iterable of module suffixes to keep."""
    blocks = [k[: -len(".proj_in.weight")] for k in params if k.endswith(".proj_in.weight")]
    # the library walks down blocks, mid block, up blocks
    order = {"down_blocks": 0, "mid_block": 1, "up_blocks": 2}
    blocks.sort(key=lambda b: (order[b.split(".")[0]], [int(t) for t in b.split(".") if t.isdigit()]))
    out = []
    for b in blocks:
        t = b + ".transformer_blocks.0."
        mods = [b + ".proj_in"] + [t + a for a in ATTN] + [t + FF1, t + FF2, b + ".proj_out"]
        if which == "all":
            keep = mods
        elif which == "existing":  # what the trainer accepted before ff.net.0.proj: everything else
            keep = [m for m in mods if not m.endswith(FF1)]
        else:
            keep = [m for m in mods if m.endswith(tuple(which))]
        out += keep
    return out


def init_adapters(params, modules, rank=4, seed=0):
    """peft keys, f32: ``lora_A`` [r, in] uniform like a Linear, ``lora_B`` [out, r] N(0, 0.02^2) - non-zero, so the branch is live."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for m in modules:
        w = params[m + ".weight"]
        n_out, n_in = int(w.shape[0]), int(w.shape[1])
        out[m + ".lora_A.default.weight"] = (torch.rand((rank, n_in), generator=g) * 2 - 1) / n_in ** 0.5
        out[m + ".lora_B.default.weight"] = 0.02 * torch.randn((n_out, rank), generator=g)
    return out


def merged(params, lora, scale, dtype=torch.float64):
    """The oracle's parameter dict with every adapter of ``lora`` folded into its module's weight (differentiable in ``lora``)."""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
    for ka, a in lora.items():
        if ".lora_A." not in ka:
            continue
        m = ka[: ka.index(".lora_A.")]
        b = lora[m + ".lora_B.default.weight"]
        w = p[m + ".weight"]
        p[m + ".weight"] = w + scale * (b.to(dtype) @ a.to(dtype)).reshape(w.shape)
    return p


def leaves(lora, dtype=torch.float64):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in lora.items()}


def forward(cfg, params, lora, scale, x, t, ctx, dtype=torch.float64):
    from oracle import unet as ou
    return ou.unet_forward(merged(params, lora, scale, dtype), cfg, x.to(dtype), t, ctx.to(dtype))


def loss_and_grads(cfg, params, lora, scale, x, t, ctx, target):
    """(pred, loss, {key: d loss / d tensor}) in float64."""
    lp = leaves(lora)
    with torch.enable_grad():
        pred = forward(cfg, params, lp, scale, x, t, ctx)
        loss = torch.nn.functional.mse_loss(pred, target.double())
        loss.backward()
    return pred.detach(), float(loss.detach()), {k: v.grad for k, v in lp.items()}
