"""Reference for LoRA on the 3x3 convs of every ResnetBlock2D (peft ``lora.Conv2d``, dropout 0), shared by test_lora_conv_cpu.py (which
checks THIS file on the CPU against peft's two-conv definition) and test_gpu_lora_conv.py (which checks the device kernels and the
trainer against it).  No new oracle code: an adapter enters as the weight it stands for,

    W_eff = W + s * (B.reshape(cout, r) @ A.reshape(r, 9 cin)).reshape(W.shape)

(y = conv(x, W) + b + s * lora_B(lora_A(x)) = conv(x, W_eff) + b: the same function), with ``A`` [r, cin, 3, 3] and ``B`` [cout, r, 1, 1]
float64 leaf tensors; autograd through ``oracle.unet.unet_forward`` + MSE then gives d(loss)/dA and d(loss)/dB.  Adapters on linears go
through tests/lora_ff_ref.py's fold, which this file's ``merged`` includes (a 2-D adapter pair folds as W + s B A)."""
import torch

CONVS = ("conv1", "conv2")


def resnet_modules(params, which=CONVS):
    """``<resnet>.conv1`` / ``.conv2`` module names in the library's flat-vector order: the resnets of the down blocks, the mid block's two,
    the up blocks'; conv1 before conv2.  ``which``: the suffixes to keep, or a callable on the module name."""
    res = [k[: -len(".conv1.weight")] for k in params if k.endswith(".conv1.weight") and ".resnets." in k]
    order = {"down_blocks": 0, "mid_block": 1, "up_blocks": 2}
    res.sort(key=lambda b: (order[b.split(".")[0]], [int(t) for t in b.split(".") if t.isdigit()]))
    mods = [r + "." + c for r in res for c in CONVS]
    if callable(which):
        return [m for m in mods if which(m)]
    return [m for m in mods if m.endswith(tuple(which))]


def init_adapters(params, modules, rank=4, seed=0):
    """peft keys, f32: ``lora_A`` [r, cin, 3, 3] uniform 1/sqrt(9 cin), ``lora_B`` [cout, r, 1, 1] N(0, 0.02^2) - non-zero, so the branch
    is live."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for m in modules:
        w = params[m + ".weight"]
        cout, cin = int(w.shape[0]), int(w.shape[1])
        out[m + ".lora_A.default.weight"] = (torch.rand((rank, cin, 3, 3), generator=g) * 2 - 1) / (9 * cin) ** 0.5
        out[m + ".lora_B.default.weight"] = 0.02 * torch.randn((cout, rank, 1, 1), generator=g)
    return out


def fold(w, a, b, scale):
    """W_eff of one module (conv: 4-D a / b; linear: 2-D), differentiable in a and b."""
    r = a.shape[0]
    return w + scale * (b.reshape(b.shape[0], r) @ a.reshape(r, -1)).reshape(w.shape)


def two_conv(x, w, bias, a, b, scale):
    """peft's definition itself: the base conv plus the scaled 1x1 conv of the 3x3 conv."""
    F = torch.nn.functional
    return F.conv2d(x, w, bias, padding=1) + scale * F.conv2d(F.conv2d(x, a, padding=1), b)


def merged(params, lora, scale, dtype=torch.float64):
    """The oracle's parameter dict with every adapter of ``lora`` folded into its module's weight (differentiable in ``lora``)."""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
    for ka, a in lora.items():
        if ".lora_A." not in ka:
            continue
        m = ka[: ka.index(".lora_A.")]
        p[m + ".weight"] = fold(p[m + ".weight"], a.to(dtype), lora[m + ".lora_B.default.weight"].to(dtype), scale)
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
