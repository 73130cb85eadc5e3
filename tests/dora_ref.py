"""Reference for DoRA adapters (peft ``use_dora=True``) on the linear targets, shared by test_dora_cpu.py (which
checks THIS file on the CPU) and test_gpu_dora.py (which checks the device model against it).  In the style of lora_ff_ref.py, and with no
new oracle code: an adapter enters the oracle as the float64 weight it stands for,

    wn    = || W + s B A ||_2 per output row, DETACHED (peft treats it as a constant; no epsilon)
    W_eff = (m / wn)[:, None] * (W + s B A)        (y = b + g o (x W^T + s (x A^T) B^T) = b + x W_eff^T: the same function)

with ``A`` / ``B`` / ``m`` float64 leaf tensors; autograd through ``oracle.unet.unet_forward`` + MSE then gives all three gradients.
``m`` and ``lora_B`` of ``ff.net.0.proj`` are in PyTorch's row order: value half first, then gate half."""
import torch

import lora_ff_ref as lref

MAG = ".lora_magnitude_vector.default.weight"


def row_norm(w, a, b, scale, dtype=torch.float64):
    """|| W + s B A || per output row, from the tensors of one module (W may be a [c, c, 1, 1] conv weight)"""
    w2 = w.to(dtype).reshape(w.shape[0], -1)
    return torch.linalg.vector_norm(w2 + scale * (b.to(dtype).reshape(w.shape[0], -1) @ a.to(dtype).reshape(a.shape[0], -1)), dim=1)


def init_magnitudes(params, lora, scale, perturb=0.0, seed=0):
    """f32 magnitudes under their in-memory keys: the row norms (peft's initialisation), times ``1 + perturb * u`` with u uniform in
    [-1, 1] so that the scale m / wn differs from 1."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for ka, a in lora.items():
        if ".lora_A." not in ka:
            continue
        m = ka[: ka.index(".lora_A.")]
        wn = row_norm(params[m + ".weight"], a, lora[m + ".lora_B.default.weight"], scale)
        u = torch.rand(wn.shape, generator=g, dtype=torch.float64) * 2 - 1
        out[m + MAG] = (wn * (1 + perturb * u)).to(torch.float32)
    return out


def merged(params, dora, scale, dtype=torch.float64):
    """The oracle's parameter dict with every DoRA adapter of ``dora`` (lora_A, lora_B and magnitude keys) folded into its module's weight;
    differentiable in all three, the row norm detached."""
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
    for ka, a in dora.items():
        if ".lora_A." not in ka:
            continue
        m = ka[: ka.index(".lora_A.")]
        b, mag = dora[m + ".lora_B.default.weight"], dora[m + MAG]
        w = p[m + ".weight"]
        v = w.reshape(w.shape[0], -1) + scale * (b.to(dtype) @ a.to(dtype))
        wn = torch.linalg.vector_norm(v, dim=1).detach()
        p[m + ".weight"] = ((mag.to(dtype) / wn)[:, None] * v).reshape(w.shape)
    return p


leaves = lref.leaves


def forward(cfg, params, dora, scale, x, t, ctx, dtype=torch.float64):
    from oracle import unet as ou
    return ou.unet_forward(merged(params, dora, scale, dtype), cfg, x.to(dtype), t, ctx.to(dtype))


def loss_and_grads(cfg, params, dora, scale, x, t, ctx, target):
    """(pred, loss, {key: d loss / d tensor}) in float64, for lora_A, lora_B and the magnitudes."""
    lp = leaves(dora)
    with torch.enable_grad():
        pred = forward(cfg, params, lp, scale, x, t, ctx)
        loss = torch.nn.functional.mse_loss(pred, target.double())
        loss.backward()
    return pred.detach(), float(loss.detach()), {k: v.grad for k, v in lp.items()}


def closed_form_grads(x, w, bias, a, b, mag, scale, dy):
    """The gradients of the contract for one linear, from dY alone (float64 in, float64 out): (dX, dA, dB, dm).
    Wg = diag(g) W, sBg = diag(g) (s B), z = x A^T, y_lin = x Wg^T + z sBg^T"""
    wn = torch.linalg.vector_norm(w + scale * (b @ a), dim=1)
    g = mag / wn
    wg, sbg = g[:, None] * w, g[:, None] * (scale * b)
    z = x @ a.t()
    y_lin = x @ wg.t() + z @ sbg.t()
    dz = dy @ sbg
    d_a = dz.t() @ x
    d_x = dy @ wg + dz @ a
    d_b = g[:, None] * (scale * (dy.t() @ z))
    d_m = (dy * y_lin).sum(0) / mag
    return d_x, d_a, d_b, d_m


def peft_forward(x, w, bias, a, b, mag, scale):
    """peft's DoRA linear, literally: base output + the LoRA branch, the pair scaled by m / ||W + s B A|| (detached), bias outside"""
    wn = torch.linalg.vector_norm(w + scale * (b @ a), dim=1).detach()
    y = (mag / wn) * (x @ w.t() + scale * ((x @ a.t()) @ b.t()))
    return y if bias is None else y + bias
