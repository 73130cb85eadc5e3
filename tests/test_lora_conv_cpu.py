"""CPU: the reference of tests/lora_conv_ref.py is peft's Conv2d LoRA, the state-dict template of the conv adapters, and the disk-key
round trip of their 4-D tensors."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lora_conv_ref as ref  # noqa: E402


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def test_folded_weight_is_the_two_conv_definition():
    """conv(x, W_eff) + b == conv(x, W) + b + s * lora_B(lora_A(x)) on float64, and so are the autograd gradients of A and B: 1e-12
    relative (float64 rounding of two association orders of sums of ~600 products)."""
    g = torch.Generator().manual_seed(5)
    for (B, H, W, cin, cout, r, s) in ((2, 5, 7, 6, 10, 4, 2.0), (1, 4, 4, 16, 8, 8, 0.5), (3, 3, 3, 8, 8, 16, 1.0)):
        x = torch.randn((B, cin, H, W), generator=g, dtype=torch.float64)
        w = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64) / (9 * cin) ** 0.5
        bias = torch.randn((cout,), generator=g, dtype=torch.float64)
        dy = torch.randn((B, cout, H, W), generator=g, dtype=torch.float64)
        a0 = torch.randn((r, cin, 3, 3), generator=g, dtype=torch.float64) / (9 * cin) ** 0.5
        b0 = torch.randn((cout, r, 1, 1), generator=g, dtype=torch.float64)
        grads = []
        outs = []
        for form in ("folded", "two_conv"):
            a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            with torch.enable_grad():
                if form == "folded":
                    y = torch.nn.functional.conv2d(x, ref.fold(w, a, b, s), bias, padding=1)
                else:
                    y = ref.two_conv(x, w, bias, a, b, s)
                (y * dy).sum().backward()
            outs.append(y.detach())
            grads.append((a.grad, b.grad))
        assert rel(outs[0], outs[1]) <= 1e-12
        assert rel(grads[0][0], grads[1][0]) <= 1e-12 and rel(grads[0][1], grads[1][1]) <= 1e-12
        assert float(grads[1][0].norm()) > 0 and float(grads[1][1].norm()) > 0
        assert rel(outs[1], torch.nn.functional.conv2d(x, w, bias, padding=1)) > 1e-3  # the adapter is not a no-op


def test_lora_conv_param_shapes():
    import mrisr
    from mrisr import params as P
    assert P.LORA_CONV_TARGETS == ("conv1", "conv2")
    for cfg, rank in ((mrisr.UNetConfig(), 4), (mrisr.UNetConfig(), 8)):
        base = {k: s for k, s, _ in P.unet_param_shapes(cfg)}
        convs = [k[: -len(".weight")] for k in base if ".resnets." in k and k.endswith((".conv1.weight", ".conv2.weight"))]
        got = list(P.lora_conv_param_shapes(cfg, rank))
        keys = [k for k, _, _ in got]
        assert len(convs) == 44 and len(keys) == len(set(keys)) == 2 * len(convs)
        shapes = {k: s for k, s, _ in got}
        total = 0
        for m in convs:
            cout, cin = base[m + ".weight"][:2]
            assert shapes[m + ".lora_A.default.weight"] == (rank, cin, 3, 3)
            assert shapes[m + ".lora_B.default.weight"] == (cout, rank, 1, 1)
            total += rank * 9 * cin + cout * rank
        assert sum(math.prod(s) for s in shapes.values()) == total
        # no other module is a target, and the attention template is what it was
        assert all(k.split(".lora_")[0] in convs for k in keys)
    assert sum(math.prod(s) for _, s, _ in P.lora_param_shapes(mrisr.UNetConfig(), 4)) == 797_184
    # a random state dict from the template: A like a conv weight, B small and non-zero
    tiny = mrisr.UNetConfig.from_oracle_like(__import__("oracle.unet", fromlist=["TINY"]).TINY)
    sd = P.random_state_dict(P.lora_conv_param_shapes(tiny, 4), seed=3, device="cpu")
    k = next(iter(sd))
    assert sd[k].ndim == 4 and float(sd[k].abs().max()) <= 1.0 / math.sqrt(9 * sd[k].shape[1])


def test_disk_key_round_trip_of_4d_adapters():
    from mrisr.train import lora_keys_from_disk, lora_keys_to_disk
    g = torch.Generator().manual_seed(9)
    m = "down_blocks.0.resnets.1.conv2"
    sd = {m + ".lora_A.default.weight": torch.randn((4, 64, 3, 3), generator=g), m + ".lora_B.default.weight": torch.randn((128, 4, 1, 1), generator=g),
          "mid_block.attentions.0.transformer_blocks.0.attn1.to_q.lora_A.default.weight": torch.randn((4, 64), generator=g)}
    for fmt, pre in (("peft", "base_model.model."), ("diffusers", "unet.")):
        disk = lora_keys_to_disk(sd, fmt)
        assert set(disk) == {pre + k.replace(".default", "") for k in sd}
        back = lora_keys_from_disk(disk)
        assert list(back) == list(sd)
        assert all(back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]) for k in sd)
    assert lora_keys_to_disk(sd, "memory") == sd
