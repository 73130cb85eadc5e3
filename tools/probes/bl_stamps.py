"""Where the tiled (gemm_bl_kernel) and halo (gemm_halo_kernel) GEMMs spend their time: clock stamps (s_memtime: shader-clock ticks, about 2.1 per ns under load) written by wave 0 of
every workgroup at eight phase boundaries (mrisr_debug_gemm_stamps), on the bench workload (SD-1.5 + rank-4 LoRA, B = 32, 32 x 32 latents,
the shipped tile table).  Two eager denoising steps per run: the first warms up, the second is stamped - the launches see their operands as
cold as a model step leaves them.  Prints the median ticks per phase over all workgroups of all launches of three signatures, with the plain
staged epilogue (flags 0) and, with --generic, also through the generic epilogue4 (mrisr_debug_gemm_flags(64)).  Stamp 1 is "head finished,
stage-0 DMA all issued" (before the launch head it was "offsets and descriptors ready", the DMA still to be issued), so the
figure to compare across builds is entry -> first stage landed (stamp 2 - stamp 0), printed on its own line.
Usage (GPU box): python tools/probes/bl_stamps.py [--generic]"""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, os.path.join(ROOT, "mri-diffusion-superresolution_amd"))
os.environ.setdefault("MRISR_TUNE_CACHE", os.path.join(ROOT, "profiles", "r03_tune_cache.tsv"))
import mrisr
from mrisr import _lib as L
from mrisr import params as P

HDR, WGS, SLOTS = 8, 1024, 256  # include/mrisr_debug.h: mrisr_debug_gemm_stamps
SLOT = HDR + 8 * WGS
RESID, LORA, CONV = 1, 2, 4
# name, tile id (csrc/gemm.hip: TILES), M, N, K, header bits that must be set
SIGNATURES = [
    ("bl64x160 M=8192 N=K=640 +resid", 26, 8192, 640, 640, RESID),
    ("bl64x64 M=2048 N=K=1280 +LoRA", 17, 2048, 1280, 1280, LORA),
    ("halo128x160 conv2 level 0 (M=32768 N=320 K=2880) +resid", 41, 32768, 320, 2880, RESID | CONV),
]
PHASES = ["head, stage-0 DMA issued", "first stage lands", "K loop", "LoRA z, bias ready", "epilogue into LDS", "residual loaded", "add + stores issued"]

B = 32
cfg = mrisr.UNetConfig()
net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4)
sd = P.random_state_dict(P.unet_param_shapes(cfg), 1, "cuda")
sd.update(P.random_state_dict(P.lora_param_shapes(cfg, 4), 4, "cuda"))
net.load_state_dict(sd)
g = torch.Generator().manual_seed(5)
x = torch.randn((B, 4, 32, 32), generator=g).cuda()
ctx = torch.randn((B, 77, 768), generator=g).cuda()
t = torch.tensor(500).cuda()
lib = L.lib()
lib.mrisr_debug_gemm_stamps.argtypes = [C.c_void_p, C.c_int]
for _ in range(2):
    net(x, t, encoder_hidden_states=ctx)
torch.cuda.synchronize()
buf = torch.zeros((SLOTS, SLOT), dtype=torch.int64, device="cuda")


def stamped_step(tile, flags):
    lib.mrisr_debug_gemm_flags(flags)
    net(x, t, encoder_hidden_states=ctx)
    buf.zero_()
    torch.cuda.synchronize()
    lib.mrisr_debug_gemm_stamps(C.c_void_p(buf.data_ptr()), tile)
    net(x, t, encoder_hidden_states=ctx)
    torch.cuda.synchronize()
    lib.mrisr_debug_gemm_stamps(C.c_void_p(0), 0)
    lib.mrisr_debug_gemm_flags(0)
    return buf.cpu()


for name, tile, M, N, K, bits in SIGNATURES:
    print(f"== {name} (tile {tile})")
    for label, flags in ((("generic epilogue (flag 64)", 64),) if "--generic" in sys.argv[1:] else ()) + (("plain staged epilogue (flags 0)", 0),):
        s = stamped_step(tile, flags)
        rows = []
        for k in range(SLOTS):
            h = s[k, :HDR]
            if int(h[7]) != 1 or (int(h[0]), int(h[1]), int(h[2])) != (M, N, K) or (int(h[4]) & bits) != bits:
                continue
            n = min(int(h[3]), WGS)
            w = s[k, HDR:HDR + 8 * n].reshape(n, 8)
            if int(w[0, 6]) == 0:  # stamp 6 is written by the staged copy-out pass only: a head-major (Q / K / V) launch, not this signature
                continue
            rows.append(w)
        if not rows:
            print(f"  {label}: no launch of this signature on tile {tile}")
            continue
        st = torch.cat(rows).double()
        d = st[:, 1:] - st[:, :-1]
        med = d.median(0).values
        tot = (st[:, 7] - st[:, 0]).median()
        print(f"  {label}: {len(rows)} launches, {st.shape[0]} workgroups; median ticks per phase, whole workgroup {tot:.0f}")
        print(f"    {'entry -> first stage landed':24s} median {(st[:, 2] - st[:, 0]).median():7.0f}   mean {(st[:, 2] - st[:, 0]).mean():8.1f}")
        for nm, v, mean in zip(PHASES, med.tolist(), d.mean(0).tolist()):
            print(f"    {nm:24s} median {v:7.0f}   mean {mean:8.1f}")
