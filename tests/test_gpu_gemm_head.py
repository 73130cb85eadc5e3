"""GPU: the launch head of the tiled (gemm_bl_kernel) and halo (gemm_halo_kernel) GEMMs (csrc/gemm_head.h) changes addressing
and issue order only - host-computed launch constants, multiply-and-shift divisions, the stage-0 DMA at the top of the kernel - so every
output bit stays what it was.  Each case of tests/gemm_head_cases.py (closed-form operands, exact in bf16) is held three ways:

  * against a float64 reference of the bf16-rounded operands at the relative-L2 bound tests/test_gpu_ops.py uses for bf16 (1.2e-2);
  * bit-equal (torch.equal) with and without the LDS poisoned before the first DMA (mrisr_debug_gemm_flags 2048: a read that ran ahead of
    its DMA, or a DMA issued ahead of the poisoning, would show NaN);
  * bit-equal to the SHA-256 recorded from the library of the commit before the head existed (tests/golden/gemm_head/bits.json, written by
    `python tests/gemm_head_cases.py --record`).

The shapes are the smallest that reach each branch of the head: see cases() there.  The whole TINY denoiser forward is held to its recorded
bits and, against the CPU oracle, to the bf16 bound of smoke() (6e-2): it is a whole network, not one GEMM, and measures 1.223e-2 - the
parent's library gives the same bits - against the single-GEMM 1.2e-2."""
import json
import os

import pytest
import torch

import gemm_head_cases as G

pytestmark = pytest.mark.gpu

TOL_BF16 = 1.2e-2  # tests/test_gpu_ops.py: TOL["bf16"]
TOL_UNET = 6e-2    # __graft_entry__.smoke(): the bf16 forward against the CPU oracle
CASES = G.cases()
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_head", "bits.json")) as _f:
    BITS = json.load(_f)


def test_every_case_has_recorded_bits():
    assert sorted(CASES) == sorted(BITS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_matches_float64_poisoned_lds_and_recorded_bits(name):
    y, yp, ref = G.run_both(CASES[name])
    e = G.rel(y, ref)
    print(f"{name}: rel-l2 vs float64 {e:.3e}")
    assert torch.isfinite(y.float()).all()
    assert e < (TOL_UNET if name.startswith("unet") else TOL_BF16), e
    assert torch.equal(y, yp), "poisoned LDS changed the result"
    assert G.digest(y) == BITS[name], "output bits differ from the ones recorded before the launch head"


def test_group_m_cases_reach_short_and_oversized_groups():
    """The group sizes of the cases above on their five M tiles (M = 272 on 64-row tiles): 2 leaves a last group of 1, 3 one of 2, 8 is larger
    than the grid.  The hook that sets them exists (a library without it would run every one of those cases in the default order), and the
    order moves no output bit."""
    from mrisr import _lib as L
    lib = L.lib()
    assert hasattr(lib, "mrisr_debug_group_m")
    base, _ = G.linear_case(G.T64x64, 272, 160, 128)()
    for gm in (1, 2, 3, 8):
        y, _ = G.linear_case(G.T64x64, 272, 160, 128, group_m=gm)()
        assert torch.equal(y, base), gm
