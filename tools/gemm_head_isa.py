"""The head of gemm_bl_kernel / gemm_halo_kernel in the compiled ISA: static instructions, scalar loads, scalar waits and integer-division
sequences between the kernel's entry and its first LDS-DMA (`buffer_load_dwordx4 ... lds`), for the three instantiations DESIGN.md 28 quotes.
Input: the gfx950 assembly of csrc/gemm.hip, e.g. from
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -save-temps=obj -c mri-diffusion-superresolution_amd/csrc/gemm.hip -o build/gemm.o
Usage: python tools/gemm_head_isa.py build/gemm-hip-amdgcn-amd-amdhsa-gfx950.s [-v]"""
import re
import sys

KERNELS = [
    ("gemm_bl_kernel<64,160,2,2,2,false>", "_ZN5mrisr14gemm_bl_kernelILi64ELi160ELi2ELi2ELi2ELb0EEE"),
    ("gemm_bl_kernel<64,64,2,2,2,true>", "_ZN5mrisr14gemm_bl_kernelILi64ELi64ELi2ELi2ELi2ELb1EEE"),
    ("gemm_halo_kernel<128,160,2,2>", "_ZN5mrisr16gemm_halo_kernelILi128ELi160ELi2ELi2EEE"),
]


def head(lines, prefix):
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(";")[0].rstrip().endswith(":"))
    ins = []
    for l in lines[start + 1:]:
        t = l.strip()
        t = t.split(";")[0].strip()
        if not t or t.startswith((".", "//")) or t.endswith(":"):
            continue
        if t.startswith("s_endpgm"):
            break
        op = t.split()[0]
        ins.append(t)
        if op.startswith("buffer_load_dwordx4") and re.search(r"\blds\b", t):
            return ins
    raise SystemExit(f"{prefix}: no LDS-DMA found")


def main():
    lines = open(sys.argv[1], errors="replace").read().splitlines()
    verbose = "-v" in sys.argv[2:]
    print("kernel | static instructions | s_load | s_waitcnt lgkmcnt | v_rcp_iflag   (entry .. first LDS-DMA)")
    for name, prefix in KERNELS:
        ins = head(lines, prefix)
        n_load = sum(1 for t in ins if t.startswith("s_load_"))
        n_wait = sum(1 for t in ins if t.startswith("s_waitcnt") and "lgkmcnt" in t)
        n_rcp = sum(1 for t in ins if t.startswith("v_rcp_iflag"))
        print(f"{name} | {len(ins)} | {n_load} | {n_wait} | {n_rcp}")
        if verbose:
            for k, t in enumerate(ins):
                if t.startswith(("s_load_", "s_waitcnt", "v_rcp_iflag", "s_cbranch", "buffer_load")):
                    print(f"    {k:5d}  {t}")


if __name__ == "__main__":
    main()
