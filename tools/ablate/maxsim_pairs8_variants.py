#!/usr/bin/env python3
"""Variant builds of rerank8.hip (diagnostics only): the shipped source compiled with another FZ_MP8_RB into
tools/ablate/libfusion_abl_<name>.so next to the shipped objects.  Usage (where hipcc is): python tools/ablate/maxsim_pairs8_variants.py
Then on the GPU: python tools/bench_maxsim_pairs_fp8.py --variant-lib tools/ablate/libfusion_abl_mp8_rb4.so

  mp8_rb4   4 row blocks in flight instead of 8: half the bytes in flight per wave (8 KiB, 32 A VGPRs), and a register budget that lets
            4 waves per SIMD run at Lq = 64 where the shipped kernel has 3 (rerank8.hip's table).  The same launch plan, the same bits:
            the maximum does not depend on how the row blocks are grouped, and the benchmark tool compares the planes.
  mp8_rb8   the shipped value, built the same way (a control: the variant route must then time like the shipped one)."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "fusion_amd", "csrc")
FLAGS = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()

VARIANTS = {"mp8_rb4": ["-DFZ_MP8_RB=4"], "mp8_rb8": ["-DFZ_MP8_RB=8"]}


def shipped_objects(replaced):
    """The built objects of every source in the Makefile's SRCS except the one this build replaces."""
    srcs = re.search(r"^SRCS := (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    return [os.path.join(CSRC, f[:-len(".hip")] + ".o") for f in srcs if f != replaced]


def main():
    objs = shipped_objects("rerank8.hip")
    for name, defs in VARIANTS.items():
        if (len(sys.argv) > 1 and name not in sys.argv[1:]) or (len(sys.argv) == 1 and name == "mp8_rb8"):
            continue
        obj = f"/tmp/rerank8_abl_{name}.o"
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *defs, "-I", CSRC, "-c", os.path.join(CSRC, "rerank8.hip"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        for ln in r.stderr.splitlines():
            if re.search(r"Function Name|VGPRs|ScratchSize|Occupancy", ln):
                print("   ", ln.split("remark:")[1].split("[-R")[0].strip())
        out = os.path.join(ROOT, "tools", "ablate", f"libfusion_abl_{name}.so")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, obj, *objs, "-ldl"])
        print("built", out)


if __name__ == "__main__":
    main()
