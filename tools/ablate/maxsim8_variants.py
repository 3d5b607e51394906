#!/usr/bin/env python3
"""Variant builds of maxsim8.hip (diagnostics only): each is a textual patch of the shipped source compiled into
tools/ablate/libfusion_abl_<name>.so next to the shipped objects.  Usage (where hipcc is): python tools/ablate/maxsim8_variants.py
Then on the GPU: python tools/bench_maxsim_fp8.py --only timing --variant-lib tools/ablate/libfusion_abl_m8_cb16.so

  m8_cb16   16 column blocks per wave (8 query blocks of 32 tokens, 128 VGPRs of query fragments): a workgroup covers 32 queries of 64
            tokens instead of 16, every document tile read from LDS feeds twice the MFMAs.  Another launch plan (the query assignment of
            tests/maxsim_cases.launch_plan no longer holds), so it is a variant and not a switch; its score planes are compared with the
            shipped kernel's by the benchmark tool."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "fusion_amd", "csrc")
SRC = open(os.path.join(CSRC, "maxsim8.hip")).read()
FLAGS = "-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage".split()

VARIANTS = {
    "m8_cb16": [("constexpr int M8_BLOCKS_PER_WAVE = 4;", "constexpr int M8_BLOCKS_PER_WAVE = 8;")],
}


def shipped_objects(replaced):
    """The built objects of every source in the Makefile's SRCS except the one this build replaces."""
    srcs = re.search(r"^SRCS := (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    return [os.path.join(CSRC, f[:-len(".hip")] + ".o") for f in srcs if f != replaced]


def main():
    objs = shipped_objects("maxsim8.hip")
    for name, patches in VARIANTS.items():
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        s = SRC
        for a, b in patches:
            assert s.count(a) == 1, (name, a)
            s = s.replace(a, b)
        src, obj = f"/tmp/maxsim8_abl_{name}.hip", f"/tmp/maxsim8_abl_{name}.o"
        open(src, "w").write(s)
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-I", CSRC, "-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        for ln in r.stderr.splitlines():
            if re.search(r"Function Name|VGPRs|ScratchSize|Occupancy", ln):
                print("   ", ln.split("remark:")[1].split("[-R")[0].strip())
        out = os.path.join(ROOT, "tools", "ablate", f"libfusion_abl_{name}.so")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, obj, *objs, "-ldl"])
        print("built", out)


if __name__ == "__main__":
    main()
