#!/usr/bin/env python
"""Register / scratch / occupancy table of the kernels of some .hip files (hipcc -Rpass-analysis=kernel-resource-usage).
usage: tools/kernel_regs.py FILE.hip [FILE.hip ...] [name filter] [-extra hipcc flags]
e.g.   tools/kernel_regs.py posepipeline_amd/csrc/conv_split*.hip conv_split48"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(src, flt, extra):
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{ROOT}/include",
           f"-I{ROOT}/posepipeline_amd/csrc", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-x", "hip", "-c", src, "-o", "/dev/null"] + extra
    t = subprocess.run(cmd, capture_output=True, text=True).stderr
    for b in re.split(r"remark: [^\n]*Function Name: ", t)[1:]:
        name = b.split("\n")[0].strip()
        dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dn = dn.replace("(anonymous namespace)::", "").replace("void ", "")
        if flt and flt not in dn:
            continue
        g = lambda k: re.search(k + r": (\d+)", b).group(1)
        print(f"{dn[:78]:80s} V{g('VGPRs'):>4s} A{g('AGPRs'):>4s} S{g('SGPRs'):>4s} scratch {g('ScratchSize .bytes/lane.'):>4s} occ {g('Occupancy .waves/SIMD.')}")


def main():
    args = sys.argv[1:]
    srcs = [a for a in args if a.endswith(".hip")]
    rest = [a for a in args if not a.endswith(".hip")]
    flt = rest[0] if rest and not rest[0].startswith("-") else ""
    for src in srcs:
        table(src, flt, rest[1:] if flt else rest)


if __name__ == "__main__":
    main()
