#!/usr/bin/env python
"""Compare the compiler's output for the split-conv kernels of two source trees, kernel by kernel.
usage: tools/kernel_isa_diff.py OLD_TREE NEW_TREE [extra hipcc flags]

Every posepipeline_amd/csrc/conv_split*.hip of each tree is compiled with the Makefile's flags plus --cuda-device-only -S and the
assembly is cut into kernels, keyed by demangled name without "(anonymous namespace)::" (so a kernel may move between files).
Per kernel: the resource figures of its metadata (VGPRs, AGPRs, SGPRs, private / group segment size, VGPR / SGPR spills), its
instruction count, and whether its instruction text is the same after normalisation (comments and directives dropped, local labels
numbered in order of appearance).  Whole texts are compared; no particular instruction is looked for.
Exit status 1 if the sets of kernel names differ or any resource figure differs, else 0 (a differing text alone is reported only)."""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FIGURES = ["vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
           "vgpr_spill_count", "sgpr_spill_count"]


def assembly(tree, src, extra):
    tree = os.path.abspath(tree)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{tree}/include",
               f"-I{tree}/posepipeline_amd/csrc", "-ffp-contract=off", "-Wno-unused-function", "-w", "--cuda-device-only", "-S",
               "-x", "hip", src, "-o", out] + extra
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{src}: compile failed\n{r.stderr[-2000:]}")
        return open(out).read()


def normalise(body):
    labels, text = {}, []
    for line in body.split("\n"):
        line = line.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.endswith(":")):
            continue                                  # comment, blank or directive
        text.append(re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), line))
    return text


def kernels(tree, extra):
    srcs = sorted(glob.glob(os.path.join(tree, "posepipeline_amd/csrc/conv_split*.hip")))
    with ThreadPoolExecutor(max_workers=4) as pool:
        return parse(list(pool.map(lambda s: assembly(tree, s, extra), srcs)))


def parse(asms):
    found = {}
    for asm in asms:
        meta = asm[asm.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in asm else ""
        for block in re.split(r"\n  - (?=\.)", meta)[1:]:
            kv = dict(re.findall(r"^(?:    )?\.(\w+):\s+(\S+)\s*$", block, re.M))
            name = kv["name"].strip("'\"")
            body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S).group(1)
            text = normalise(body)
            ninstr = sum(1 for t in text if not t.endswith(":"))
            found[name] = ([int(kv[f]) for f in FIGURES], ninstr, text)
    names = list(found)
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.strip().split("\n")
    return {p.replace("(anonymous namespace)::", "").replace("void ", "", 1): found[n] for n, p in zip(names, plain)}


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    extra = sys.argv[3:]
    old, new = kernels(sys.argv[1], extra), kernels(sys.argv[2], extra)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name[:100]:100s} only in {'NEW' if name in new else 'OLD'}")
            bad += 1
            continue
        (fo, no, to), (fn, nn, tn) = old[name], new[name]
        figs = " ".join(f"{a}" if a == b else f"{a}->{b}!" for a, b in zip(fo, fn))
        count = f"{no}" if no == nn else f"{no}->{nn}"
        print(f"{name[:100]:100s} V A S priv lds vspill sspill: {figs}  instr {count}  {'same' if to == tn else 'differs'}")
        bad += fo != fn
    same = sum(1 for n in old if n in new and old[n][2] == new[n][2])
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {same} with the same text; {bad} with other names or resource figures")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
