#!/usr/bin/env python3
"""Per-phase instruction budget of the fused NS frame kernels (costs no GPU time).

Compiles the kernel source with -DNS1_BUDGET (ns_kernels1.hip): the NS_STAMP marks become assembly
comments and the steady-state conditions (past start-up, no tracker publish, histogram window open,
no libm fallback) are asserted, so the code between two marks is what one wave executes per frame.
Prints, per phase, the instruction classes of the <IO16 = false> instantiation; branch targets that
survive are listed so that a cold block cannot hide inside a phase.

--flow selects the hand-off instantiation <IO16 = false, FLOW = true> (the headline of bench.py) instead of the first
<false, ...> match (the plain build), compiles with the per-file flags of build.py (EXTRA["ns_kernels1.hip"]: the
register figures of that instantiation depend on them) and adds a "loop body" row: what lies between the header of
the step loop and its back edge, i.e. one steady-state frame step without the once-per-chunk set-up in front of it.

usage: tools/ns_valu_budget.py [source.hip] [--flow] [--dump out.s] [extra hipcc flags...]
"""
import importlib.util
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["in+energy", "fftF", "g2loads+magn+log", "sums1", "trackers", "startup", "snr", "flat+diff", "lrt+exp",
         "hist+prob", "noiseupd", "gain", "ifft", "gainfac", "ola", "scalars", "tail"]


def classify(op):
    if op.startswith("v_"):
        if op.startswith(("v_mov_b", "v_accvgpr")):
            return "mov"
        if op.startswith("v_cndmask"):
            return "cndmask"
        if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
            return "lane"
        if op.startswith("v_permlane"):
            return "permlane"
        if op.startswith("v_cmp") or op.startswith("v_cmpx"):
            return "cmp"
        if "_dpp" in op:
            return "dpp"
        if op.startswith("v_pk_"):
            return "pk_f32"
        if op.endswith("_f64") or "_f64_" in op:
            return "f64"
        if op.startswith(("v_rcp", "v_rsq", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")):
            return "trans"
        if op.startswith("v_cvt"):
            return "cvt"
        if re.match(r"v_(max|min|med3)_", op):
            return "cmp"  # v_max_f32 issues at the 2.8-cycle rate
        if re.match(r"v_(add|sub|subrev|mul|fma|fmac|mac|mad|ldexp|rndne|fract|floor|trunc)_f32", op) or op.startswith("v_fma_f32"):
            return "f32"
        return "int/bit"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


VALU = ("mov", "cndmask", "lane", "permlane", "cmp", "dpp", "pk_f32", "f64", "trans", "cvt", "f32", "int/bit")
# SIMD cycles per wave64 instruction with four waves per SIMD issuing (tools/probe/issue_probe3.hip,
# profiles/r03_issue_probe3.txt): plain f32 / integer / move 1.7, packed f32 / f64 / compare / select /
# lane / DPP / conversion 2.8, transcendental and v_permlane32_swap 5.3
PRICE = {"mov": 1.73, "f32": 1.73, "int/bit": 1.75, "cndmask": 2.78, "lane": 2.8, "cmp": 2.78, "dpp": 2.78,
         "pk_f32": 2.78, "f64": 2.77, "cvt": 2.7, "trans": 5.3, "permlane": 5.3}


def main():
    args = sys.argv[1:]
    src = os.path.join(ROOT, "audiosignalprocess_amd", "csrc", "ns_kernels1.hip")
    dump = None
    flow = False
    extra = []
    i = 0
    while i < len(args):
        if args[i] == "--dump":
            dump = args[i + 1]
            i += 2
        elif args[i] == "--flow":
            flow = True
            i += 1
        elif args[i].endswith(".hip"):
            src = args[i]
            i += 1
        else:
            extra.append(args[i])
            i += 1
    perfile = ["-mllvm", "-amdgpu-kernarg-preload-count=8"]
    if flow:  # the product's own flags for this file (a plain list in build.py; loaded without importing the package)
        spec = importlib.util.spec_from_file_location("asp_build", os.path.join(ROOT, "audiosignalprocess_amd", "build.py"))
        bld = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bld)
        perfile = list(bld.EXTRA["ns_kernels1.hip"])
    out = dump or os.path.join(tempfile.mkdtemp(), "k.s")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"] + perfile + ["-DNS1_BUDGET", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "audiosignalprocess_amd", "csrc"), "-S", "--cuda-device-only", "-o", out, src] + extra
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    # the <false, ...> instantiation (--flow: <false, true>): from its label to its s_endpgm
    want = r"^_Z.*kernelILb0ELb1E.*:" if flow else r"^_Z.*kernelILb0E.*:"
    start = next(i for i, l in enumerate(lines) if re.match(want, l))
    body = []
    for l in lines[start + 1:]:
        body.append(l)
        if l.strip().startswith(".Lfunc_end"):
            break
    phase = -1
    per = collections.OrderedDict()
    labels = collections.defaultdict(list)
    # the step loop (--flow): the backward branch with the longest reach that spans phase marks, and its target
    loop = None
    if flow:
        where = {}
        for n, l in enumerate(body):
            m = re.match(r"^(\.LBB\S+):", l.strip())
            if m:
                where[m.group(1)] = n
        marks = [n for n, l in enumerate(body) if l.strip().startswith("; NS_PHASE")]
        for n, l in enumerate(body):
            t = l.split()
            if len(t) >= 2 and t[0].startswith(("s_cbranch", "s_branch")) and where.get(t[1], n) < n:
                h = where[t[1]]
                if any(h < k < n for k in marks) and (loop is None or n - h > loop[1] - loop[0]):
                    loop = (h, n)
    inloop = collections.Counter()
    for n, l in enumerate(body):
        t = l.strip()
        m = re.match(r"; NS_PHASE (\d+)", t)
        if m:
            phase = int(m.group(1))
            continue
        if not t or t.startswith((";", ".")) and not re.match(r"^\.LBB", t):
            continue
        if re.match(r"^\.LBB\S+:", t):
            labels[phase].append(t.split(":")[0])
            continue
        op = t.split()[0]
        per.setdefault(phase, collections.Counter())[classify(op)] += 1
        if loop and loop[0] <= n <= loop[1]:
            inloop[classify(op)] += 1
    cols = list(VALU) + ["s_nop", "salu", "lds", "vmem", "waitcnt", "branch"]
    print("%-18s %5s %6s | " % ("phase", "VALU", "cycles") + " ".join("%7s" % c for c in cols))
    tot = collections.Counter()
    for ph, c in per.items():
        v = sum(c[k] for k in VALU)
        name = "prologue" if ph < 0 else "%2d %s" % (ph, NAMES[ph] if ph < len(NAMES) else "")
        cyc = sum(c[k] * PRICE[k] for k in VALU)
        print("%-18s %5d %6.0f | " % (name, v, cyc) + " ".join("%7d" % c[k] for k in cols) + ("   labels: %d" % len(labels[ph]) if labels[ph] else ""))
        tot.update(c)
    v = sum(tot[k] for k in VALU)
    print("%-18s %5d %6.0f | " % ("total", v, sum(tot[k] * PRICE[k] for k in VALU)) + " ".join("%7d" % tot[k] for k in cols))
    if flow:
        if loop:
            v = sum(inloop[k] for k in VALU)
            print("%-18s %5d %6.0f | " % ("loop body", v, sum(inloop[k] * PRICE[k] for k in VALU)) + " ".join("%7d" % inloop[k] for k in cols)
                  + "   (%s .. its back edge)" % body[loop[0]].strip().rstrip(":"))
        else:
            print("loop body: no backward branch across the phase marks found")
    m = re.search(r"\.vgpr_count:\s+(\d+)", "\n".join(lines[::-1]))
    for l in lines:
        if "vgpr_count" in l or "sgpr_count" in l or "vgpr_spill" in l:
            print(l.strip())


if __name__ == "__main__":
    main()
