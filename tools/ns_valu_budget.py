#!/usr/bin/env python3
"""Per-phase instruction budget of the fused NS frame kernels (costs no GPU time).

Compiles the kernel source with -DNS1_BUDGET (ns_kernels1.hip): the PRODUCT code -- both bodies of the step, the
run-time predicate between them, no assumption beyond the product's own -- with the NS_STAMP marks as assembly comments
and nothing else changed (no scheduling barrier at a mark: the scheduler may move an instruction across one, so the
per-phase rows are approximate and only their sum is exact).  A mark names the body it stands in: 0 the shared code
(head of the step up to the predicate, tail behind the two bodies), 1 the steady body, 2 the generic body, 3 aside:
blocks the source brackets as not part of a step that goes on (NS_BUDGET_ASIDE .. NS_BUDGET_BACK in ns_kernels1.hip:
the zero-energy exit with its copy of the next step's head, the walk's write-back, drain and publish, the copy of the
head in front of the loop).
Prints, per body and phase, the instruction classes of the <IO16 = false> instantiation in layout order; branch
targets are counted per row so that a conditional block cannot hide inside a phase.

--flow selects the hand-off instantiation <IO16 = false, FLOW = true> (the headline of bench.py) instead of the first
<false, ...> match (the plain build), compiles with the per-file flags of build.py (EXTRA["ns_kernels1.hip"]: the
register figures of that instantiation depend on them) and adds two rows.  "steady step": the sum of the shared rows
(-) and the steady body's rows (S): what a wave executes in a step of the steady body that is followed by another
step of its walk.  The aside rows (A) are left out.  How the conditional blocks that remain in it are counted: in
full, as if entered every step -- the libm fallbacks the compiler left inline and the per-lane branches ("branch
targets inside" counts them); the row is an upper bound of the executed path by those blocks only.  Attribution is by
layout order (an instruction belongs to the last mark in front of it), so a block the compiler moved behind another
mark is counted there.  "generic body": the instructions under the generic body's marks, for comparison.
The marks are asm volatile statements: they keep the compiler from moving memory operations across them, so the
marked build is scheduled a little differently from the product (the hand-off instantiation: 126 VGPRs against 116;
the register figures printed at the end are the marked build's, profiles/*_resource_usage.txt has the product's).

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
    phase = (0, -1)
    per = collections.OrderedDict()
    labels = collections.defaultdict(list)
    inloop = collections.Counter()
    inloop_labels = 0
    generic = collections.Counter()
    for n, l in enumerate(body):
        t = l.strip()
        m = re.match(r"; NS_PHASE (\d+) body (\d)", t)
        if m:
            phase = (int(m.group(2)), int(m.group(1)))
            continue
        if not t or t.startswith((";", ".")) and not re.match(r"^\.LBB", t):
            continue
        if re.match(r"^\.LBB\S+:", t):
            labels[phase].append(t.split(":")[0])
            if phase[1] >= 0 and phase[0] in (0, 1):
                inloop_labels += 1
            continue
        op = t.split()[0]
        per.setdefault(phase, collections.Counter())[classify(op)] += 1
        if phase[1] >= 0 and phase[0] in (0, 1):
            inloop[classify(op)] += 1
        if phase[0] == 2:
            generic[classify(op)] += 1
    cols = list(VALU) + ["s_nop", "salu", "lds", "vmem", "waitcnt", "branch"]
    print("%-18s %5s %6s | " % ("phase", "VALU", "cycles") + " ".join("%7s" % c for c in cols))
    tot = collections.Counter()
    for ph, c in per.items():
        v = sum(c[k] for k in VALU)
        name = "prologue" if ph[1] < 0 else "%s%2d %s" % ("-SGA"[ph[0]], ph[1], NAMES[ph[1]] if ph[1] < len(NAMES) else "aside")
        cyc = sum(c[k] * PRICE[k] for k in VALU)
        print("%-18s %5d %6.0f | " % (name, v, cyc) + " ".join("%7d" % c[k] for k in cols) + ("   labels: %d" % len(labels[ph]) if labels[ph] else ""))
        tot.update(c)
    v = sum(tot[k] for k in VALU)
    print("%-18s %5d %6.0f | " % ("total", v, sum(tot[k] * PRICE[k] for k in VALU)) + " ".join("%7d" % tot[k] for k in cols))
    if flow:
        if inloop:
            v = sum(inloop[k] for k in VALU)
            print("%-18s %5d %6.0f | " % ("steady step", v, sum(inloop[k] * PRICE[k] for k in VALU)) + " ".join("%7d" % inloop[k] for k in cols)
                  + "   (rows - and S; branch targets inside: %d)" % inloop_labels)
            v = sum(generic[k] for k in VALU)
            print("%-18s %5d %6.0f | " % ("generic body", v, sum(generic[k] * PRICE[k] for k in VALU)) + " ".join("%7d" % generic[k] for k in cols))
        else:
            print("steady step: no phase marks found")
    # register figures of every kernel of the (marked) build, by name
    name = None
    for l in lines:
        m = re.match(r"\s*\.name:\s+(\S+)", l)
        if m and not m.group(1).endswith(".kd"):
            name = m.group(1)
        m = re.match(r"\s*\.(sgpr_count|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", l)
        if m:
            print("%-22s %4s  %s" % (m.group(1), m.group(2), name))


if __name__ == "__main__":
    main()
