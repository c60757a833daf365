#!/usr/bin/env python3
"""Is the device listing of a source file the one an earlier revision gave?  (costs no GPU time)

Compiles one file of audiosignalprocess_amd/csrc twice to gfx950 assembly -- from a git revision (the file and the
headers of that revision, unpacked into a temporary directory) and from the working tree -- with build.py's FLAGS, its
per-file EXTRA and its include paths, and prints per function (kernels and the out-of-line device functions) whether
the two instruction streams are equal once comment lines, directives and the __hip_cuid_* symbol are dropped.  Where
they are not, the kernels' register, spill, scratch and LDS figures and the instruction totals stand side by side.
It compares and nothing else: no instruction is inspected.  Exit status 0: every function equal; 1: not.

usage: tools/listing_diff.py <file.hip> <revision>
"""
import concurrent.futures
import importlib.util
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = ["vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
           "group_segment_fixed_size"]


def load_build():  # build.py's lists, without importing the package (which would load the library)
    spec = importlib.util.spec_from_file_location("asp_build", os.path.join(ROOT, "audiosignalprocess_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    return bld


def compile_listing(bld, root, name, out):
    csrc = os.path.join(root, "audiosignalprocess_amd", "csrc")
    cmd = ([bld.hipcc()] + bld.FLAGS + bld.EXTRA.get(name, []) + ["-I" + os.path.join(root, "include"), "-I" + csrc]
           + ["-S", "--offload-device-only", "-o", out, os.path.join(csrc, name)])
    subprocess.run(cmd, check=True)
    return open(out).read().split("\n")


def parse(lines):
    """({function: [instruction or label, ...]}, {kernel: {figure: value}}) of a listing, functions in layout order"""
    funcs, cur = {}, None
    for l in lines:
        t = l.split(";")[0].strip()
        if "__hip_cuid_" in l or not t:
            continue
        m = re.match(r"^([A-Za-z_$][\w$]*):$", t)  # a function's label (local labels and metadata keys carry a dot)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if t.startswith(".Lfunc_end"):
            cur = None
        if cur is None or (t.startswith(".") and not re.match(r"^\.LBB\S+:$", t)):
            continue
        cur.append(t)
    figures, block = {}, {}
    for l in lines + ["- ."]:  # the metadata: one block of alphabetical keys per kernel, opened by "- ."
        if re.match(r"\s*- \.", l):
            if block.get("name") in funcs:
                figures[block["name"]] = {k: int(block[k]) for k in FIGURES if k in block}
            block = {}
        m = re.match(r"\s*(?:- )?\.(\w+):\s+(\S+)\s*$", l)
        if m:
            block[m.group(1)] = m.group(2)
    return {k: v for k, v in funcs.items() if v}, figures


def demangled(names):
    try:
        out = subprocess.run(["c++filt", "-p"] + names, check=True, capture_output=True, text=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    name, rev = os.path.basename(sys.argv[1]), sys.argv[2]
    bld = load_build()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "audiosignalprocess_amd/csrc", "include"], check=True,
                             capture_output=True).stdout
        old_root = os.path.join(tmp, "old")
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old_root)
        with concurrent.futures.ThreadPoolExecutor(2) as ex:
            old = ex.submit(compile_listing, bld, old_root, name, os.path.join(tmp, "old.s"))
            new = ex.submit(compile_listing, bld, ROOT, name, os.path.join(tmp, "new.s"))
            (f0, r0), (f1, r1) = parse(old.result()), parse(new.result())
    names = list(f0) + [n for n in f1 if n not in f0]
    pretty = demangled(names)
    differ = 0
    for n in names:
        a, b = f0.get(n), f1.get(n)
        kind = "kernel" if n in r0 or n in r1 else "function"
        if a == b:
            print("equal    %-8s %s  (%d lines)" % (kind, pretty[n], len(a)))
            continue
        differ += 1
        print("DIFFERS  %-8s %s" % (kind, pretty[n]))
        print("    %-28s %10s %10s" % ("", rev[:10], "tree"))
        count = lambda f: "-" if f is None else sum(1 for t in f if not t.endswith(":"))
        print("    %-28s %10s %10s" % ("instructions", count(a), count(b)))
        for prefix in ("v_", "s_", "ds_"):
            cnt = lambda f: "-" if f is None else sum(1 for t in f if t.startswith(prefix))
            print("    %-28s %10s %10s" % ("  " + prefix + "*", cnt(a), cnt(b)))
        for k in FIGURES:
            if n in r0 or n in r1:
                print("    %-28s %10s %10s" % (k, r0.get(n, {}).get(k, "-"), r1.get(n, {}).get(k, "-")))
    print("%s against %s: %d of %d functions differ" % (name, rev, differ, len(names)))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
