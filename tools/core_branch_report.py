#!/usr/bin/env python3
"""Which lines and branches of a CPU-built core do the suite's runs never reach?

    python tools/core_branch_report.py all golden > profiles/core_branches_parent.txt
    python tools/core_branch_report.py nsx agc both > profiles/core_branches.txt

For a named core (aecm nsx splrs agc ts bf hpf ab, or all) this builds csrc/<core>_restate.cpp with g++ --coverage -O0
in a temporary directory, replays a set of runs against that library in a child process, runs gcov -b -c (-m, for
readable function names) from the directory of the compile -- the notes file holds relative source paths, and gcov run
from elsewhere reports nothing without saying so -- and prints every line of csrc/<core>_core.h that never ran and
every branch that was never taken, with function and source line.  CPU only; needs g++ and gcov.

Run sets, over the core's tests/test_<core>*_host.py files:
  edges   the tests named in EDGE_TESTS below: the EDGE_RUNS, SEEDED and EDGE_GRID cases of tests/nsx_runs.py and
          tests/agc_runs.py and the fused call's test (a core without an entry has no such set);
  golden  every other test of those files: what the host suite replayed before the edge runs;
  both    every test of those files.
The child loads the instrumented library wherever a test opens lib<core>_restate.so: ctypes.CDLL is wrapped, so the
tests themselves do not know.  The one-lane CPU build never takes the other arm of an `if (L.id == 0)`, `if (g.is(n))`
or `if (write)`; the report marks those lines with (lane), tests/core_branch_exemptions.py names the class once.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audiosignalprocess_amd", "csrc")
HOST_TESTS = {"aecm": ["test_aecm_host.py"], "nsx": ["test_nsx_host.py"], "splrs": ["test_splrs_host.py"],
              "agc": ["test_agc_host.py"], "ts": ["test_ts_host.py"], "bf": ["test_bf_host.py", "test_bf_edges_host.py"],
              "hpf": ["test_hpf_host.py"], "ab": ["test_ab_host.py"]}
SETS = ("golden", "edges", "both")
EDGE_TESTS = {
    "nsx": ["test_restatement_equals_edge_golden", "test_restatement_equals_seeded_edge_case",
            "test_edge_golden_stores_what_names_a_failing_block"],
    "agc": ["test_restatement_equals_edge_golden", "test_restatement_equals_seeded_edge_case",
            "test_gain_table_equals_the_reference_over_the_edge_grid", "test_by_mode_frames_equal_the_explicit_operations"],
}


def selection(core, which):
    names = " or ".join(EDGE_TESTS.get(core, []))
    if which == "both" or (which == "golden" and not names):
        return []
    if not names:
        raise SystemExit("%s has no edge tests" % core)
    return ["-k", names if which == "edges" else "not (%s)" % names]


LANE = re.compile(r"^(\} else )?if \((L\.id == 0|g\.is\(\d\)|write)\)")   # a lane condition alone, not one term of several


def drive(core, which, lib):
    """child process: every open of lib<core>_restate.so goes to the instrumented build"""
    import ctypes

    import pytest

    name = "lib%s_restate.so" % core
    plain = ctypes.CDLL.__init__

    def redirected(self, path, *a, **kw):
        plain(self, lib if isinstance(path, str) and os.path.basename(path) == name else path, *a, **kw)

    ctypes.CDLL.__init__ = redirected
    files = [os.path.join(ROOT, "tests", f) for f in HOST_TESTS[core]]
    return int(pytest.main(["-q", "-x", "-p", "no:cacheprovider", "--rootdir", ROOT] + selection(core, which) + files))


def measure(core, which):
    """Returns (rows, totals): rows are (function, line, kind, branch, source) with kind "line" (never executed) or
    "branch" (never taken; branch is gcov's index on that line), totals (lines, lines run, branches, branches taken)."""
    for exe in ("g++", "gcov"):
        if shutil.which(exe) is None:
            raise RuntimeError("%s not found: the branch report cannot be made" % exe)
    header = "%s_core.h" % core
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "lib%s_restate.so" % core)
        subprocess.run(["g++", "-O0", "--coverage", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, os.path.join(CSRC, "%s_restate.cpp" % core), "-o", lib], check=True, cwd=tmp)
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--drive", core, which, lib], cwd=tmp, env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if run.returncode != 0:
            raise RuntimeError("the %s runs of %s did not pass on the instrumented library:\n%s" % (which, core, run.stdout[-4000:]))
        gcda = [f for f in os.listdir(tmp) if f.endswith(".gcda")]
        if not gcda:
            raise RuntimeError("the instrumented library wrote no counts")
        subprocess.run(["gcov", "-b", "-c", "-m", gcda[0]], check=True, cwd=tmp, stdout=subprocess.DEVNULL)
        with open(os.path.join(tmp, header + ".gcov")) as f:
            return parse_gcov(f.read().splitlines())


def parse_gcov(text):
    # A template's lines come once with the counts of all its instantiations added up, then once more per instantiation
    # between rows of dashes, and only there with their branches: a line counts where it is first met, a branch is taken
    # when any instantiation takes it.
    func, line_no, ran, count_of, branch_of = "?", 0, {}, {}, {}
    for row in text:
        m = re.match(r"function (.+) called \d+ returned", row)
        if m:
            func = simple_name(m.group(1))
            continue
        m = re.match(r"\s*([^:\s]+):\s*(\d+):(.*)", row)
        if m:
            line_no = int(m.group(2))
            count = m.group(1).rstrip("*")
            if count != "-" and line_no > 0 and line_no not in ran:
                ran[line_no] = count not in ("#####", "=====", "0")
                count_of[line_no] = (func, m.group(3).strip())
            continue
        m = re.match(r"branch\s+(\d+) (never executed|taken (\d+))", row)
        if m:
            key = (line_no, int(m.group(1)))
            hit = m.group(2) != "never executed" and int(m.group(3)) > 0
            branch_of[key] = (func, branch_of.get(key, (func, False))[1] or hit)
    rows = [(count_of[n][0], n, "line", -1, count_of[n][1]) for n in sorted(ran) if not ran[n]]
    # a line that never ran has said so once: its branches are not listed again
    rows += [(f, n, "branch", b, count_of.get(n, (f, ""))[1]) for (n, b), (f, hit) in sorted(branch_of.items())
             if not hit and ran.get(n, True)]
    rows.sort(key=lambda r: (r[1], r[3]))
    return rows, (len(ran), sum(ran.values()), len(branch_of), sum(hit for _, hit in branch_of.values()))


def simple_name(name):
    """do_it from aspcore::do_it(int) or from _ZN7aspcore5do_itILi1EEEvi"""
    m = re.match(r"_ZN?", name)
    if not m:
        return re.sub(r"[(<].*", "", name).split(" ")[-1].split("::")[-1]
    rest, last = name[m.end():], name
    while True:
        m = re.match(r"(\d+)", rest)
        if not m:
            return last
        k = int(m.group(1))
        last, rest = rest[m.end():m.end() + k], rest[m.end() + k:]


def report(core, which):
    rows, (lines, lines_run, branches, taken) = measure(core, which)
    print("== %s_core.h, run set '%s': %d of %d lines never executed (%.2f %% executed), %d of %d branches never taken "
          "(%.2f %% taken)" % (core, which, lines - lines_run, lines, 100.0 * lines_run / max(lines, 1), branches - taken,
                               branches, 100.0 * taken / max(branches, 1)))
    for func, line_no, kind, br, source in rows:
        what = "never executed" if kind == "line" else "branch %d never taken%s" % (br, " (lane)" if LANE.search(source) else "")
        print("%-28s %s_core.h:%-5d %-30s | %s" % (func, core, line_no, what, source))
    print()


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--drive":
        sys.exit(drive(sys.argv[2], sys.argv[3], sys.argv[4]))
    args = sys.argv[1:]
    which = args.pop() if args and args[-1] in SETS else "golden"
    cores = list(HOST_TESTS) if not args or args == ["all"] else args
    for c in cores:
        if c not in HOST_TESTS:
            raise SystemExit("unknown core %r (%s, or all)" % (c, " ".join(HOST_TESTS)))
        report(c, which)
