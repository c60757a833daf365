"""The golden and edge runs together take every line and branch of csrc/nsx_core.h and csrc/agc_core.h, except what
tests/core_branch_exemptions.py lists with its reason.  Builds each core with g++ --coverage -O0, replays
tests/test_<core>_host.py against it and reads gcov (tools/core_branch_report.py).  CPU only; a missing g++ or gcov is
a failure, not a skip."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import core_branch_report  # noqa: E402

from tests.core_branch_exemptions import CLASSES, EXEMPT, NEVER  # noqa: E402


@pytest.mark.parametrize("core", ["nsx", "agc"])
def test_every_untaken_branch_is_listed_and_every_listed_one_is_untaken(core):
    rows, (lines, lines_run, branches, taken) = core_branch_report.measure(core, "both")
    listed = EXEMPT[core]
    untaken = {}
    for func, line, kind, branch, source in rows:
        if any(match(func, source) for match in CLASSES.values()):
            continue
        untaken[(line, branch if kind == "branch" else None)] = (func, source)
    missing = sorted(k for k in untaken if k not in listed)
    assert not missing, "untaken and not on the exemption list of %s: %r" % (
        core, [(k, untaken[k][0], untaken[k][1][:60]) for k in missing])
    stale = sorted(k for k in listed if k not in untaken)
    assert not stale, "listed for %s but taken by the runs: %r" % (core, stale)
    assert all(len(reason) > 12 and reason.endswith(".") for reason in listed.values())   # a sentence each
    assert not [k for k in listed if k[0] in NEVER[core]]
    print("%s_core.h: %d of %d lines executed, %d of %d branches taken" % (core, lines_run, lines, taken, branches))


def test_the_two_classes_match_what_they_name():
    assert CLASSES["lane"]("f", "if (L.id == 0) {") and CLASSES["lane"]("f", "if (g.is(0)) s.x = 1;") and CLASSES["lane"]("f", "if (write) env[k] = m;")
    assert not CLASSES["lane"]("f", "if (zeros < 9) {")
    assert CLASSES["div"]("div_w32w16", "if (den == 0) return 0x7FFFFFFF;") and not CLASSES["div"]("div_w32w16", "if (den == -1) return 0;")
    assert not CLASSES["div"]("process_core", "x = den != 0 ? a / den : 0;")
