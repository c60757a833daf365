"""CPU suite: the planning step of the AEC list calls (csrc/aec_control.h, plan_list) as a stand-alone, sanitized host
program.

tests/host/aec_list_control_check.cpp includes the control plane, plans the ragged schedule of tests/aec_list_cases.py
(and the same schedule with every count times five, so that calls are cut into launches) the way AspAecBatch_RunList
does, and checks every descriptor against the bounds aec_list_kernel relies on: ring indices, far-ring slots, at most
three far partitions, two sub-frames, two blocks.  Built with AddressSanitizer and UndefinedBehaviorSanitizer, the
runtimes linked in statically, and run as a child process in the caller's environment as it is."""
import os
import subprocess

from tests.aec_list_cases import DELAYS, S, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_planning_under_sanitizers(tmp_path):
    sched = tmp_path / "schedule.txt"
    with open(sched, "w") as f:
        f.write("%d\n%s\n" % (S, " ".join(str(d) for d in DELAYS)))
        for st, ct in schedule():
            f.write("%d %s\n" % (len(st), " ".join("%d %d" % (s, c) for s, c in zip(st, ct))))
    exe = str(tmp_path / "aec_list_control_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "audiosignalprocess_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "aec_list_control_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe, str(sched)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stderr == ""
    assert "all bounds held" in r.stdout and len(r.stdout.strip().splitlines()) == 1
