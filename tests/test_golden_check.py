"""The committed NSX and AGC goldens are what the reference build gives today: both writers' --check mode regenerates
every array of nsx_golden.npz / agc_golden.npz and of the two edge goldens from oracle/_ref/ (built by build() where
the reference is present) and compares it with the file.  Skips where neither the reference build nor the reference
is present; a reference without its build (build() not run) is a failure."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("edges", [False, True], ids=["golden", "edges"])
@pytest.mark.parametrize("module", ["nsx", "agc"])
def test_writer_check_reproduces_the_committed_golden(module, edges):
    lib = os.path.join(ROOT, "oracle", "_ref", "lib%s_ref.so" % module)
    reference = os.path.join(os.environ.get("REF", "/root/reference"), "WebRtc_AMP_Port")   # oracle/Makefile's default
    assert os.path.exists(lib) or not os.path.isdir(reference), "the reference is present but %s is not built: run build()" % lib
    if not os.path.exists(lib):
        pytest.skip("oracle/_ref/lib%s_ref.so (the reference build) is absent" % module)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "golden", "make_%s_golden.py" % module), "--check"] + (["--edges"] if edges else [])
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert ", 0 differ" in r.stdout
