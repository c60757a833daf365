"""Register figures of the list kernels of the pair-layout NS frame step (ns_kernels1.hip, ns_list1_kernel), from the
compiler's own resource remarks: they hold the budget of the product kernels (tests/test_ns_resources.py) -- at most 128
VGPRs for four waves per SIMD, no spilled VGPR or SGPR, no scratch.  Needs hipcc, no GPU."""
import os
import subprocess

import pytest

from audiosignalprocess_amd import build
from tests.test_ns_resources import KEYS, MAX_VGPRS, resource_remarks


@pytest.fixture(scope="module")
def list_resources(tmp_path_factory):
    src = os.path.join(build.CSRC, "ns_kernels1.hip")
    obj = str(tmp_path_factory.mktemp("ns1list") / "ns_kernels1.o")
    cmd = ([build.hipcc()] + build.FLAGS + build.EXTRA["ns_kernels1.hip"]
           + ["-I" + os.path.join(build.ROOT, "include"), "-I" + build.CSRC, "--cuda-device-only",
              "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return {k: v for k, v in resource_remarks(r.stdout).items() if "ns_list1_kernel" in k}


def test_both_list_kernels_report(list_resources):
    names = sorted(list_resources)
    assert len(names) == 2, names
    for io16 in "01":
        assert any("ns_list1_kernelILb%sE" % io16 in n for n in names), (io16, names)
    for n, fig in list_resources.items():
        assert "ns_frame1_kernel" not in n, n  # (test_ns_resources.py counts exactly four of those)
        assert set(fig) == set(KEYS.values()), (n, fig)


def test_list_kernels_hold_the_product_budget(list_resources):
    assert list_resources
    for n, fig in sorted(list_resources.items()):
        print(n, fig)
        assert fig["vgprs"] <= MAX_VGPRS, (n, fig)
        assert fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0, (n, fig)
        assert fig["scratch"] == 0, (n, fig)
