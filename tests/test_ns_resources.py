"""Register figures of the pair-layout NS frame kernel (ns_kernels1.hip), from the compiler's own resource remarks.

Four waves per SIMD need <= 128 VGPRs; the hand-off instantiations sit exactly there and hold it only with the
per-file flags of build.py (-disable-machine-licm) and the ns_cold() copies of the rarely taken paths
(profiles/README.md, "NS hand-off build", findings 5 and 9).  A spill or a 129th register costs a quarter of the
occupancy or puts scratch traffic into the step without failing any other test, so the figures are asserted here:
every ns_frame1_kernel instantiation at most 128 VGPRs, no spilled VGPR or SGPR, no scratch.  Needs hipcc, no GPU."""
import os
import re
import subprocess

import pytest

from audiosignalprocess_amd import build

MAX_VGPRS = 128
KEYS = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill"}


def resource_remarks(text):
    """{function name: {vgprs, scratch, sgpr_spill, vgpr_spill}} from -Rpass-analysis=kernel-resource-usage output."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\d+)\b", line)
        if m and cur is not None and m.group(1) in KEYS:
            cur[KEYS[m.group(1)]] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def ns1_resources(tmp_path_factory):
    src = os.path.join(build.CSRC, "ns_kernels1.hip")
    obj = str(tmp_path_factory.mktemp("ns1res") / "ns_kernels1.o")
    cmd = ([build.hipcc()] + build.FLAGS + build.EXTRA["ns_kernels1.hip"]
           + ["-I" + os.path.join(build.ROOT, "include"), "-I" + build.CSRC, "--cuda-device-only",
              "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return {k: v for k, v in resource_remarks(r.stdout).items() if "ns_frame1_kernel" in k}


def test_all_four_instantiations_report(ns1_resources):
    names = sorted(ns1_resources)
    assert len(names) == 4, names
    for io16 in "01":
        for flow in "01":
            assert any("ns_frame1_kernelILb%sELb%sE" % (io16, flow) in n for n in names), (io16, flow, names)
    for n, fig in ns1_resources.items():
        assert set(fig) == set(KEYS.values()), (n, fig)


def test_registers_fit_four_waves_per_simd_without_spills(ns1_resources):
    for n, fig in sorted(ns1_resources.items()):
        print(n, fig)
    for n, fig in ns1_resources.items():
        assert fig["vgprs"] <= MAX_VGPRS, (n, fig)
        assert fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0, (n, fig)
        assert fig["scratch"] == 0, (n, fig)
