"""The product kernels of ns_kernels1.hip carry no diagnostics: the listing of the product build (compiled as
tests/test_ns_resources.py compiles it) reads no clock -- neither the shader clock nor the real-time counter of the
phase stamps -- in any ns_frame1_kernel instantiation (DIAG = false); the stamps live in ns_frame1_diag_kernel only.

The diagnostic kernels (DIAG = true) are held to the resource rule of the product kernels -- at most 128 VGPRs, no
spilled VGPR or SGPR, no scratch, so four waves per SIMD and no scratch traffic inside the step they time.
tests/test_ns_resources.py selects functions by "ns_frame1_kernel" and so does not see them; the same assertions are
made here for every ns_frame1 function of the file.  Needs hipcc, no GPU."""
import os
import re
import subprocess

import pytest

from audiosignalprocess_amd import build

from tests.test_ns_resources import MAX_VGPRS, resource_remarks

CLOCKS = ("s_memtime", "s_memrealtime")


@pytest.fixture(scope="module")
def ns1_functions(tmp_path_factory):
    """{function name: its instructions} of the gfx950 listing of ns_kernels1.hip"""
    src = os.path.join(build.CSRC, "ns_kernels1.hip")
    asm = str(tmp_path_factory.mktemp("ns1asm") / "ns_kernels1.s")
    cmd = ([build.hipcc()] + build.FLAGS + build.EXTRA["ns_kernels1.hip"]
           + ["-I" + os.path.join(build.ROOT, "include"), "-I" + build.CSRC, "--cuda-device-only", "-S", src, "-o", asm])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    out, cur = {}, None
    for line in open(asm):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line.startswith("\t") and not line.lstrip().startswith((";", ".")):
            cur.append(line.split()[0])
    return out


def test_product_instantiations_read_no_clock(ns1_functions):
    product = {n: ops for n, ops in ns1_functions.items() if "ns_frame1_kernel" in n}
    assert len(product) == 4, sorted(product)
    for n, ops in product.items():
        assert len(ops) > 1000, (n, len(ops))
        assert not [op for op in ops if op.startswith(CLOCKS)], n


def test_diagnostic_instantiations_hold_the_stamps(ns1_functions):
    diag = {n: ops for n, ops in ns1_functions.items() if "ns_frame1_diag_kernel" in n}
    assert len(diag) == 2, sorted(diag)   # plain and hand-off, float frames: what the stamp entry points launch
    for n, ops in diag.items():
        assert [op for op in ops if op.startswith(CLOCKS)], n


@pytest.fixture(scope="module")
def ns1_all_resources(tmp_path_factory):
    src = os.path.join(build.CSRC, "ns_kernels1.hip")
    obj = str(tmp_path_factory.mktemp("ns1res_all") / "ns_kernels1.o")
    cmd = ([build.hipcc()] + build.FLAGS + build.EXTRA["ns_kernels1.hip"]
           + ["-I" + os.path.join(build.ROOT, "include"), "-I" + build.CSRC, "--cuda-device-only",
              "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return {k: v for k, v in resource_remarks(r.stdout).items() if "ns_frame1_" in k}


def test_diagnostic_kernels_keep_the_resource_rule_of_the_product_kernels(ns1_all_resources):
    diag = {n: f for n, f in ns1_all_resources.items() if "ns_frame1_diag_kernel" in n}
    assert len(diag) == 2 and len(ns1_all_resources) == 6, sorted(ns1_all_resources)
    for n, fig in sorted(ns1_all_resources.items()):
        print(n, fig)
        assert fig["vgprs"] <= MAX_VGPRS, (n, fig)
        assert fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0, (n, fig)
        assert fig["scratch"] == 0, (n, fig)
