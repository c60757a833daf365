"""The list entry points of the BT batch (AspBtBatch_DenoiseList / AspBtBatch_FlushList) exist in all three places a
caller meets them: exported by libasp_amd.so, declared in include/asp_bt.h with the documented signatures, and declared
by the Python mirror.  Needs the built library, no GPU."""
import ctypes as C
import os
import re

from audiosignalprocess_amd import bt
from audiosignalprocess_amd.build import ROOT

NAMES = ("AspBtBatch_DenoiseList", "AspBtBatch_FlushList")
SIGNATURES = {
    "AspBtBatch_DenoiseList":
        "int AspBtBatch_DenoiseList(AspBtBatch* b, const int32_t* streams, const int32_t* counts, int n, "
        "const float* in, float* out, int max_blocks, int mem);",
    "AspBtBatch_FlushList":
        "int AspBtBatch_FlushList(AspBtBatch* b, const int32_t* streams, const int32_t* hops, int n, "
        "const float* in, float* out, int max_hops, int mem);",
}


def test_library_exports_both_symbols(built_lib):
    lib = C.CDLL(built_lib)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_header_declares_both_with_the_documented_signatures():
    text = open(os.path.join(ROOT, "include", "asp_bt.h")).read()
    flat = re.sub(r"\s+", " ", text)
    for name, sig in SIGNATURES.items():
        assert sig in flat, name
    # the contract's comment sits above the two declarations and says what a flush entry with no hop does
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", text))  # (without the comment's leading asterisks)
    comment = flat[flat.index("Macroblocks of SOME stream-channels"):flat.index(SIGNATURES[NAMES[0]][:40])]
    assert "hops == 0 consumes the tail" in comment
    assert "do not list it" in comment
    assert "ring of 8 slots" in comment


def test_python_mirror_declares_both(built_lib):
    lib = bt._lib()
    vp, ip = C.c_void_p, C.c_int
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.argtypes == [vp, vp, vp, ip, vp, vp, ip, ip], name
        assert fn.restype == C.c_int, name
    for method in ("denoise_list", "denoise_list_device", "flush_list", "flush_list_device"):
        assert callable(getattr(bt.BtBatch, method)), method
