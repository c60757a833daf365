"""The list entry points of the NS batch (AspNsBatch_AnalyzeProcessList / ...ListS16) exist in all three places a
caller meets them: exported by libasp_amd.so, declared in include/asp_ns.h with the documented signatures, and declared
by the Python mirror.  Needs the built library, no GPU."""
import ctypes as C
import os
import re

from audiosignalprocess_amd import ns
from audiosignalprocess_amd.build import ROOT

NAMES = ("AspNsBatch_AnalyzeProcessList", "AspNsBatch_AnalyzeProcessListS16")
SIGNATURES = {
    "AspNsBatch_AnalyzeProcessList":
        "int AspNsBatch_AnalyzeProcessList(AspNsBatch* b, const int32_t* streams, const int32_t* counts, int n, "
        "const float* in, float* out, int max_frames, int mem);",
    "AspNsBatch_AnalyzeProcessListS16":
        "int AspNsBatch_AnalyzeProcessListS16(AspNsBatch* b, const int32_t* streams, const int32_t* counts, int n, "
        "const int16_t* in, int16_t* out, int max_frames, int mem);",
}


def test_library_exports_both_symbols(built_lib):
    lib = C.CDLL(built_lib)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_header_declares_both_with_the_documented_signatures():
    text = open(os.path.join(ROOT, "include", "asp_ns.h")).read()
    flat = re.sub(r"\s+", " ", text)
    for name, sig in SIGNATURES.items():
        assert sig in flat, name
    assert "16 kHz" in text[text.index("Fused Analyze+Process of SOME streams"):text.index(SIGNATURES[NAMES[0]][:40])]


def test_python_mirror_declares_both(built_lib):
    lib = ns.load_library()
    vp, ip = C.c_void_p, C.c_int
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn.argtypes == [vp, vp, vp, ip, vp, vp, ip, ip], name
        assert fn.restype == C.c_int, name
    assert callable(ns.NsBatch.analyze_process_list) and callable(ns.NsBatch.analyze_process_list_device)
