"""The list entry point of the AEC batch (AspAecBatch_RunList) exists in all three places a caller meets it: exported
by libasp_amd.so, declared in include/asp_aec.h with the documented signature and the figures a caller sizes memory by,
and declared by the Python mirror; and a control-only handle answers the documented codes.  Needs the built library,
no GPU."""
import ctypes as C
import os
import re

import numpy as np

from audiosignalprocess_amd import aec
from audiosignalprocess_amd.build import ROOT
from tests.aec_list_cases import control_lib, control_only, run_list_control

SIGNATURE = ("int AspAecBatch_RunList(AspAecBatch* b, const int32_t* streams, const int32_t* counts, int n, "
             "const float* farend, const float* nearend, float* out, int nrOfSamples, int max_frames, "
             "const int16_t* msInSndCardBuf /* [n] */, int32_t* status /* [n], may be null */, int mem);")


def test_library_exports_the_symbol(built_lib):
    assert hasattr(C.CDLL(built_lib), "AspAecBatch_RunList")


def test_header_declares_it_with_the_documented_signature_and_figures():
    text = open(os.path.join(ROOT, "include", "asp_aec.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert SIGNATURE in flat
    doc = text[text.index("BufferFarend + Process of SOME streams"):text.index("int AspAecBatch_RunList")]
    assert re.search(r"#define ASP_AEC_LIST_MAX_FRAMES 8\b", doc) and re.search(r"#define ASP_AEC_LIST_SLOTS 4\b", doc)
    for word in ("BLOCKS", "ASP_ERR_PARAM", "ASP_ERR_STATE", "first list call", "control-only"):
        assert word in doc, word


def test_python_mirror_declares_it(built_lib):
    lib = aec._lib()
    vp, ip = C.c_void_p, C.c_int
    fn = lib.AspAecBatch_RunList
    assert fn.argtypes == [vp, vp, vp, ip, vp, vp, vp, ip, ip, vp, vp, ip]
    assert fn.restype == C.c_int
    assert callable(aec.AecBatch.run_list) and callable(aec.AecBatch.run_list_device)


def test_control_only_handle_answers_the_documented_codes(built_lib):
    lib = control_lib()
    h = control_only(lib, 16000, 0, streams=4)
    status = np.full(2, 9, np.int32)
    assert run_list_control(lib, h, [3, 1], [2, 1], 160, [0, 501], status=status) == -1   # as ProcessV: any -1
    assert status.tolist() == [0, -1]
    assert run_list_control(lib, h, [3, 1], [2, 1], 80, [0, 0]) == 0                       # both call sizes
    assert run_list_control(lib, h, [], [], 160, []) == 0                                  # ASP_OK: empty
    assert run_list_control(lib, h, [1, 1], [1, 1], 160, [0, 0]) == -1                     # ASP_ERR_PARAM
    assert run_list_control(lib, h, [4], [1], 160, [0]) == -1
    assert run_list_control(lib, h, [0], [2], 160, [0], max_frames=1) == -1
    assert b"listed twice" not in lib.AspNs_last_error() and b"count" in lib.AspNs_last_error()
    assert lib.AspAecBatch_Init(h, 32000, 48000) == 0
    assert run_list_control(lib, h, [0], [1], 160, [0]) == -4                              # ASP_ERR_STATE: 32 kHz
    assert b"per-stream control" in lib.AspNs_last_error()
    assert lib.AspAecBatch_Free(h) == 0
