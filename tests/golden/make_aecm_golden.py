"""Writes tests/golden/aecm_golden.npz from the reference AECM compiled in place:

    python tests/golden/make_aecm_golden.py <libaecmref.so>

Each run drives WebRtcAecm_Create / Init / set_config / BufferFarend / Process through ctypes on inputs
from synth.aecm_pair, following the schedule of aecm_runs.RUNS (delay jitter, out-of-range delays, delay
jumps, Process without BufferFarend, InitEchoPath / set_config / re-Init mid-run, extreme inputs).  The
golden stores no audio input, only the synth arguments and a sha256 of the regenerated input, and per
frame: the output, the return value and the error code.
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.aecm_runs import RUNS, inputs, schedule  # noqa: E402


class AecmConfig(ctypes.Structure):
    _fields_ = [("cngMode", ctypes.c_int16), ("echoMode", ctypes.c_int16)]


def bind(path):
    L = ctypes.CDLL(path)
    P, I16P = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int16)
    L.WebRtcAecm_Create.argtypes = [ctypes.POINTER(P)]
    L.WebRtcAecm_Free.argtypes = [P]
    L.WebRtcAecm_Init.argtypes = [P, ctypes.c_int32]
    L.WebRtcAecm_BufferFarend.argtypes = [P, I16P, ctypes.c_int16]
    L.WebRtcAecm_Process.argtypes = [P, I16P, I16P, I16P, ctypes.c_int16, ctypes.c_int16]
    L.WebRtcAecm_set_config.argtypes = [P, AecmConfig]
    L.WebRtcAecm_InitEchoPath.argtypes = [P, ctypes.c_void_p, ctypes.c_size_t]
    L.WebRtcAecm_get_error_code.argtypes = [P]
    return L


def run_reference(L, spec):
    far, near, clean = inputs(spec)
    F, n = far.shape[0], far.shape[1]
    h = ctypes.c_void_p()
    assert L.WebRtcAecm_Create(ctypes.byref(h)) == 0
    out = np.zeros((F, n), np.int16)
    ret = np.zeros(F, np.int32)
    err = np.zeros(F, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))
    for f, ev in enumerate(schedule(spec)):
        if ev.get("init"):
            L.WebRtcAecm_Init(h, ev["init"])
        if ev.get("config"):
            L.WebRtcAecm_set_config(h, AecmConfig(*ev["config"]))
        if ev.get("echo_path") is not None:
            p = np.ascontiguousarray(ev["echo_path"], np.int16)
            L.WebRtcAecm_InitEchoPath(h, p.ctypes.data, 130)
        if ev["far"]:
            L.WebRtcAecm_BufferFarend(h, ptr(far[f]), n)
        o = out[f]
        c = ptr(clean[f]) if spec["clean"] else None
        ret[f] = L.WebRtcAecm_Process(h, ptr(near[f]), c, ptr(o), n, ev["ms"])
        err[f] = L.WebRtcAecm_get_error_code(h)
    L.WebRtcAecm_Free(h)
    return out, ret, err


def main():
    L = bind(sys.argv[1])
    data = {}
    for i, spec in enumerate(RUNS):
        far, near, clean = inputs(spec)
        out, ret, err = run_reference(L, spec)
        data["r%d_sha" % i] = np.frombuffer(hashlib.sha256(far.tobytes() + near.tobytes() + clean.tobytes()).digest(), np.uint8)
        data["r%d_out" % i] = out
        data["r%d_ret" % i] = ret
        data["r%d_err" % i] = err
    np.savez_compressed(os.path.join(HERE, "aecm_golden.npz"), **data)


if __name__ == "__main__":
    main()
