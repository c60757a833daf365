"""Python mirror of the batched mobile echo canceller's C-ABI (include/asp_aecm.h) over ctypes.
Plumbing only -- every call goes into libasp_amd.so; no CPU fallback."""
import ctypes as C

import numpy as np

from ._abi import MEM_HOST
from .ns import AspError, _check, _declare, device_count, load_library as _load  # noqa: F401

AECM_UNINITIALIZED_ERROR = 12002
AECM_NULL_POINTER_ERROR = 12003
AECM_BAD_PARAMETER_ERROR = 12004
AECM_BAD_PARAMETER_WARNING = 12100

_sig_done = False


class AecmConfig(C.Structure):
    _fields_ = [("cngMode", C.c_int16), ("echoMode", C.c_int16)]


def _state_size():
    lib = _load()
    lib.AspAecm_state_size.restype = C.c_size_t
    return lib.AspAecm_state_size()


def load_library():
    """libasp_amd.so with argtypes / restype set on every AECM entry point."""
    global _sig_done, AspAecmStateBytes
    lib = _load()
    if not _sig_done:
        vp, ip, i16, sz = C.c_void_p, C.c_int, C.c_int16, C.c_size_t
        sig = {
            "AspAecmBatch_Create": [C.POINTER(vp), ip, ip],
            "AspAecmBatch_Free": [vp],
            "AspAecmBatch_num_streams": [vp],
            "AspAecmBatch_Init": [vp, C.c_int32],
            "AspAecmBatch_InitStream": [vp, ip, C.c_int32],
            "AspAecmBatch_set_config": [vp, AecmConfig],
            "AspAecmBatch_set_config_stream": [vp, ip, AecmConfig],
            "AspAecmBatch_InitEchoPath_stream": [vp, ip, vp],
            "AspAecmBatch_GetEchoPath_stream": [vp, ip, vp],
            "AspAecmBatch_BufferFarend": [vp, vp, ip, ip],
            "AspAecmBatch_Process": [vp, vp, vp, vp, ip, i16, ip],
            "AspAecmBatch_ProcessV": [vp, vp, vp, vp, ip, vp, ip],
            "AspAecmBatch_ProcessFrames": [vp, ip, vp, vp, vp, vp, ip, vp, vp, ip],
            "AspAecmBatch_get_error_code": [vp, ip],
            "AspAecmBatch_ExportState": [vp, ip, vp],
            "AspAecmBatch_ImportState": [vp, ip, vp],
            "AspAecmBatch_SetStream": [vp, vp],
            "AspAecmBatch_Synchronize": [vp],
            "WebRtcAecm_Create": [C.POINTER(vp)],
            "WebRtcAecm_Free": [vp],
            "WebRtcAecm_Init": [vp, C.c_int32],
            "WebRtcAecm_BufferFarend": [vp, vp, i16],
            "WebRtcAecm_Process": [vp, vp, vp, vp, i16, i16],
            "WebRtcAecm_set_config": [vp, AecmConfig],
            "WebRtcAecm_get_config": [vp, C.POINTER(AecmConfig)],
            "WebRtcAecm_InitEchoPath": [vp, vp, sz],
            "WebRtcAecm_GetEchoPath": [vp, vp, sz],
            "WebRtcAecm_get_error_code": [vp],
        }
        _declare(lib, sig)
        lib.WebRtcAecm_echo_path_size_bytes.argtypes = []
        lib.WebRtcAecm_echo_path_size_bytes.restype = sz
        lib.AspAecm_state_size.argtypes = []
        lib.AspAecm_state_size.restype = sz
        _sig_done = True
    return lib


AspAecmStateBytes = C.c_uint8 * _state_size()  # AspAecmState, opaque bytes


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class AecmBatch:
    """num_streams independent echo cancellers; host numpy buffers (ASP_MEM_HOST)."""

    def __init__(self, num_streams, fs=None, device=0):
        self.lib = load_library()
        self.S = num_streams
        h = C.c_void_p()
        _check(self.lib.AspAecmBatch_Create(C.byref(h), num_streams, device), "AspAecmBatch_Create")
        self.h = h
        if fs is not None:
            self.init(fs)

    def init(self, fs):
        _check(self.lib.AspAecmBatch_Init(self.h, fs), "Init")

    def init_stream(self, s, fs):
        _check(self.lib.AspAecmBatch_InitStream(self.h, s, fs), "InitStream")

    def set_config(self, cng=1, echo=3, stream=None):
        cfg = AecmConfig(cng, echo)
        if stream is None:
            return self.lib.AspAecmBatch_set_config(self.h, cfg)
        return self.lib.AspAecmBatch_set_config_stream(self.h, stream, cfg)

    def init_echo_path(self, s, path):
        p = np.ascontiguousarray(path, np.int16)
        _check(self.lib.AspAecmBatch_InitEchoPath_stream(self.h, s, _p(p)), "InitEchoPath")

    def get_echo_path(self, s):
        p = np.zeros(65, np.int16)
        _check(self.lib.AspAecmBatch_GetEchoPath_stream(self.h, s, _p(p)), "GetEchoPath")
        return p

    def process_frames(self, far, near, clean, ms):
        """far (or None) / near / clean (or None): [F][S][n] int16; ms [F][S] -> out [F][S][n], ret [F][S]."""
        near = np.ascontiguousarray(near, np.int16)
        F, S, n = near.shape
        far = None if far is None else np.ascontiguousarray(far, np.int16)
        clean = None if clean is None else np.ascontiguousarray(clean, np.int16)
        ms = np.ascontiguousarray(np.broadcast_to(np.asarray(ms, np.int16), (F, S)))
        out = np.zeros((F, S, n), np.int16)
        ret = np.zeros((F, S), np.int32)
        _check(self.lib.AspAecmBatch_ProcessFrames(self.h, F, _p(far), _p(near), _p(clean), _p(out), n, _p(ms),
                                                   _p(ret), MEM_HOST), "ProcessFrames")
        return out, ret

    def error_code(self, s):
        return self.lib.AspAecmBatch_get_error_code(self.h, s)

    def export_state(self, s):
        b = np.zeros(_state_size(), np.uint8)
        _check(self.lib.AspAecmBatch_ExportState(self.h, s, _p(b)), "ExportState")
        return b

    def import_state(self, s, b):
        b = np.ascontiguousarray(b, np.uint8)
        _check(self.lib.AspAecmBatch_ImportState(self.h, s, _p(b)), "ImportState")

    def close(self):
        if self.h:
            self.lib.AspAecmBatch_Free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["AecmBatch", "AecmConfig", "load_library", "device_count"]
