"""Python mirror of the batched voice activity detector's C-ABI (include/asp_vad.h) over ctypes.
Plumbing only -- every call goes into libasp_amd.so; no CPU fallback."""
import ctypes as C

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST
from .ns import AspError, _check, _declare, load_library  # noqa: F401

_sig_done = False

_I16, _I32 = C.c_int16, C.c_int32


class AspVadState(C.Structure):
    """include/asp_vad.h: AspVadState (VadInstT field by field)."""

    _fields_ = [("vad", _I32), ("downsampling_filter_states", _I32 * 4), ("S_48_24", _I32 * 8),
                ("S_24_24", _I32 * 16), ("S_24_16", _I32 * 8), ("S_16_8", _I32 * 8),
                ("noise_means", _I16 * 12), ("speech_means", _I16 * 12), ("noise_stds", _I16 * 12),
                ("speech_stds", _I16 * 12), ("frame_counter", _I32), ("over_hang", _I16),
                ("num_of_speech", _I16), ("index_vector", _I16 * 96), ("low_value_vector", _I16 * 96),
                ("mean_value", _I16 * 6), ("upper_state", _I16 * 5), ("lower_state", _I16 * 5),
                ("hp_filter_state", _I16 * 4), ("over_hang_max_1", _I16 * 3), ("over_hang_max_2", _I16 * 3),
                ("individual", _I16 * 3), ("total", _I16 * 3), ("init_flag", _I32)]


def _lib():
    global _sig_done
    lib = load_library()
    if not _sig_done:
        vp, ip = C.c_void_p, C.c_int
        sig = {
            "AspVadBatch_Create": [C.POINTER(vp), ip, ip],
            "AspVadBatch_Free": [vp],
            "AspVadBatch_num_streams": [vp],
            "AspVadBatch_Init": [vp],
            "AspVadBatch_set_mode": [vp, ip],
            "AspVadBatch_InitStream": [vp, ip],
            "AspVadBatch_set_mode_stream": [vp, ip, ip],
            "AspVadBatch_Process": [vp, ip, ip, vp, ip, vp, vp, ip],
            "AspVadBatch_ExportState": [vp, ip, C.POINTER(AspVadState)],
            "AspVadBatch_ImportState": [vp, ip, C.POINTER(AspVadState)],
            "AspVadBatch_SetStream": [vp, vp],
            "AspVadBatch_Synchronize": [vp],
            "AspVadBatch_Features": [vp, vp, ip, vp, ip],
            "AspVad_debug_gaussian": [vp, vp, vp, ip, vp, vp, ip],
            "WebRtcVad_Create": [C.POINTER(vp)],
            "WebRtcVad_Init": [vp],
            "WebRtcVad_set_mode": [vp, ip],
            "WebRtcVad_Process": [vp, ip, vp, ip],
            "WebRtcVad_ValidRateAndFrameLength": [ip, ip],
        }
        _declare(lib, sig)
        lib.WebRtcVad_Free.argtypes = [vp]
        lib.WebRtcVad_Free.restype = None
        _sig_done = True
    return lib


class VadBatch:
    """N independent VAD streams on one GPU; Init (mode 0) on creation unless init=False."""

    def __init__(self, num_streams, device=0, mode=None, init=True):
        self.lib = _lib()
        self.S = int(num_streams)
        h = C.c_void_p()
        _check(self.lib.AspVadBatch_Create(C.byref(h), self.S, device), "AspVadBatch_Create")
        self.h = h
        if init:
            self.init()
        if mode is not None:
            self.set_mode(mode)

    def init(self):
        _check(self.lib.AspVadBatch_Init(self.h), "AspVadBatch_Init")

    def init_stream(self, s):
        _check(self.lib.AspVadBatch_InitStream(self.h, int(s)), "AspVadBatch_InitStream")

    def set_mode(self, mode):
        _check(self.lib.AspVadBatch_set_mode(self.h, int(mode)), "AspVadBatch_set_mode")

    def set_mode_stream(self, s, mode):
        _check(self.lib.AspVadBatch_set_mode_stream(self.h, int(s), int(mode)), "AspVadBatch_set_mode_stream")

    def process(self, fs, x):
        """x [F][S][L] int16 -> (decisions [F][S] int8, levels [F][S] int32)"""
        x = np.ascontiguousarray(x, np.int16)
        F, S, L = x.shape
        assert S == self.S
        dec = np.empty((F, S), np.int8)
        lev = np.empty((F, S), np.int32)
        _check(self.lib.AspVadBatch_Process(self.h, int(fs), L, x.ctypes.data, F, dec.ctypes.data, lev.ctypes.data,
                                            MEM_HOST), "AspVadBatch_Process")
        return dec, lev

    def process_device(self, fs, x, dec, lev=None):
        """torch tensors on the batch's device: x [F][S][L] int16, dec [F][S] int8, lev [F][S] int32 or None;
        asynchronous on the batch's stream"""
        F, S, L = x.shape
        _check(self.lib.AspVadBatch_Process(self.h, int(fs), int(L), x.data_ptr(), int(F), dec.data_ptr(),
                                            lev.data_ptr() if lev is not None else None, MEM_DEVICE),
               "AspVadBatch_Process")

    def features(self, x8):
        """x8 [S][80|160|240] int16 at 8 kHz -> [S][7] int16 (six features, total energy)"""
        x8 = np.ascontiguousarray(x8, np.int16)
        out = np.empty((self.S, 7), np.int16)
        _check(self.lib.AspVadBatch_Features(self.h, x8.ctypes.data, x8.shape[1], out.ctypes.data, MEM_HOST),
               "AspVadBatch_Features")
        return out

    def export_state(self, s):
        st = AspVadState()
        _check(self.lib.AspVadBatch_ExportState(self.h, int(s), C.byref(st)), "AspVadBatch_ExportState")
        return st

    def import_state(self, s, st):
        _check(self.lib.AspVadBatch_ImportState(self.h, int(s), C.byref(st)), "AspVadBatch_ImportState")

    def state_bytes(self):
        """every stream's AspVadState as [S][736] uint8"""
        out = np.empty((self.S, C.sizeof(AspVadState)), np.uint8)
        for s in range(self.S):
            st = self.export_state(s)   # held while its bytes are copied
            out[s] = np.frombuffer(bytes(st), np.uint8)
        return out

    def set_stream(self, hip_stream):
        _check(self.lib.AspVadBatch_SetStream(self.h, hip_stream), "AspVadBatch_SetStream")

    def synchronize(self):
        _check(self.lib.AspVadBatch_Synchronize(self.h), "AspVadBatch_Synchronize")

    def close(self):
        if getattr(self, "h", None):
            self.lib.AspVadBatch_Free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def debug_gaussian(inp, mean, std, device=0):
    """WebRtcVad_GaussianProbability on the device -> (probability int32, delta int16)"""
    lib = _lib()
    inp, mean, std = (np.ascontiguousarray(v, np.int16) for v in (inp, mean, std))
    n = inp.size
    p, d = np.empty(n, np.int32), np.empty(n, np.int16)
    _check(lib.AspVad_debug_gaussian(inp.ctypes.data, mean.ctypes.data, std.ctypes.data, n, p.ctypes.data,
                                     d.ctypes.data, device), "AspVad_debug_gaussian")
    return p, d
