"""Python mirror of the batched fixed-point resampler's C-ABI (include/asp_resampler.h) over ctypes.
Plumbing only -- every call goes into libasp_amd.so; no CPU fallback.  Restate is the test-only CPU build
of the same core (lib/libsplrs_restate.so), one channel per instance."""
import ctypes as C
import os

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST  # noqa: F401
from .build import LIBDIR
from .ns import AspError, _check, _declare, device_count, load_library as _load  # noqa: F401

MODES = ["1To1", "1To2", "1To3", "1To4", "1To6", "1To12", "2To3", "2To11", "4To11", "8To11", "11To16", "11To32",
         "2To1", "3To1", "4To1", "6To1", "12To1", "3To2", "11To2", "11To4", "11To8"]


class AspResamplerState(C.Structure):
    _fields_ = [("mode", C.c_int32), ("in_freq_khz", C.c_int32), ("out_freq_khz", C.c_int32),
                ("stage", (C.c_int32 * 32) * 3)]

    def stages(self):
        """The three stage states as an int32 array [3][32]."""
        return np.array(self.stage, np.int32).reshape(3, 32)


_sig_done = False


def load_library():
    """libasp_amd.so with argtypes / restype set on every resampler entry point."""
    global _sig_done
    lib = _load()
    if not _sig_done:
        vp, ip = C.c_void_p, C.c_int
        _declare(lib, {
            "AspResamplerBatch_Create": [C.POINTER(vp), ip, ip],
            "AspResamplerBatch_Free": [vp],
            "AspResamplerBatch_num_streams": [vp],
            "AspResamplerBatch_Reset": [vp, ip, ip, ip],
            "AspResamplerBatch_ResetIfNeeded": [vp, ip, ip, ip],
            "AspResamplerBatch_ResetStream": [vp, ip],
            "AspResamplerBatch_OutLength": [vp, ip],
            "AspResamplerBatch_Push": [vp, vp, ip, vp, ip, C.POINTER(ip), ip],
            "AspResamplerBatch_PushFrames": [vp, vp, ip, ip, vp, ip],
            "AspResamplerBatch_ExportState": [vp, ip, ip, vp],
            "AspResamplerBatch_ImportState": [vp, ip, ip, vp],
            "AspResamplerBatch_SetStream": [vp, vp],
            "AspResamplerBatch_Synchronize": [vp],
        })
        lib.AspResampler_state_size.argtypes = []
        lib.AspResampler_state_size.restype = C.c_size_t
        _sig_done = True
    return lib


class ResamplerBatch:
    """AspResamplerBatch_* on host arrays.  Reset / push return the reference's 0 / -1; any other failure raises."""

    def __init__(self, num_streams, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.AspResamplerBatch_Create(C.byref(self.h), num_streams, device), "AspResamplerBatch_Create")
        self.S = num_streams

    def close(self):
        if self.h:
            self.lib.AspResamplerBatch_Free(self.h)
            self.h = C.c_void_p()

    def reset(self, in_freq, out_freq, channels=1):
        return self.lib.AspResamplerBatch_Reset(self.h, in_freq, out_freq, channels)

    def reset_if_needed(self, in_freq, out_freq, channels=1):
        return self.lib.AspResamplerBatch_ResetIfNeeded(self.h, in_freq, out_freq, channels)

    def reset_stream(self, stream):
        _check(self.lib.AspResamplerBatch_ResetStream(self.h, stream), "AspResamplerBatch_ResetStream")

    def out_length(self, length_in):
        return self.lib.AspResamplerBatch_OutLength(self.h, length_in)

    def push(self, x, max_len=None):
        """x: int16 [S][length_in].  Returns (rc, out [S][out_len]); rc = -1 is the reference's refusal (out None)."""
        S, n = x.shape
        assert S == self.S and x.dtype == np.int16 and x.flags.c_contiguous
        if max_len is None:
            max_len = max(self.out_length(n), 0)
        y = np.zeros((S, max(max_len, 1)), np.int16)
        k = C.c_int(0)
        rc = self.lib.AspResamplerBatch_Push(self.h, x.ctypes.data, n, y.ctypes.data, max_len, C.byref(k), MEM_HOST)
        if rc == -1:
            return rc, None
        _check(rc, "AspResamplerBatch_Push")
        return 0, np.ascontiguousarray(y.reshape(-1)[:S * k.value].reshape(S, k.value))

    def push_frames(self, x):
        """x: int16 [F][S][length_in] -> [F][S][out_len]."""
        F, S, n = x.shape
        assert S == self.S and x.dtype == np.int16 and x.flags.c_contiguous
        m = self.out_length(n)
        if m < 0:
            raise AspError("AspResamplerBatch_PushFrames: the reference rejects length %d in this mode" % n)
        y = np.zeros((F, S, m), np.int16)
        _check(self.lib.AspResamplerBatch_PushFrames(self.h, x.ctypes.data, n, F, y.ctypes.data, MEM_HOST),
               "AspResamplerBatch_PushFrames")
        return y

    def export_state(self, stream, channel=0):
        st = AspResamplerState()
        _check(self.lib.AspResamplerBatch_ExportState(self.h, stream, channel, C.addressof(st)),
               "AspResamplerBatch_ExportState")
        return st

    def import_state(self, stream, st, channel=0):
        return self.lib.AspResamplerBatch_ImportState(self.h, stream, channel, C.addressof(st))


class Restate:
    """The CPU build of csrc/splrs_core.h, one channel (tests only)."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = C.CDLL(os.path.join(LIBDIR, "libsplrs_restate.so"))
            L.SplrsRestate_Create.restype = C.c_void_p
            L.SplrsRestate_Free.argtypes = [C.c_void_p]
            L.SplrsRestate_Reset.argtypes = [C.c_void_p, C.c_int, C.c_int]
            L.SplrsRestate_Push.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
            L.SplrsRestate_State.argtypes = [C.c_void_p]
            L.SplrsRestate_State.restype = C.POINTER(AspResamplerState)
            cls._lib = L
        return cls._lib

    def __init__(self, in_freq=None, out_freq=None):
        self.L = self.lib()
        self.h = C.c_void_p(self.L.SplrsRestate_Create())
        if in_freq is not None:
            self.reset(in_freq, out_freq)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.SplrsRestate_Free(self.h)
            self.h = None

    def reset(self, in_freq, out_freq):
        return self.L.SplrsRestate_Reset(self.h, in_freq, out_freq)

    def push(self, x, max_len=None):
        """x: int16 [length_in].  Returns (rc, out)."""
        x = np.ascontiguousarray(x, np.int16)
        if max_len is None:
            max_len = 12 * x.size
        y = np.zeros(max(max_len, 1), np.int16)
        k = C.c_int(0)
        rc = self.L.SplrsRestate_Push(self.h, x.ctypes.data, x.size, y.ctypes.data, max_len, C.byref(k))
        return (rc, None) if rc else (0, y[:k.value].copy())

    @property
    def state(self):
        return self.L.SplrsRestate_State(self.h).contents
