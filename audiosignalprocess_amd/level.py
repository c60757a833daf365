"""Python mirror of the batched level estimator's C-ABI (include/asp_level.h) over ctypes.  Plumbing only -- every
call goes into libasp_amd.so; no CPU fallback.  Restate is the test-only CPU build of the same core (in
lib/libhpf_restate.so, beside the high-pass filter's)."""
import ctypes as C

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST  # noqa: F401
from .hpf import restate_library
from .ns import AspError, _check, _declare, device_count, load_library as _load  # noqa: F401

MAX_SAMPLES, MAX_CHANNELS, MIN_LEVEL = 480, 16, 127


class AspLevelState(C.Structure):
    _fields_ = [("sum_square", C.c_float), ("sample_count", C.c_int32)]

    def pair(self):
        """(the sum's 32 bits, the count)"""
        return int(np.float32(self.sum_square).view(np.uint32)), int(self.sample_count)


_sig_done = False


def load_library():
    """libasp_amd.so with argtypes / restype set on every level estimator entry point."""
    global _sig_done
    lib = _load()
    if not _sig_done:
        vp, ip = C.c_void_p, C.c_int
        _declare(lib, {
            "AspLevelBatch_Create": [C.POINTER(vp), ip, ip],
            "AspLevelBatch_Free": [vp],
            "AspLevelBatch_num_streams": [vp],
            "AspLevelBatch_Reset": [vp],
            "AspLevelBatch_ResetStream": [vp, ip],
            "AspLevelBatch_Process": [vp, vp, ip, ip, ip, ip],
            "AspLevelBatch_ProcessMuted": [vp, ip],
            "AspLevelBatch_ProcessMutedStream": [vp, ip, ip],
            "AspLevelBatch_RMS": [vp, vp],
            "AspLevelBatch_RMS_stream": [vp, ip, vp],
            "AspLevelBatch_ExportState": [vp, ip, vp],
            "AspLevelBatch_ImportState": [vp, ip, vp],
            "AspLevelBatch_SetStream": [vp, vp],
            "AspLevelBatch_Synchronize": [vp],
        })
        lib.AspLevel_state_size.argtypes = []
        lib.AspLevel_state_size.restype = C.c_size_t
        _sig_done = True
    return lib


class LevelBatch:
    """AspLevelBatch_*; audio is int16 [F][S][C][n] in host memory (numpy), or a device address through
    process_device."""

    def __init__(self, num_streams, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.AspLevelBatch_Create(C.byref(self.h), num_streams, device), "AspLevelBatch_Create")
        self.S = num_streams

    def close(self):
        if self.h:
            self.lib.AspLevelBatch_Free(self.h)
            self.h = C.c_void_p()

    def reset(self, stream=None):
        if stream is None:
            return self.lib.AspLevelBatch_Reset(self.h)
        return self.lib.AspLevelBatch_ResetStream(self.h, stream)

    def process(self, x):
        """x: int16 [F][S][C][n]."""
        assert x.dtype == np.int16 and x.shape[1] == self.S and x.flags.c_contiguous
        _check(self.lib.AspLevelBatch_Process(self.h, x.ctypes.data, x.shape[0], x.shape[2], x.shape[3], MEM_HOST),
               "AspLevelBatch_Process")

    def process_device(self, src, num_frames, num_channels, samples):
        _check(self.lib.AspLevelBatch_Process(self.h, src, num_frames, num_channels, samples, MEM_DEVICE),
               "AspLevelBatch_Process")

    def muted(self, length, stream=None):
        if stream is None:
            return self.lib.AspLevelBatch_ProcessMuted(self.h, length)
        return self.lib.AspLevelBatch_ProcessMutedStream(self.h, stream, length)

    def rms(self, stream=None):
        """RMS() of every stream (int32 [S]) or of one (int); resets what it read."""
        if stream is None:
            out = np.zeros(self.S, np.int32)
            _check(self.lib.AspLevelBatch_RMS(self.h, out.ctypes.data), "AspLevelBatch_RMS")
            return out
        v = C.c_int32()
        _check(self.lib.AspLevelBatch_RMS_stream(self.h, stream, C.addressof(v)), "AspLevelBatch_RMS_stream")
        return v.value

    def export_state(self, stream):
        st = AspLevelState()
        _check(self.lib.AspLevelBatch_ExportState(self.h, stream, C.addressof(st)), "AspLevelBatch_ExportState")
        return st

    def import_state(self, stream, st):
        return self.lib.AspLevelBatch_ImportState(self.h, stream, C.addressof(st))

    def synchronize(self):
        _check(self.lib.AspLevelBatch_Synchronize(self.h), "AspLevelBatch_Synchronize")


class Restate:
    """The CPU build of csrc/level_core.h, one stream (tests only)."""

    def __init__(self):
        self.L = restate_library()
        self.L.LevelRestate_State.restype = C.POINTER(AspLevelState)
        self.h = C.c_void_p(self.L.LevelRestate_Create())

    def __del__(self):
        if getattr(self, "h", None):
            self.L.LevelRestate_Free(self.h)
            self.h = None

    def reset(self):
        self.L.LevelRestate_Reset(self.h)

    def process(self, row):
        row = np.ascontiguousarray(row, np.int16).reshape(-1)
        self.L.LevelRestate_Process(self.h, row.ctypes.data, row.size)

    def muted(self, length):
        self.L.LevelRestate_ProcessMuted(self.h, length)

    def rms(self):
        return self.L.LevelRestate_RMS(self.h)

    def state(self):
        return self.L.LevelRestate_State(self.h).contents.pair()


def smoke_check(S=5, C_=2, F=4, n=480):
    """S streams x F frames of C_ channels on the GPU against the CPU build of the same core; True when the
    accumulators are bit-equal and RMS() agrees."""
    rng = np.random.default_rng(4)
    x = (rng.integers(-32768, 32768, (F, S, C_, n)) >> np.arange(S)[None, :, None, None]).astype(np.int16)
    b = LevelBatch(S)
    b.process(x)
    ok = b.muted(n, stream=1) == 0
    got = [b.export_state(s).pair() for s in range(S)]
    levels = b.rms()
    b.close()
    for s in range(S):
        cpu = Restate()
        cpu.process(x[:, s])
        if s == 1:
            cpu.muted(n)
        ok = ok and cpu.state() == got[s] and cpu.rms() == levels[s]
    return bool(ok)
