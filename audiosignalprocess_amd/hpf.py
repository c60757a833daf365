"""Python mirror of the batched high-pass filter's C-ABI (include/asp_hpf.h) over ctypes.  Plumbing only -- every
call goes into libasp_amd.so; no CPU fallback.  Restate is the test-only CPU build of the same core
(lib/libhpf_restate.so)."""
import ctypes as C
import os

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST  # noqa: F401
from .build import LIBDIR
from .ns import AspError, _check, _declare, device_count, load_library as _load  # noqa: F401

MAX_SAMPLES = 160


class AspHpfState(C.Structure):
    _fields_ = [("y", C.c_int16 * 4), ("x", C.c_int16 * 2), ("coeff_set", C.c_int16), ("reserved", C.c_int16)]

    def words(self):
        """y[0..3], x[0..1] as int16 [6]."""
        return np.array(list(self.y) + list(self.x), np.int16)


_sig_done = False


def load_library():
    """libasp_amd.so with argtypes / restype set on every high-pass filter entry point."""
    global _sig_done
    lib = _load()
    if not _sig_done:
        vp, ip = C.c_void_p, C.c_int
        _declare(lib, {
            "AspHpfBatch_Create": [C.POINTER(vp), ip, ip, ip],
            "AspHpfBatch_Free": [vp],
            "AspHpfBatch_num_streams": [vp],
            "AspHpfBatch_num_channels": [vp],
            "AspHpfBatch_Init": [vp, ip],
            "AspHpfBatch_InitStream": [vp, ip, ip],
            "AspHpfBatch_Process": [vp, vp, vp, ip, ip, ip],
            "AspHpfBatch_ProcessFloatS16": [vp, vp, vp, ip, ip, ip],
            "AspHpfBatch_ExportState": [vp, ip, ip, vp],
            "AspHpfBatch_ImportState": [vp, ip, ip, vp],
            "AspHpfBatch_SetStream": [vp, vp],
            "AspHpfBatch_Synchronize": [vp],
            "AspHpf_Create": [C.POINTER(vp)],
            "AspHpf_Init": [vp, ip],
            "AspHpf_Process": [vp, vp, ip],
            "AspHpf_Free": [vp],
        })
        lib.AspHpf_state_size.argtypes = []
        lib.AspHpf_state_size.restype = C.c_size_t
        _sig_done = True
    return lib


class HpfBatch:
    """AspHpfBatch_*; audio is int16 (or FloatS16 float32) [F][S][C][n] in host memory (numpy), or device addresses
    through process_device."""

    def __init__(self, num_streams, num_channels=1, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.AspHpfBatch_Create(C.byref(self.h), num_streams, num_channels, device), "AspHpfBatch_Create")
        self.S, self.C = num_streams, num_channels

    def close(self):
        if self.h:
            self.lib.AspHpfBatch_Free(self.h)
            self.h = C.c_void_p()

    def init(self, sample_rate_hz, stream=None):
        if stream is None:
            return self.lib.AspHpfBatch_Init(self.h, sample_rate_hz)
        return self.lib.AspHpfBatch_InitStream(self.h, stream, sample_rate_hz)

    def process(self, x, in_place=False):
        """x: int16 or float32 [F][S][C][n]; returns the filtered frames (x itself when in_place)."""
        assert x.dtype in (np.int16, np.float32) and x.shape[1:3] == (self.S, self.C) and x.flags.c_contiguous
        y = x if in_place else np.empty_like(x)
        fn = self.lib.AspHpfBatch_Process if x.dtype == np.int16 else self.lib.AspHpfBatch_ProcessFloatS16
        _check(fn(self.h, x.ctypes.data, y.ctypes.data, x.shape[0], x.shape[3], MEM_HOST), "AspHpfBatch_Process")
        return y

    def process_device(self, src, dst, num_frames, samples, is_float=False):
        """src, dst: device addresses of [F][S][C][n] arrays; returns once the launch is queued."""
        fn = self.lib.AspHpfBatch_ProcessFloatS16 if is_float else self.lib.AspHpfBatch_Process
        _check(fn(self.h, src, dst, num_frames, samples, MEM_DEVICE), "AspHpfBatch_Process")

    def export_state(self, stream, channel=0):
        st = AspHpfState()
        _check(self.lib.AspHpfBatch_ExportState(self.h, stream, channel, C.addressof(st)), "AspHpfBatch_ExportState")
        return st

    def import_state(self, stream, channel, st):
        return self.lib.AspHpfBatch_ImportState(self.h, stream, channel, C.addressof(st))

    def synchronize(self):
        _check(self.lib.AspHpfBatch_Synchronize(self.h), "AspHpfBatch_Synchronize")


def _restate_lib():
    L = C.CDLL(os.path.join(LIBDIR, "libhpf_restate.so"))
    vp, ip = C.c_void_p, C.c_int
    L.HpfRestate_Create.restype = vp
    L.HpfRestate_Free.argtypes = [vp]
    L.HpfRestate_State.argtypes = [vp]
    L.HpfRestate_State.restype = C.POINTER(AspHpfState)
    L.HpfRestate_Init.argtypes = [vp, ip]
    L.HpfRestate_Process.argtypes = [vp, vp, ip]
    L.HpfRestate_ProcessFloatS16.argtypes = [vp, vp, ip]
    L.LevelRestate_Create.restype = vp
    for name in ("Free", "Reset", "RMS"):
        getattr(L, "LevelRestate_" + name).argtypes = [vp]
    L.LevelRestate_State.argtypes = [vp]
    L.LevelRestate_Process.argtypes = [vp, vp, ip]
    L.LevelRestate_ProcessMuted.argtypes = [vp, ip]
    return L


_restate = None


def restate_library():
    """lib/libhpf_restate.so: the CPU build of the filter's and the level estimator's cores (tests only)."""
    global _restate
    if _restate is None:
        _restate = _restate_lib()
    return _restate


class Restate:
    """The CPU build of csrc/hpf_core.h, one stream-channel (tests only)."""

    def __init__(self, sample_rate_hz=None):
        self.L = restate_library()
        self.h = C.c_void_p(self.L.HpfRestate_Create())
        if sample_rate_hz is not None:
            assert self.init(sample_rate_hz) == 0

    def __del__(self):
        if getattr(self, "h", None):
            self.L.HpfRestate_Free(self.h)
            self.h = None

    def init(self, sample_rate_hz):
        return self.L.HpfRestate_Init(self.h, sample_rate_hz)

    def process(self, frame):
        """One frame, int16 or FloatS16 float32 [n]; returns the filtered copy."""
        y = np.ascontiguousarray(frame).copy()
        fn = self.L.HpfRestate_Process if y.dtype == np.int16 else self.L.HpfRestate_ProcessFloatS16
        assert y.dtype in (np.int16, np.float32) and fn(self.h, y.ctypes.data, y.size) == 0
        return y

    def run(self, x):
        """x: [F][n]; every frame in turn."""
        return np.stack([self.process(f) for f in x])

    @property
    def st(self):
        return self.L.HpfRestate_State(self.h).contents

    def state(self):
        return self.st.words()


def smoke_check(S=5, C_=2, F=6):
    """S streams x C_ channels x F frames (mixed coefficient sets, full-scale noise, so the clamp fires) on the GPU
    against the CPU build of the same core; True when bit-equal in output and state."""
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, (F, S, C_, 160)).astype(np.int16)
    b = HpfBatch(S, C_)
    ok = b.init(16000) == 0 and b.init(8000, stream=2) == 0
    y = b.process(x)
    for s in range(S):
        for c in range(C_):
            cpu = Restate(8000 if s == 2 else 16000)
            ok = ok and np.array_equal(cpu.run(x[:, s, c]), y[:, s, c])
            ok = ok and np.array_equal(cpu.state(), b.export_state(s, c).words())
    b.close()
    return bool(ok)
