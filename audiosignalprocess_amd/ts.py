"""Python mirror of the batched transient suppressor's C-ABI (include/asp_ts.h) over ctypes.  Plumbing only
-- every call goes into libasp_amd.so; no CPU fallback.  Restate is the test-only CPU build of the same
core (lib/libts_restate.so)."""
import ctypes as C
import os

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST  # noqa: F401
from .build import LIBDIR
from .ns import AspError, _check, _declare, device_count, load_library as _load  # noqa: F401

I32, U32, F32 = C.c_int32, C.c_uint32, C.c_float
LEAVES, NODES, HISTORY, MAX_QUEUE = 8, 7, 15, 180

# AspTsState in its order: (name, ctype, shape)
FIELDS = [
    ("sample_rate_hz", I32, ()), ("detection_rate_hz", I32, ()), ("num_channels", I32, ()),
    ("detector_smoothed", F32, ()), ("keypress_counter", I32, ()), ("chunks_since_keypress", I32, ()),
    ("detection_enabled", I32, ()), ("suppression_enabled", I32, ()), ("use_hard_restoration", I32, ()),
    ("chunks_since_voice_change", I32, ()), ("seed", U32, ()), ("using_reference", I32, ()),
    ("chunks_at_startup_left_to_delete", I32, ()), ("reference_energy", F32, ()),
    ("detector_using_reference", I32, ()), ("previous_results", F32, (3,)),
    ("last_first_moment", F32, (LEAVES,)), ("last_second_moment", F32, (LEAVES,)),
    ("moment_sum", F32, (LEAVES,)), ("moment_sum_of_squares", F32, (LEAVES,)), ("queue_pos", I32, ()),
    ("moment_queue", F32, (LEAVES, MAX_QUEUE)), ("node_history", F32, (NODES, HISTORY)),
]


def _ctype(t, shape):
    for k in reversed(shape):
        t = t * k
    return t


class AspTsState(C.Structure):
    _fields_ = [(n, _ctype(t, s)) for n, t, s in FIELDS]


def state_dict(st):
    """Every field of an AspTsState as a numpy array; the moment queues oldest first, [LEAVES][3 T]."""
    d = {n: np.array(getattr(st, n), dtype=np.dtype(t)).reshape(s or (1,)) for n, t, s in FIELDS}
    T = st.detection_rate_hz // 800
    q = d["moment_queue"][:, :3 * T].reshape(LEAVES, 3, T)
    d["moment_queue"] = np.roll(q, -int(st.queue_pos), axis=1).reshape(LEAVES, 3 * T)
    del d["queue_pos"]
    return d


def lengths(rate, det_rate):
    """(analysis length N, chunk L, bins, detection chunk D)."""
    N = {8000: 128, 16000: 256, 32000: 512, 48000: 1024}[rate]
    return N, rate // 100, N // 2 + 1, det_rate // 100


_sig_done = False


def load_library():
    """libasp_amd.so with argtypes / restype set on every transient-suppressor entry point."""
    global _sig_done
    lib = _load()
    if not _sig_done:
        vp, ip, sz = C.c_void_p, C.c_int, C.c_size_t
        sig = {
            "AspTsBatch_Create": [C.POINTER(vp), ip, ip],
            "AspTsBatch_Free": [vp],
            "AspTsBatch_num_streams": [vp],
            "AspTsBatch_Initialize": [vp, ip, ip, ip],
            "AspTsBatch_InitializeStream": [vp, ip],
            "AspTsBatch_state_floats": [vp],
            "AspTsBatch_GetState": [vp, ip, vp, vp],
            "AspTsBatch_SetState": [vp, ip, vp, vp],
            "AspTsBatch_Suppress": [vp, vp, sz, ip, vp, sz, vp, sz, vp, vp, vp, vp, ip],
            "AspTsBatch_SuppressFrames": [vp, ip, vp, sz, ip, vp, sz, vp, sz, vp, vp, vp, vp, ip],
            "AspTs_table": [ip, ip, vp, ip],
            "AspTsBatch_SetStream": [vp, vp],
            "AspTsBatch_Synchronize": [vp],
        }
        _declare(lib, sig)
        lib.AspTs_state_size.argtypes = []
        lib.AspTs_state_size.restype = C.c_size_t
        _sig_done = True
    return lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a)  # a device address


class TsBatch:
    """AspTsBatch_* on host buffers (numpy): data float32 [F][S][C][L], detection [F][S][D], reference [F][S][R],
    per-stream scalars [F][S]."""

    def __init__(self, num_streams, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.AspTsBatch_Create(C.byref(self.h), num_streams, device), "AspTsBatch_Create")
        self.S = num_streams

    def close(self):
        if self.h:
            self.lib.AspTsBatch_Free(self.h)
            self.h = C.c_void_p()

    def initialize(self, rate, det_rate, channels, stream=None):
        if stream is not None:
            return self.lib.AspTsBatch_InitializeStream(self.h, stream)
        return self.lib.AspTsBatch_Initialize(self.h, rate, det_rate, channels)

    def suppress_frames(self, data, voice, keys, detection=None, reference=None, present=None, single=False):
        """Returns (rc, data after, results [F][S]).  single: one chunk through AspTsBatch_Suppress."""
        y = np.ascontiguousarray(data, np.float32).copy()
        F, S, Cn, L = y.shape
        assert S == self.S
        det = None if detection is None else np.ascontiguousarray(detection, np.float32)
        ref = None if reference is None else np.ascontiguousarray(reference, np.float32)
        pr = None if present is None else np.ascontiguousarray(present, np.uint8)
        vp = np.ascontiguousarray(voice, np.float32).reshape(F, S)
        kp = np.ascontiguousarray(keys, np.uint8).reshape(F, S)
        res = np.zeros((F, S), np.int32)
        D = L if det is None else det.shape[-1]
        R = 0 if ref is None else ref.shape[-1]
        if single:
            assert F == 1
            rc = self.lib.AspTsBatch_Suppress(self.h, _ptr(y), L, Cn, _ptr(det), D, _ptr(ref), R, _ptr(pr), _ptr(vp),
                                              _ptr(kp), _ptr(res), MEM_HOST)
        else:
            rc = self.lib.AspTsBatch_SuppressFrames(self.h, F, _ptr(y), L, Cn, _ptr(det), D, _ptr(ref), R, _ptr(pr),
                                                    _ptr(vp), _ptr(kp), _ptr(res), MEM_HOST)
        return rc, y, res

    def get_state(self, stream):
        st = AspTsState()
        buf = np.zeros(self.lib.AspTsBatch_state_floats(self.h), np.float32)
        _check(self.lib.AspTsBatch_GetState(self.h, stream, C.addressof(st), _ptr(buf)), "AspTsBatch_GetState")
        return st, buf

    def set_state(self, stream, st, buf):
        return self.lib.AspTsBatch_SetState(self.h, stream, C.addressof(st), _ptr(np.ascontiguousarray(buf, np.float32)))


def table(lib_fn, which, n):
    out = np.zeros(n + 2, np.float32)
    k = lib_fn(which, n, out.ctypes.data, out.size)
    if k < 0:
        raise ValueError("no such table")
    return out[:k]


class Restate:
    """The CPU build of csrc/ts_core.h, one stream (tests only)."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = C.CDLL(os.path.join(LIBDIR, "libts_restate.so"))
            vp, sz = C.c_void_p, C.c_size_t
            L.TsRestate_Create.restype = vp
            L.TsRestate_Free.argtypes = [vp]
            L.TsRestate_State.argtypes = [vp]
            L.TsRestate_State.restype = C.POINTER(AspTsState)
            L.TsRestate_Buffers.argtypes = [vp]
            L.TsRestate_Buffers.restype = C.POINTER(F32)
            L.TsRestate_BufferFloats.argtypes = [vp]
            L.TsRestate_Initialize.argtypes = [vp, C.c_int, C.c_int, C.c_int]
            L.TsRestate_Suppress.argtypes = [vp, vp, sz, C.c_int, vp, sz, vp, sz, F32, C.c_int]
            L.TsRestate_table.argtypes = [C.c_int, C.c_int, vp, C.c_int]
            L.TsRestate_phases.argtypes = [vp]
            L.TsRestate_phase_table.restype = C.POINTER(F32)
            L.TsRestate_eval.argtypes = [C.c_int, vp, vp, sz]
            L.TsRestate_lcg_jump.argtypes = [U32, U32]
            L.TsRestate_lcg_jump.restype = U32
            cls._lib = L
        return cls._lib

    def __init__(self):
        self.L = self.lib()
        self.h = C.c_void_p(self.L.TsRestate_Create())

    def __del__(self):
        if getattr(self, "h", None):
            self.L.TsRestate_Free(self.h)
            self.h = None

    def initialize(self, rate, det_rate, channels):
        return self.L.TsRestate_Initialize(self.h, rate, det_rate, channels)

    def suppress(self, data, voice, key, detection=None, reference=None, data_length=None, channels=None,
                 detection_length=None):
        """data float32 [C][L]; returns (rc, data after)."""
        y = np.ascontiguousarray(data, np.float32).copy()
        det = None if detection is None else np.ascontiguousarray(detection, np.float32)
        ref = None if reference is None else np.ascontiguousarray(reference, np.float32)
        L = y.shape[-1] if data_length is None else data_length
        D = (L if det is None else det.size) if detection_length is None else detection_length
        rc = self.L.TsRestate_Suppress(self.h, y.ctypes.data, L, y.shape[0] if channels is None else channels,
                                       _ptr(det), D, _ptr(ref), 0 if ref is None else ref.size, float(voice), int(key))
        return rc, y

    @property
    def state(self):
        return self.L.TsRestate_State(self.h).contents

    @property
    def buffers(self):
        n = self.L.TsRestate_BufferFloats(self.h)
        return np.ctypeslib.as_array(self.L.TsRestate_Buffers(self.h), (n,)).copy()


def smoke_check(S=3, F=24):
    """S streams x F chunks at 16 kHz (suppression enabled by two keypresses, soft restoration) on the GPU
    against the CPU build of the same core; True when bit-equal."""
    from .synth import ts_chunks

    x, ref = ts_chunks(S, F, 16000, 1)
    keys = np.zeros((F, S), np.uint8)
    keys[1:3] = 1
    voice = np.full((F, S), 0.5, np.float32)
    b = TsBatch(S)
    ok = b.initialize(16000, 16000, 1) == 0
    rc, y, _ = b.suppress_frames(x, voice, keys, reference=ref)
    b.close()
    ok = ok and rc == 0
    for s in range(S):
        cpu = Restate()
        cpu.initialize(16000, 16000, 1)
        for f in range(F):
            _, want = cpu.suppress(x[f, s], voice[f, s], keys[f, s], reference=ref[f, s])
            ok = ok and np.array_equal(want.view(np.uint32), y[f, s].view(np.uint32))
    return bool(ok)
