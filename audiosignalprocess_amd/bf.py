"""Python mirror of the batched beamformer's C-ABI (include/asp_bf.h) over ctypes.  Plumbing only -- every call
goes into libasp_amd.so; no CPU fallback.  Restate is the test-only CPU build of the same core
(lib/libbf_restate.so)."""
import ctypes as C
import os

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST  # noqa: F401
from .build import LIBDIR
from .ns import AspError, _check, _declare, device_count, load_library as _load  # noqa: F401

I32, F32 = C.c_int32, C.c_float
BINS, CHUNK, BUFFER, MIN_MICS, MAX_MICS = 129, 160, 384, 2, 8
# the Initialize-time tables, in the header's numbering
TABLES = ("window", "wave_numbers", "mask_thresholds", "delay_sum_masks", "target_cov_mats", "interf_cov_mats",
          "rxiws", "rpsiws", "reflected_rpsiws", "decay_threshold")

# AspBfState in its order: (name, ctype, shape)
FIELDS = [
    ("num_mics", I32, ()), ("frame_offset", I32, ()), ("current_block_ix", I32, ()), ("previous_block_ix", I32, ()),
    ("is_target_present", I32, ()), ("interference_blocks_count", I32, ()), ("high_pass_postfilter_mask", F32, ()),
    ("reserved", I32, ()), ("postfilter_masks", F32, (2, BINS)),
]


def _ctype(t, shape):
    for k in reversed(shape):
        t = t * k
    return t


class AspBfState(C.Structure):
    _fields_ = [(n, _ctype(t, s)) for n, t, s in FIELDS]


def state_dict(st, buffers):
    """Every field of an AspBfState and the buffer array as numpy arrays (input_buffer [M][384], output_buffer
    [384]); `reserved` left out."""
    d = {n: np.array(getattr(st, n), dtype=np.dtype(t)).reshape(s or (1,)) for n, t, s in FIELDS if n != "reserved"}
    M = int(st.num_mics)
    buffers = np.asarray(buffers, np.float32)
    d["input_buffer"] = buffers[:M * BUFFER].reshape(M, BUFFER).copy()
    d["output_buffer"] = buffers[M * BUFFER:(M + 1) * BUFFER].copy()
    return d


def table_length(which, M):
    return (256, BINS, BINS, BINS * M * 2, BINS * M * M * 2, BINS * M * M * 2, BINS, BINS, BINS, 1)[which]


def linear_geometry(num_mics, spacing):
    """[M][3] float32: a uniform linear array along x, the first microphone at the origin."""
    g = np.zeros((num_mics, 3), np.float32)
    g[:, 0] = np.arange(num_mics, dtype=np.float32) * np.float32(spacing)
    return g


_sig_done = False


def load_library():
    """libasp_amd.so with argtypes / restype set on every beamformer entry point."""
    global _sig_done
    lib = _load()
    if not _sig_done:
        vp, ip = C.c_void_p, C.c_int
        sig = {
            "AspBfBatch_Create": [C.POINTER(vp), ip, ip],
            "AspBfBatch_Free": [vp],
            "AspBfBatch_num_streams": [vp],
            "AspBfBatch_Initialize": [vp, ip, vp, ip, ip],
            "AspBfBatch_InitializeStream": [vp, ip],
            "AspBfBatch_ProcessChunk": [vp, vp, vp, vp, vp, vp, ip],
            "AspBfBatch_ProcessChunks": [vp, ip, vp, vp, vp, vp, vp, ip],
            "AspBfBatch_state_floats": [vp],
            "AspBfBatch_GetState": [vp, ip, vp, vp],
            "AspBfBatch_SetState": [vp, ip, vp, vp],
            "AspBfBatch_GetTables": [vp, ip, vp, ip],
            "AspBfBatch_SetTables": [vp, ip, vp, ip],
            "AspBfBatch_SetStream": [vp, vp],
            "AspBfBatch_Synchronize": [vp],
            "AspBf_debug_hypotf": [vp, vp, vp, C.c_size_t, ip],
        }
        _declare(lib, sig)
        lib.AspBf_state_size.argtypes = []
        lib.AspBf_state_size.restype = C.c_size_t
        _sig_done = True
    return lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a)  # a device address


class BfBatch:
    """AspBfBatch_* on host buffers (numpy): input float32 [F][S][M][160], high band the same or None."""

    def __init__(self, num_streams, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.AspBfBatch_Create(C.byref(self.h), num_streams, device), "AspBfBatch_Create")
        self.S = num_streams
        self.M = 0

    def close(self):
        if self.h:
            self.lib.AspBfBatch_Free(self.h)
            self.h = C.c_void_p()

    def initialize(self, geometry, chunk_size_ms=10, sample_rate_hz=16000, num_mics=None, stream=None):
        if stream is not None:
            return self.lib.AspBfBatch_InitializeStream(self.h, stream)
        g = np.ascontiguousarray(geometry, np.float32)
        M = g.shape[0] if num_mics is None else num_mics
        rc = self.lib.AspBfBatch_Initialize(self.h, M, _ptr(g), chunk_size_ms, sample_rate_hz)
        if rc == 0:
            self.M = M
        return rc

    def process_chunks(self, x, high=None, single=False):
        """Returns (rc, output [F][S][160], high output [F][S][160] or None, target_present uint8 [F][S]).
        single: one chunk through AspBfBatch_ProcessChunk."""
        x = np.ascontiguousarray(x, np.float32)
        F, S, M, L = x.shape
        assert S == self.S and M == self.M and L == CHUNK
        hi = None if high is None else np.ascontiguousarray(high, np.float32)
        assert hi is None or hi.shape == x.shape
        y = np.zeros((F, S, CHUNK), np.float32)
        hy = None if hi is None else np.zeros((F, S, CHUNK), np.float32)
        tp = np.zeros((F, S), np.uint8)
        if single:
            assert F == 1
            rc = self.lib.AspBfBatch_ProcessChunk(self.h, _ptr(x), _ptr(hi), _ptr(y), _ptr(hy), _ptr(tp), MEM_HOST)
        else:
            rc = self.lib.AspBfBatch_ProcessChunks(self.h, F, _ptr(x), _ptr(hi), _ptr(y), _ptr(hy), _ptr(tp), MEM_HOST)
        return rc, y, hy, tp

    def get_state(self, stream):
        st = AspBfState()
        buf = np.zeros(self.lib.AspBfBatch_state_floats(self.h), np.float32)
        _check(self.lib.AspBfBatch_GetState(self.h, stream, C.addressof(st), _ptr(buf)), "AspBfBatch_GetState")
        return st, buf

    def set_state(self, stream, st, buf):
        return self.lib.AspBfBatch_SetState(self.h, stream, C.addressof(st), _ptr(np.ascontiguousarray(buf, np.float32)))

    def get_table(self, which):
        out = np.zeros(table_length(which, self.M), np.float32)
        n = self.lib.AspBfBatch_GetTables(self.h, which, _ptr(out), out.size)
        if n != out.size:
            raise AspError("AspBfBatch_GetTables(%d) returned %d" % (which, n))
        return out

    def set_table(self, which, values):
        v = np.ascontiguousarray(values, np.float32).ravel()
        return self.lib.AspBfBatch_SetTables(self.h, which, _ptr(v), v.size)

    def synchronize(self):
        return self.lib.AspBfBatch_Synchronize(self.h)


class Restate:
    """The CPU build of csrc/bf_core.h, one stream (tests only)."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = C.CDLL(os.path.join(LIBDIR, "libbf_restate.so"))
            vp, ip = C.c_void_p, C.c_int
            L.BfRestate_Create.restype = vp
            L.BfRestate_Free.argtypes = [vp]
            L.BfRestate_State.argtypes = [vp]
            L.BfRestate_State.restype = C.POINTER(AspBfState)
            L.BfRestate_Buffers.argtypes = [vp]
            L.BfRestate_Buffers.restype = C.POINTER(F32)
            L.BfRestate_BufferFloats.argtypes = [vp]
            L.BfRestate_Why.argtypes = [vp]
            L.BfRestate_Why.restype = C.c_char_p
            L.BfRestate_Initialize.argtypes = [vp, ip, vp, ip, ip]
            L.BfRestate_ProcessChunk.argtypes = [vp, vp, vp, vp, vp]
            L.BfRestate_GetTables.argtypes = [vp, ip, vp, ip]
            L.BfRestate_SetTables.argtypes = [vp, ip, vp, ip]
            L.BfRestate_Params.argtypes = [vp, vp]
            L.BfRestate_MicSpacing.argtypes = [vp]
            L.BfRestate_MicSpacing.restype = F32
            L.BfRestate_hypotf.argtypes = [vp, vp, vp, C.c_size_t]
            cls._lib = L
        return cls._lib

    def __init__(self):
        self.L = self.lib()
        self.h = C.c_void_p(self.L.BfRestate_Create())
        self.M = 0

    def __del__(self):
        if getattr(self, "h", None):
            self.L.BfRestate_Free(self.h)
            self.h = None

    def initialize(self, geometry, chunk_size_ms=10, sample_rate_hz=16000, num_mics=None):
        g = np.ascontiguousarray(geometry, np.float32)
        M = g.shape[0] if num_mics is None else num_mics
        rc = self.L.BfRestate_Initialize(self.h, M, _ptr(g), chunk_size_ms, sample_rate_hz)
        if rc == 0:
            self.M = M
        return rc

    @property
    def why(self):
        return self.L.BfRestate_Why(self.h).decode()

    def process_chunk(self, x, high=None):
        """x float32 [M][160]; returns (output [160], high output [160] or None, is_target_present)."""
        x = np.ascontiguousarray(x, np.float32)
        hi = None if high is None else np.ascontiguousarray(high, np.float32)
        y = np.zeros(CHUNK, np.float32)
        hy = None if hi is None else np.zeros(CHUNK, np.float32)
        tp = self.L.BfRestate_ProcessChunk(self.h, _ptr(x), _ptr(hi), _ptr(y), _ptr(hy))
        if tp < 0:
            raise ValueError("BfRestate_ProcessChunk refused the call")
        return y, hy, tp

    def get_table(self, which):
        out = np.zeros(table_length(which, self.M), np.float32)
        assert self.L.BfRestate_GetTables(self.h, which, _ptr(out), out.size) == out.size
        return out

    def set_table(self, which, values):
        v = np.ascontiguousarray(values, np.float32).ravel()
        return self.L.BfRestate_SetTables(self.h, which, _ptr(v), v.size)

    def params(self):
        out = np.zeros(5, np.int32)
        self.L.BfRestate_Params(self.h, _ptr(out))
        return out

    @property
    def state(self):
        return self.L.BfRestate_State(self.h).contents

    @property
    def buffers(self):
        n = self.L.BfRestate_BufferFloats(self.h)
        return np.ctypeslib.as_array(self.L.BfRestate_Buffers(self.h), (n,)).copy()


def smoke_check(S=3, F=12, M=4):
    """S streams x F chunks of a 4-microphone array with the high band on the GPU against the CPU build of the
    same core, with the CPU build's tables on both sides; True when bit-equal."""
    from .synth import bf_chunks

    x, hi = bf_chunks(S, F, M, seed=3, broadside=((0, 6),), offaxis=((4, 12),), silent=((8, 9),))
    g = linear_geometry(M, 0.04)
    cpu = Restate()
    cpu.initialize(g)
    b = BfBatch(S)
    ok = b.initialize(g) == 0
    for which in range(len(TABLES)):   # one set of tables on both sides: the CPU build's
        ok = ok and b.set_table(which, cpu.get_table(which)) == 0
    rc, y, hy, tp = b.process_chunks(x, hi)
    b.close()
    ok = ok and rc == 0
    for s in range(S):
        cpu = Restate()
        cpu.initialize(g)
        for f in range(F):
            wy, why, wtp = cpu.process_chunk(x[f, s], hi[f, s])
            ok = ok and np.array_equal(wy.view(np.uint32), y[f, s].view(np.uint32))
            ok = ok and np.array_equal(why.view(np.uint32), hy[f, s].view(np.uint32)) and wtp == tp[f, s]
    return bool(ok)
