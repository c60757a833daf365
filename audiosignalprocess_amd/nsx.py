"""Python mirror of the batched fixed-point noise suppressor's C-ABI (include/asp_nsx.h) over ctypes.
Plumbing only -- every call goes into libasp_amd.so; no CPU fallback.  Restate is the test-only CPU build
of the same core (lib/libnsx_restate.so)."""
import ctypes as C
import os

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST  # noqa: F401
from .build import LIBDIR
from .ns import AspError, _check, _declare, device_count, load_library as _load  # noqa: F401

I16, U16, I32, U32 = C.c_int16, C.c_uint16, C.c_int32, C.c_uint32
# NoiseSuppressionFixedC without its pointers, in its order: (name, ctype, count)
FIELDS = [
    ("fs", U32, 1), ("analysisBuffer", I16, 256), ("synthesisBuffer", I16, 256), ("noiseSupFilter", U16, 129),
    ("overdrive", U16, 1), ("denoiseBound", U16, 1), ("noiseEstLogQuantile", I16, 387),
    ("noiseEstDensity", I16, 387), ("noiseEstCounter", I16, 3), ("noiseEstQuantile", I16, 129),
    ("anaLen", I32, 1), ("anaLen2", I32, 1), ("magnLen", I32, 1), ("aggrMode", I32, 1), ("stages", I32, 1),
    ("initFlag", I32, 1), ("gainMap", I32, 1), ("maxLrt", I32, 1), ("minLrt", I32, 1),
    ("logLrtTimeAvgW32", I32, 129), ("featureLogLrt", I32, 1), ("thresholdLogLrt", I32, 1),
    ("weightLogLrt", I16, 1), ("featureSpecDiff", U32, 1), ("thresholdSpecDiff", U32, 1),
    ("weightSpecDiff", I16, 1), ("featureSpecFlat", U32, 1), ("thresholdSpecFlat", U32, 1),
    ("weightSpecFlat", I16, 1), ("avgMagnPause", I32, 129), ("magnEnergy", U32, 1), ("sumMagn", U32, 1),
    ("curAvgMagnEnergy", U32, 1), ("timeAvgMagnEnergy", U32, 1), ("timeAvgMagnEnergyTmp", U32, 1),
    ("whiteNoiseLevel", U32, 1), ("initMagnEst", U32, 129), ("pinkNoiseNumerator", I32, 1),
    ("pinkNoiseExp", I32, 1), ("minNorm", I32, 1), ("zeroInputSignal", I32, 1), ("prevNoiseU32", U32, 129),
    ("prevMagnU16", U16, 129), ("priorNonSpeechProb", I16, 1), ("blockIndex", I32, 1), ("modelUpdate", I32, 1),
    ("cntThresUpdate", I32, 1), ("histLrt", I16, 1000), ("histSpecFlat", I16, 1000), ("histSpecDiff", I16, 1000),
    ("dataBufHBFX", I16, 512), ("qNoise", I32, 1), ("prevQNoise", I32, 1), ("prevQMagn", I32, 1),
    ("blockLen10ms", I32, 1), ("real", I16, 256), ("imag", I16, 256), ("energyIn", I32, 1),
    ("scaleEnergyIn", I32, 1), ("normData", I32, 1),
]


class AspNsxState(C.Structure):
    _fields_ = [(n, t if k == 1 else t * k) for n, t, k in FIELDS]


def state_dict(st):
    """Every field of an AspNsxState (or of the reference's struct) as a numpy array."""
    return {n: np.array(getattr(st, n), dtype=np.dtype(t)).reshape(-1) for n, t, k in FIELDS}


_sig_done = False


def load_library():
    """libasp_amd.so with argtypes / restype set on every NSX entry point."""
    global _sig_done
    lib = _load()
    if not _sig_done:
        vp, ip = C.c_void_p, C.c_int
        sig = {
            "AspNsxBatch_Create": [C.POINTER(vp), ip, ip],
            "AspNsxBatch_Free": [vp],
            "AspNsxBatch_num_streams": [vp],
            "AspNsxBatch_Init": [vp, U32],
            "AspNsxBatch_InitStream": [vp, ip, U32],
            "AspNsxBatch_set_policy": [vp, ip],
            "AspNsxBatch_set_policy_stream": [vp, ip, ip],
            "AspNsxBatch_Process": [vp, vp, vp, vp, vp, ip, ip, ip],
            "AspNsxBatch_ProcessFrames": [vp, ip, vp, vp, vp, vp, ip, ip, ip],
            "AspNsxBatch_ExportState": [vp, ip, vp],
            "AspNsxBatch_ImportState": [vp, ip, vp],
            "AspNsxBatch_SetStream": [vp, vp],
            "AspNsxBatch_Synchronize": [vp],
            "WebRtcNsx_Create": [C.POINTER(vp)],
            "WebRtcNsx_Free": [vp],
            "WebRtcNsx_Init": [vp, U32],
            "WebRtcNsx_set_policy": [vp, ip],
            "WebRtcNsx_Process": [vp, vp, ip, vp],
            "AspNsx_last_refused": [],
        }
        _declare(lib, sig)
        lib.WebRtcNsx_Process.restype = None
        lib.AspNsx_state_size.argtypes = []
        lib.AspNsx_state_size.restype = C.c_size_t
        _sig_done = True
    return lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a)  # a device address


class NsxBatch:
    """AspNsxBatch_*: numpy arrays are host buffers, ints are device addresses (mem=MEM_DEVICE)."""

    def __init__(self, num_streams, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.AspNsxBatch_Create(C.byref(self.h), num_streams, device), "AspNsxBatch_Create")
        self.S = num_streams

    def close(self):
        if self.h:
            self.lib.AspNsxBatch_Free(self.h)
            self.h = C.c_void_p()

    def init(self, fs, stream=None):
        return self.lib.AspNsxBatch_Init(self.h, fs) if stream is None else self.lib.AspNsxBatch_InitStream(self.h, stream, fs)

    def set_policy(self, mode, stream=None):
        if stream is None:
            return self.lib.AspNsxBatch_set_policy(self.h, mode)
        return self.lib.AspNsxBatch_set_policy_stream(self.h, stream, mode)

    def process_frames(self, x, out=None):
        """x: int16 [F][bands][S][n] (host).  Returns the output in the same layout; out=x runs in place."""
        F, nb, S, n = x.shape
        assert S == self.S and x.dtype == np.int16 and x.flags.c_contiguous
        # the C-ABI takes the low band [F][S][n] and the high bands [F][nb - 1][S][n] as separate planes
        low = np.ascontiguousarray(x[:, 0])
        high = np.ascontiguousarray(x[:, 1:]) if nb > 1 else None
        lo, ho = (low, high) if out is x else (np.zeros_like(low), None if high is None else np.zeros_like(high))
        _check(self.lib.AspNsxBatch_ProcessFrames(self.h, F, _ptr(low), _ptr(high), _ptr(lo), _ptr(ho), nb, n, MEM_HOST),
               "AspNsxBatch_ProcessFrames")
        y = np.empty_like(x)
        y[:, 0] = lo
        if nb > 1:
            y[:, 1:] = ho
        return y

    def export_state(self, stream):
        st = AspNsxState()
        _check(self.lib.AspNsxBatch_ExportState(self.h, stream, C.addressof(st)), "AspNsxBatch_ExportState")
        return st

    def import_state(self, stream, st):
        return self.lib.AspNsxBatch_ImportState(self.h, stream, C.addressof(st))


class Restate:
    """The CPU build of csrc/nsx_core.h, one stream (tests only)."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = C.CDLL(os.path.join(LIBDIR, "libnsx_restate.so"))
            L.NsxRestate_Create.restype = C.c_void_p
            L.NsxRestate_Free.argtypes = [C.c_void_p]
            L.NsxRestate_Init.argtypes = [C.c_void_p, U32]
            L.NsxRestate_set_policy.argtypes = [C.c_void_p, C.c_int]
            L.NsxRestate_Process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
            L.NsxRestate_State.argtypes = [C.c_void_p]
            L.NsxRestate_State.restype = C.POINTER(AspNsxState)
            L.NsxRestate_Tables.argtypes = [C.c_void_p]
            L.NsxRestate_Tables.restype = C.c_void_p
            cls._lib = L
        return cls._lib

    def __init__(self):
        self.L = self.lib()
        self.h = C.c_void_p(self.L.NsxRestate_Create())

    def __del__(self):
        if getattr(self, "h", None):
            self.L.NsxRestate_Free(self.h)
            self.h = None

    def init(self, fs):
        return self.L.NsxRestate_Init(self.h, fs)

    def set_policy(self, mode):
        return self.L.NsxRestate_set_policy(self.h, mode)

    def process(self, x):
        """x: int16 [bands][n]; returns the output [bands][n]."""
        x = np.ascontiguousarray(x, np.int16)
        y = np.zeros_like(x)
        nb = x.shape[0]
        ip = (C.c_void_p * nb)(*[x[b].ctypes.data for b in range(nb)])
        op = (C.c_void_p * nb)(*[y[b].ctypes.data for b in range(nb)])
        if self.L.NsxRestate_Process(self.h, ip, nb, op) != 0:
            raise RuntimeError("NsxRestate_Process refused the call")
        return y

    @property
    def state(self):
        return self.L.NsxRestate_State(self.h).contents

    def tables(self):
        """The generated tables as a dict of int16 arrays (NsxTables, csrc/nsx_layout.h)."""
        names = [("sin1024", 1024), ("win128", 128), ("win256", 256), ("logFrac", 256), ("counterDiv", 201),
                 ("logTable", 9), ("logIndex", 129), ("sumLogIndex", 66), ("sumSqLogIndex", 66), ("detEstMatrix", 66),
                 ("factor1", 257), ("factor2", 3 * 257), ("indicator", 17)]
        total = sum(k for _, k in names)
        raw = np.ctypeslib.as_array((I16 * total).from_address(self.L.NsxRestate_Tables(self.h))).copy()
        out, o = {}, 0
        for n, k in names:
            out[n] = raw[o:o + k]
            o += k
        return out
