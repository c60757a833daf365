"""Python mirror of the batched legacy gain control's C-ABI (include/asp_agc.h) over ctypes.  Plumbing only
-- every call goes into libasp_amd.so; no CPU fallback.  Restate is the test-only CPU build of the same
core (lib/libagc_restate.so)."""
import ctypes as C
import os

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST  # noqa: F401
from .build import LIBDIR
from .ns import AspError, _check, _declare, device_count, load_library as _load  # noqa: F401

I16, U16, I32, U32, U8 = C.c_int16, C.c_uint16, C.c_int32, C.c_uint32, C.c_uint8
OP_FAR, OP_ADD_MIC, OP_VIRTUAL_MIC, OP_PROCESS, OP_BY_MODE = 1, 2, 4, 8, 16


def _vad(p):
    return [(p + "_downState", I32, 8), (p + "_HPstate", I16, 1), (p + "_counter", I16, 1), (p + "_logRatio", I16, 1),
            (p + "_meanLongTerm", I16, 1), (p + "_varianceLongTerm", I32, 1), (p + "_stdLongTerm", I16, 1),
            (p + "_meanShortTerm", I16, 1), (p + "_varianceShortTerm", I32, 1), (p + "_stdShortTerm", I16, 1)]


# LegacyAgc in its order, AgcVad and DigitalAgc flattened: (name, ctype, count)
FIELDS = [
    ("fs", U32, 1), ("compressionGaindB", I16, 1), ("targetLevelDbfs", I16, 1), ("agcMode", I16, 1),
    ("limiterEnable", U8, 1), ("defaultConfig_targetLevelDbfs", I16, 1), ("defaultConfig_compressionGaindB", I16, 1),
    ("defaultConfig_limiterEnable", U8, 1), ("usedConfig_targetLevelDbfs", I16, 1),
    ("usedConfig_compressionGaindB", I16, 1), ("usedConfig_limiterEnable", U8, 1), ("initFlag", I16, 1),
    ("lastError", I16, 1), ("analogTargetLevel", I32, 1), ("startUpperLimit", I32, 1), ("startLowerLimit", I32, 1),
    ("upperPrimaryLimit", I32, 1), ("lowerPrimaryLimit", I32, 1), ("upperSecondaryLimit", I32, 1),
    ("lowerSecondaryLimit", I32, 1), ("targetIdx", U16, 1), ("analogTarget", I16, 1), ("filterState", I32, 8),
    ("upperLimit", I32, 1), ("lowerLimit", I32, 1), ("Rxx160w32", I32, 1), ("Rxx16_LPw32", I32, 1),
    ("Rxx160_LPw32", I32, 1), ("Rxx16_LPw32Max", I32, 1), ("Rxx16_vectorw32", I32, 10), ("Rxx16w32_array", I32, 10),
    ("env", I32, 20), ("Rxx16pos", I16, 1), ("envSum", I16, 1), ("vadThreshold", I16, 1), ("inActive", I16, 1),
    ("msTooLow", I16, 1), ("msTooHigh", I16, 1), ("changeToSlowMode", I16, 1), ("firstCall", I16, 1),
    ("msZero", I16, 1), ("msecSpeechOuterChange", I16, 1), ("msecSpeechInnerChange", I16, 1),
    ("activeSpeech", I16, 1), ("muteGuardMs", I16, 1), ("inQueue", I16, 1), ("micRef", I32, 1),
    ("gainTableIdx", U16, 1), ("micGainIdx", I32, 1), ("micVol", I32, 1), ("maxLevel", I32, 1), ("maxAnalog", I32, 1),
    ("maxInit", I32, 1), ("minLevel", I32, 1), ("minOutput", I32, 1), ("zeroCtrlMax", I32, 1),
    ("lastInMicLevel", I32, 1), ("scale", I16, 1),
] + _vad("vadMic") + [
    ("digitalAgc_capacitorSlow", I32, 1), ("digitalAgc_capacitorFast", I32, 1), ("digitalAgc_gain", I32, 1),
    ("digitalAgc_gainTable", I32, 32), ("digitalAgc_gatePrevious", I16, 1), ("digitalAgc_agcMode", I16, 1),
] + _vad("vadNearend") + _vad("vadFarend") + [("lowLevelSignal", I16, 1)]


class AspAgcState(C.Structure):
    _fields_ = [(n, t if k == 1 else t * k) for n, t, k in FIELDS]


class WebRtcAgcConfig(C.Structure):
    _fields_ = [("targetLevelDbfs", I16), ("compressionGaindB", I16), ("limiterEnable", U8)]


def state_dict(st):
    """Every field of an AspAgcState as a numpy array."""
    return {n: np.array(getattr(st, n), dtype=np.dtype(t)).reshape(-1) for n, t, k in FIELDS}


_sig_done = False


def load_library():
    """libasp_amd.so with argtypes / restype set on every AGC entry point."""
    global _sig_done
    lib = _load()
    if not _sig_done:
        vp, ip = C.c_void_p, C.c_int
        cfg = WebRtcAgcConfig
        sig = {
            "AspAgc_gain_table": [vp, I16, I16, U8, I16],
            "AspAgcBatch_Create": [C.POINTER(vp), ip, ip],
            "AspAgcBatch_Free": [vp],
            "AspAgcBatch_num_streams": [vp],
            "AspAgcBatch_Init": [vp, I32, I32, I16, U32],
            "AspAgcBatch_InitStream": [vp, ip, I32, I32, I16, U32],
            "AspAgcBatch_set_config": [vp, cfg],
            "AspAgcBatch_set_config_stream": [vp, ip, cfg],
            "AspAgcBatch_get_config_stream": [vp, ip, C.POINTER(cfg)],
            "AspAgcBatch_last_error_stream": [vp, ip],
            "AspAgcBatch_set_mic_level": [vp, I32],
            "AspAgcBatch_set_mic_level_stream": [vp, ip, I32],
            "AspAgcBatch_get_mic_level_stream": [vp, ip, C.POINTER(I32)],
            "AspAgcBatch_AddFarend": [vp, vp, ip, ip],
            "AspAgcBatch_AddMic": [vp, vp, vp, ip, ip, ip],
            "AspAgcBatch_VirtualMic": [vp, vp, vp, ip, ip, vp, vp, ip],
            "AspAgcBatch_Process": [vp, vp, vp, vp, vp, ip, ip, vp, vp, vp, vp, ip],
            "AspAgcBatch_ProcessFrames": [vp, ip, vp, vp, vp, vp, vp, ip, ip, vp, vp, vp, vp, ip],
            "AspAgcBatch_returns": [vp, vp, ip],
            "AspAgcBatch_ExportState": [vp, ip, vp],
            "AspAgcBatch_ImportState": [vp, ip, vp],
            "AspAgcBatch_SetStream": [vp, vp],
            "AspAgcBatch_Synchronize": [vp],
            "WebRtcAgc_Create": [C.POINTER(vp)],
            "WebRtcAgc_Free": [vp],
            "WebRtcAgc_Init": [vp, I32, I32, I16, U32],
            "WebRtcAgc_set_config": [vp, cfg],
            "WebRtcAgc_get_config": [vp, C.POINTER(cfg)],
            "WebRtcAgc_AddFarend": [vp, vp, I16],
            "WebRtcAgc_AddMic": [vp, vp, I16, I16],
            "WebRtcAgc_VirtualMic": [vp, vp, I16, I16, I32, C.POINTER(I32)],
            "WebRtcAgc_Process": [vp, vp, I16, I16, vp, I32, C.POINTER(I32), I16, C.POINTER(U8)],
        }
        _declare(lib, sig)
        lib.AspAgc_state_size.argtypes = []
        lib.AspAgc_state_size.restype = C.c_size_t
        _sig_done = True
    return lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a)  # a device address


def split(x):
    """int16 [F][bands][S][n] -> the C-ABI's planes: low [F][S][n], high [F][bands - 1][S][n] or None."""
    low = np.ascontiguousarray(x[:, 0])
    high = np.ascontiguousarray(x[:, 1:]) if x.shape[1] > 1 else None
    return low, high


def join(low, high):
    F, S, n = low.shape
    y = np.empty((F, 1 if high is None else 1 + high.shape[1], S, n), np.int16)
    y[:, 0] = low
    if high is not None:
        y[:, 1:] = high
    return y


class AgcBatch:
    """AspAgcBatch_* on host buffers (numpy); audio is int16 [F][bands][S][n], per-stream scalars [F][S]."""

    def __init__(self, num_streams, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.AspAgcBatch_Create(C.byref(self.h), num_streams, device), "AspAgcBatch_Create")
        self.S = num_streams

    def close(self):
        if self.h:
            self.lib.AspAgcBatch_Free(self.h)
            self.h = C.c_void_p()

    def init(self, min_level, max_level, mode, fs, stream=None):
        if stream is None:
            return self.lib.AspAgcBatch_Init(self.h, min_level, max_level, mode, fs)
        return self.lib.AspAgcBatch_InitStream(self.h, stream, min_level, max_level, mode, fs)

    def set_config(self, target, compression, limiter, stream=None):
        cfg = WebRtcAgcConfig(target, compression, limiter)
        if stream is None:
            return self.lib.AspAgcBatch_set_config(self.h, cfg)
        return self.lib.AspAgcBatch_set_config_stream(self.h, stream, cfg)

    def get_config(self, stream):
        cfg = WebRtcAgcConfig()
        rc = self.lib.AspAgcBatch_get_config_stream(self.h, stream, C.byref(cfg))
        return rc, (cfg.targetLevelDbfs, cfg.compressionGaindB, cfg.limiterEnable)

    def last_error(self, stream):
        return self.lib.AspAgcBatch_last_error_stream(self.h, stream)

    def set_mic_level(self, level, stream=None):
        if stream is None:
            return self.lib.AspAgcBatch_set_mic_level(self.h, level)
        return self.lib.AspAgcBatch_set_mic_level_stream(self.h, stream, level)

    def get_mic_level(self, stream):
        v = I32()
        _check(self.lib.AspAgcBatch_get_mic_level_stream(self.h, stream, C.byref(v)), "AspAgcBatch_get_mic_level_stream")
        return v.value

    def returns(self, count):
        rc = np.zeros(count, np.int32)
        _check(self.lib.AspAgcBatch_returns(self.h, _ptr(rc), count), "AspAgcBatch_returns")
        return rc

    def add_farend(self, far):
        """far: int16 [S][n]."""
        far = np.ascontiguousarray(far, np.int16)
        _check(self.lib.AspAgcBatch_AddFarend(self.h, _ptr(far), far.shape[-1], MEM_HOST), "AspAgcBatch_AddFarend")

    def add_mic(self, x):
        """x: int16 [bands][S][n]; returns what AddMic left in it."""
        low, high = split(np.ascontiguousarray(x[None]))
        _check(self.lib.AspAgcBatch_AddMic(self.h, _ptr(low), _ptr(high), x.shape[0], x.shape[2], MEM_HOST),
               "AspAgcBatch_AddMic")
        return join(low, high)[0]

    def virtual_mic(self, x, level_in):
        """x: int16 [bands][S][n], level_in int32 [S]; returns (x after, micLevelOut [S])."""
        low, high = split(np.ascontiguousarray(x[None]))
        li = np.ascontiguousarray(level_in, np.int32)
        lo = np.zeros(self.S, np.int32)
        _check(self.lib.AspAgcBatch_VirtualMic(self.h, _ptr(low), _ptr(high), x.shape[0], x.shape[2], _ptr(li), _ptr(lo),
                                               MEM_HOST), "AspAgcBatch_VirtualMic")
        return join(low, high)[0], lo

    def process(self, x, level_in, echo=None, in_place=False):
        """x: int16 [bands][S][n]; returns (out, outMicLevel [S], saturationWarning [S])."""
        low, high = split(np.ascontiguousarray(x[None]))
        lo, ho = (low, high) if in_place else (np.zeros_like(low), None if high is None else np.zeros_like(high))
        li = np.ascontiguousarray(level_in, np.int32)
        ec = None if echo is None else np.ascontiguousarray(echo, np.int16)
        out, sat = np.zeros(self.S, np.int32), np.zeros(self.S, np.uint8)
        _check(self.lib.AspAgcBatch_Process(self.h, _ptr(low), _ptr(high), _ptr(lo), _ptr(ho), x.shape[0], x.shape[2],
                                            _ptr(li), _ptr(ec), _ptr(out), _ptr(sat), MEM_HOST), "AspAgcBatch_Process")
        return join(lo, ho)[0], out, sat

    def process_frames(self, x, far=None, level_in=None, echo=None, in_place=False):
        """x: int16 [F][bands][S][n], far [F][S][n] or None, level_in int32 [F][S] or None (chained), echo int16
        [F][S] or None.  Returns (out like x, outMicLevel [F][S], saturationWarning [F][S])."""
        F, nb, S, n = x.shape
        assert S == self.S and x.dtype == np.int16
        low, high = split(x)
        lo, ho = (low, high) if in_place else (np.zeros_like(low), None if high is None else np.zeros_like(high))
        fa = None if far is None else np.ascontiguousarray(far, np.int16)
        li = None if level_in is None else np.ascontiguousarray(level_in, np.int32)
        ec = None if echo is None else np.ascontiguousarray(echo, np.int16)
        out, sat = np.zeros((F, S), np.int32), np.zeros((F, S), np.uint8)
        _check(self.lib.AspAgcBatch_ProcessFrames(self.h, F, _ptr(fa), _ptr(low), _ptr(high), _ptr(lo), _ptr(ho), nb, n,
                                                  _ptr(li), _ptr(ec), _ptr(out), _ptr(sat), MEM_HOST),
               "AspAgcBatch_ProcessFrames")
        return join(lo, ho), out, sat

    def export_state(self, stream):
        st = AspAgcState()
        _check(self.lib.AspAgcBatch_ExportState(self.h, stream, C.addressof(st)), "AspAgcBatch_ExportState")
        return st

    def import_state(self, stream, st):
        return self.lib.AspAgcBatch_ImportState(self.h, stream, C.addressof(st))


class Restate:
    """The CPU build of csrc/agc_core.h, one stream (tests only)."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = C.CDLL(os.path.join(LIBDIR, "libagc_restate.so"))
            vp = C.c_void_p
            L.AgcRestate_Create.restype = vp
            L.AgcRestate_Free.argtypes = [vp]
            L.AgcRestate_State.argtypes = [vp]
            L.AgcRestate_State.restype = C.POINTER(AspAgcState)
            L.AgcRestate_Init.argtypes = [vp, I32, I32, I16, U32]
            L.AgcRestate_set_config.argtypes = [vp, I16, I16, U8]
            L.AgcRestate_gain_table.argtypes = [vp, I16, I16, U8, I16]
            L.AgcRestate_Frame.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, I32, I16, C.POINTER(I32),
                                           C.POINTER(I32), C.POINTER(U8)]
            cls._lib = L
        return cls._lib

    def __init__(self):
        self.L = self.lib()
        self.h = C.c_void_p(self.L.AgcRestate_Create())

    def __del__(self):
        if getattr(self, "h", None):
            self.L.AgcRestate_Free(self.h)
            self.h = None

    def init(self, min_level, max_level, mode, fs):
        return self.L.AgcRestate_Init(self.h, min_level, max_level, mode, fs)

    def set_config(self, target, compression, limiter):
        return self.L.AgcRestate_set_config(self.h, target, compression, limiter)

    @classmethod
    def gain_table(cls, compression, target, limiter, analog_target):
        t = np.zeros(32, np.int32)
        return cls.lib().AgcRestate_gain_table(t.ctypes.data, compression, target, limiter, analog_target), t

    def frame(self, ops, x=None, far=None, level_in=0, echo=0):
        """One frame of the operations in `ops` (OP_*).  x: int16 [bands][n] or None.  Returns (rc, x after,
        VirtualMic's micLevelOut, Process's outMicLevel, saturationWarning)."""
        y, nb, n, bp = None, 1, 0, None
        if x is not None:
            y = np.ascontiguousarray(x, np.int16).copy()
            nb, n = y.shape
            bp = (C.c_void_p * nb)(*[y[b].ctypes.data for b in range(nb)])
        if far is not None:
            far = np.ascontiguousarray(far, np.int16)
            n = far.size
        vm, out, sat = I32(), I32(), U8()
        rc = self.L.AgcRestate_Frame(self.h, ops, None if far is None else far.ctypes.data, bp, nb, n, None, level_in, echo,
                                     C.byref(vm), C.byref(out), C.byref(sat))
        return rc, y, vm.value, out.value, sat.value

    @property
    def state(self):
        return self.L.AgcRestate_State(self.h).contents


def smoke_check(S=5, F=12):
    """S adaptive-analog streams x F frames on the GPU against the CPU build of the same core; True when bit-equal."""
    from .synth import agc_frames

    x = agc_frames(S, F, 160, 1)
    b = AgcBatch(S)
    ok = b.init(0, 255, 1, 16000) == 0 and b.set_mic_level(80) == 0
    y = b.process_frames(x)[0]
    b.close()
    cpu, level = Restate(), 80
    cpu.init(0, 255, 1, 16000)
    for f in range(F):
        _, want, _, level, _ = cpu.frame(OP_BY_MODE | OP_PROCESS, x[f, :, 2], level_in=level)
        ok = ok and np.array_equal(want, y[f, :, 2])
    return bool(ok)
