"""The ragged schedule of the AEC list-call tests (AspAecBatch_RunList): which streams a tick lists, in which order,
with how many frames each, and each stream's reported delay.  Kept apart from the GPU test so that the CPU suite checks
its shape and drives the control plane over it (tests/test_aec_list_schedule.py, test_aec_list_control.py,
test_aec_list_control_host.py)."""
import ctypes as C

import numpy as np

S = 9
TOTAL, IDLE = 120, 7  # every stream but IDLE ends at 120 frames; IDLE is never listed
DELAYS = [0, 0, 20, 40, 60, 100, 5, 250, 30]  # ms, per stream
# (fs, samples per call, extended filter)
CONFIGS = [(16000, 160, 0), (8000, 80, 0), (16000, 160, 1)]


def schedule():
    """[(streams, counts)] per tick, fixed seed: each listed stream gets 0..3 frames, the order changes from tick to tick."""
    rng = np.random.RandomState(20241021)
    left = {s: TOTAL for s in range(S) if s != IDLE}
    ticks = [(np.array([5], np.int32), np.array([1], np.int32))]  # a tick with n == 1
    left[5] -= 1
    while any(left.values()):
        streams, counts = [], []
        for s in rng.permutation([s for s in left if left[s]]):
            c = min(int(rng.choice([0, 1, 1, 1, 2, 3])), left[s])
            if c == 0 and rng.rand() < 0.5:
                continue  # no frame: sometimes not listed, sometimes listed with count 0
            streams.append(s)
            counts.append(c)
            left[s] -= c
        if streams:
            ticks.append((np.array(streams, np.int32), np.array(counts, np.int32)))
    return ticks


def control_lib():
    """The library with the control-only constructor declared (no device is touched through it)."""
    from audiosignalprocess_amd import aec as aec_mod

    lib = aec_mod._lib()
    lib.AspAecBatch_CreateControlOnly.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    return lib


def control_only(lib, fs, ext, streams=S):
    h = C.c_void_p()
    assert lib.AspAecBatch_CreateControlOnly(C.byref(h), streams) == 0
    assert lib.AspAecBatch_Init(h, fs, 48000) == 0
    if ext:
        assert lib.AspAecBatch_enable_delay_correction(h, 1) == 0
    return h


def control_fields(lib, h, s):
    from audiosignalprocess_amd._abi import AspAecControl

    c = AspAecControl()
    assert lib.AspAecBatch_GetControlStream(h, s, C.byref(c)) == 0
    return tuple(getattr(c, name) for name, _t in c._fields_)


def run_list_control(lib, h, streams, counts, n, delays, max_frames=None, status=None):
    """AspAecBatch_RunList on a control-only handle: the buffers are checked for NULL only."""
    streams = np.ascontiguousarray(streams, np.int32)
    counts = np.ascontiguousarray(counts, np.int32)
    ms = np.ascontiguousarray(delays, np.int16)
    if max_frames is None:
        max_frames = int(counts.max()) if len(counts) else 0
    dummy = np.zeros(4, np.float32)
    return lib.AspAecBatch_RunList(h, streams.ctypes.data, counts.ctypes.data, len(streams), dummy.ctypes.data,
                                   dummy.ctypes.data, dummy.ctypes.data, n, max_frames, ms.ctypes.data,
                                   None if status is None else status.ctypes.data, 1)
