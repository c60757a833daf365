"""The control plane of AspAecBatch_RunList on control-only handles (no device): the ragged schedule of
tests/aec_list_cases.py through list calls against a second handle driven densely with BufferFarend + ProcessV at the
same per-stream delays.  After every tick every listed stream's control plane equals, field for field, the dense
handle's at that stream's own frame count; the stream never listed keeps its initial one; and every refusal leaves all
control planes as they were.  Needs the built library, no GPU."""
import ctypes as C

import numpy as np
import pytest

from tests.aec_list_cases import CONFIGS, DELAYS, IDLE, TOTAL, S, control_fields, control_lib, control_only, \
    run_list_control, schedule

ASP_ERR_PARAM, ASP_ERR_STATE = -1, -4  # include/asp_ns.h


def dense_history(lib, fs, n, ext, frames=TOTAL):
    """[frame count][stream] -> control fields of a handle fed `frame count` dense BufferFarend + ProcessV frames"""
    h = control_only(lib, fs, ext)
    dummy = np.zeros(S * n, np.float32)
    ms = np.asarray(DELAYS, np.int16)
    hist = [[control_fields(lib, h, s) for s in range(S)]]
    for _ in range(frames):
        assert lib.AspAecBatch_BufferFarend(h, dummy.ctypes.data, n, 1) == 0
        assert lib.AspAecBatch_ProcessV(h, dummy.ctypes.data, dummy.ctypes.data, n, ms.ctypes.data, None, None, 1) == 0
        hist.append([control_fields(lib, h, s) for s in range(S)])
    assert lib.AspAecBatch_Free(h) == 0
    return hist


@pytest.mark.parametrize("fs,n,ext", CONFIGS)
def test_ragged_list_calls_equal_dense_calls_per_stream(built_lib, fs, n, ext):
    lib = control_lib()
    hist = dense_history(lib, fs, n, ext)
    h = control_only(lib, fs, ext)
    done = np.zeros(S, int)
    for tick, (st, ct) in enumerate(schedule()):
        status = np.full(len(st), 77, np.int32)
        assert run_list_control(lib, h, st, ct, n, [DELAYS[s] for s in st], status=status) == 0, tick
        assert (status == 0).all(), (tick, status)
        done[st] += ct
        for s in range(S):
            assert control_fields(lib, h, s) == hist[done[s]][s], (tick, s, done[s])
    assert done[IDLE] == 0 and control_fields(lib, h, IDLE) == hist[0][IDLE]
    assert lib.AspAecBatch_Free(h) == 0


def test_status_is_the_or_over_an_entrys_frames(built_lib):
    """A delay outside 0 .. 500 ms: -1 for that entry alone, and its frames are processed all the same."""
    lib = control_lib()
    h, g = control_only(lib, 16000, 0), control_only(lib, 16000, 0)
    delays = np.asarray([0, 700, -3, 40], np.int16)
    status = np.zeros(4, np.int32)
    assert run_list_control(lib, h, [2, 5, 6, 8], [3, 2, 1, 0], 160, delays, status=status) == -1
    assert status.tolist() == [0, -1, -1, 0]
    for s, c, d in ((2, 3, 0), (5, 2, 700), (6, 1, -3)):  # the same frames one stream at a time on the other handle
        one = np.zeros(1, np.int32)
        assert run_list_control(lib, g, [s], [c], 160, [d], status=one) == one[0] == (0 if d == 0 else -1)
    for s in range(S):
        assert control_fields(lib, h, s) == control_fields(lib, g, s), s
    assert lib.AspAecBatch_Free(h) == 0 and lib.AspAecBatch_Free(g) == 0


def test_refusals_leave_every_control_plane_unchanged(built_lib):
    from audiosignalprocess_amd._abi import AecConfig

    err_param, err_state = ASP_ERR_PARAM, ASP_ERR_STATE
    lib = control_lib()
    h = control_only(lib, 16000, 0)
    assert run_list_control(lib, h, [1, 3, 4], [2, 1, 3], 160, [0, 20, 40]) == 0  # per-stream control, streams apart
    snap = [control_fields(lib, h, s) for s in range(S)]
    ok = dict(streams=[0, 2, 5], counts=[1, 2, 0], n=160, delays=[0, 0, 0], max_frames=2)

    def call(**kw):
        a = dict(ok, **kw)
        return run_list_control(lib, h, a["streams"], a["counts"], a["n"], a["delays"], max_frames=a["max_frames"])

    assert call(streams=[0, 2, 2]) == err_param          # listed twice
    assert call(streams=[0, 2, S]) == err_param          # outside the batch
    assert call(streams=[0, -1, 5]) == err_param
    assert call(counts=[1, 3, 0]) == err_param           # count > max_frames
    assert call(counts=[1, -1, 0]) == err_param
    assert call(n=96) == err_param                       # nrOfSamples
    assert call(max_frames=-1, counts=[0, 0, 0]) == err_param
    st = np.arange(S + 1, dtype=np.int32) % S
    z = np.zeros(S + 1, np.int16)
    d = np.zeros(4, np.float32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("h", h), ("st", st.ctypes.data), ("ct", z.astype(np.int32).ctypes.data),
                                                    ("n", 3), ("far", d.ctypes.data), ("near", d.ctypes.data),
                                                    ("out", d.ctypes.data), ("nr", 160), ("mf", 1), ("ms", z.ctypes.data),
                                                    ("status", None), ("mem", 1))]
    assert lib.AspAecBatch_RunList(*args()) == 0
    assert lib.AspAecBatch_RunList(*args(n=S + 1)) == err_param      # n > num_streams
    assert lib.AspAecBatch_RunList(*args(n=-1)) == err_param
    assert lib.AspAecBatch_RunList(*args(mem=2)) == err_param
    for null in ("st", "ct", "far", "near", "out", "ms"):
        assert lib.AspAecBatch_RunList(*args(**{null: None})) == err_param, null
    assert lib.AspAecBatch_RunList(*args(h=None)) == err_param
    assert [control_fields(lib, h, s) for s in range(S)] == snap
    # empty calls: fine, and nothing moves
    assert call(streams=[], counts=[], delays=[], max_frames=3) == 0
    assert call(counts=[0, 0, 0], max_frames=0) == 0
    assert [control_fields(lib, h, s) for s in range(S)] == snap
    assert lib.AspAecBatch_Free(h) == 0

    # the modes per-stream control refuses, and a handle that was never initialised
    for setup in ("32k", "logging", "metrics", "skew", "uninit"):
        g = C.c_void_p()
        assert lib.AspAecBatch_CreateControlOnly(C.byref(g), S) == 0
        if setup != "uninit":
            assert lib.AspAecBatch_Init(g, 32000 if setup == "32k" else 16000, 48000) == 0
        if setup == "logging":
            assert lib.AspAecBatch_set_config(g, AecConfig(1, 0, 0, 1)) == 0
        if setup == "metrics":
            assert lib.AspAecBatch_set_config(g, AecConfig(1, 0, 1, 0)) == 0
        if setup == "skew":
            assert lib.AspAecBatch_set_config(g, AecConfig(1, 1, 0, 0)) == 0
        before = control_fields(lib, g, 0)
        assert run_list_control(lib, g, [0, 2], [1, 1], 160, [0, 0]) == err_state, setup
        assert control_fields(lib, g, 0) == before, setup
        assert lib.AspAecBatch_Free(g) == 0


def test_uniform_calls_before_between_and_after_list_calls(built_lib):
    """BufferFarend + Process / ProcessV frames, list calls and InitStream on one handle equal the same frames fed
    densely: list calls of all streams by one frame are dense frames."""
    lib = control_lib()
    h, g = control_only(lib, 16000, 0), control_only(lib, 16000, 0)
    dummy = np.zeros(S * 160, np.float32)
    ms = np.asarray(DELAYS, np.int16)
    every = np.arange(S, dtype=np.int32)

    def dense(handle, uniform=None):
        assert lib.AspAecBatch_BufferFarend(handle, dummy.ctypes.data, 160, 1) == 0
        if uniform is not None:
            assert lib.AspAecBatch_Process(handle, dummy.ctypes.data, dummy.ctypes.data, 160, uniform, 0, 1) == 0
        else:
            assert lib.AspAecBatch_ProcessV(handle, dummy.ctypes.data, dummy.ctypes.data, 160, ms.ctypes.data, None, None, 1) == 0

    for f in range(8):           # lock-step frames first: the list call then moves the batch to per-stream control
        dense(h, 30)
        dense(g, 30)
    for rnd in range(3):
        assert run_list_control(lib, h, every[::-1], np.full(S, 11), 160, ms[::-1]) == 0
        for f in range(11):
            dense(g)
        if rnd == 1:
            assert lib.AspAecBatch_InitStream(h, 5) == 0 and lib.AspAecBatch_InitStream(g, 5) == 0
        dense(h)
        dense(g)
        dense(h, 35)
        dense(g, 35)
        for s in range(S):
            assert control_fields(lib, h, s) == control_fields(lib, g, s), (rnd, s)
    assert lib.AspAecBatch_Free(h) == 0 and lib.AspAecBatch_Free(g) == 0
