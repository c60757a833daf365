"""GPU tests of the AEC list calls (AspAecBatch_RunList, aec_list_kernel): some streams of a batch, each by its own
number of frames, in one launch.

The bar throughout is bit equality against a second batch driven densely with BufferFarend + ProcessV at the same
per-stream reported delays: outputs as uint32 views, every byte of every stream's exported AspAecState, every field of
its control plane.  Only the last test measures against the oracle, with the bars of
tests/test_aec_gpu.py::test_free_running_vs_oracle.  Sizes are the smallest that reach every path: nine streams (three
workgroups, the last with one live wave), per-stream delays that end the start-up phases at different frames."""
import ctypes as C

import numpy as np
import pytest

from audiosignalprocess_amd.synth import aec_frames
from tests.aec_list_cases import CONFIGS, DELAYS, IDLE, TOTAL, S, schedule

pytestmark = pytest.mark.gpu

ASP_ERR_PARAM, ASP_ERR_STATE = -1, -4  # include/asp_ns.h
SENTINEL = np.uint32(0x7FC0ABCD)       # a NaN pattern no kernel produces


@pytest.fixture(scope="module")
def aec():
    from audiosignalprocess_amd import aec as mod
    from audiosignalprocess_amd import ns

    assert ns.device_count() >= 1, "GPU tests need a HIP device"
    return mod


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frames(n, F, streams=S):
    """far, near [F][streams][n] from synth.aec_frames (160-sample frames cut in two for n = 80)"""
    far, near = aec_frames(streams, F if n == 160 else (F + 1) // 2)
    cut = lambda a: a.reshape(-1, streams, 160 // n, n).transpose(0, 2, 1, 3).reshape(-1, streams, n)[:F]
    return cut(far), cut(near)


def _batch(aec, fs, ext, streams=S):
    g = aec.AecBatch(streams, fs)
    assert g.init_rc == 0
    if ext:
        g.enable_delay_correction(1)
    return g


def _state_bytes(g, s):
    st = g.export_state(s)
    return C.string_at(C.byref(st), C.sizeof(st))


def _control(g, s):
    c = g.control_stream(s)
    return tuple(getattr(c, name) for name, _t in c._fields_)


def _snapshot(g, streams=S):
    return [(_state_bytes(g, s), _control(g, s)) for s in range(streams)]


def _assert_same(got, want, what, streams=None):
    for s in (range(len(want)) if streams is None else streams):
        assert got[s][1] == want[s][1], (what, s, "control plane")
        assert got[s][0] == want[s][0], (what, s, "exported state")


_dense_cache = {}


def dense(aec, fs, n, ext, F, delays=DELAYS):
    """The reference of these tests, computed once per configuration: F dense BufferFarend + ProcessV frames ->
    (out [F][S][n], {F: snapshot of every stream after them})."""
    key = (fs, n, ext, F, tuple(delays))
    if key not in _dense_cache:
        far, near = _frames(n, F)
        g = _batch(aec, fs, ext)
        snaps = {}
        out = np.empty((F, S, n), np.float32)
        for f in range(F):
            assert g.buffer_farend(far[f]) == 0
            out[f], status = g.process_v(near[f], delays)
            assert (status == 0).all()
        snaps[F] = _snapshot(g)
        g.close()
        out.setflags(write=False)
        _dense_cache[key] = (out, snaps)
    return _dense_cache[key]


def _sentinel(shape):
    return np.full(shape, SENTINEL, np.uint32).view(np.float32)


@pytest.mark.parametrize("fs,n,ext", [(16000, 160, 0), (16000, 80, 0), (8000, 80, 0), (16000, 160, 1)])
def test_one_list_call_of_all_streams_equals_the_dense_run(aec, fs, n, ext):
    """All nine streams, permuted, by 70 frames in ONE call: cut into nine launches, start-up ends inside it at a
    different frame per stream (16 kHz / 80 samples never leaves it, as in the reference: the pass-through path)."""
    F = 70
    want, snaps = dense(aec, fs, n, ext, F)
    far, near = _frames(n, F)
    order = np.array([4, 8, 0, 6, 2, 7, 1, 5, 3], np.int32)
    g = _batch(aec, fs, ext)
    out, status = g.run_list(order, np.full(S, F), far[:, order], near[:, order], [DELAYS[s] for s in order])
    assert (status == 0).all()
    assert np.array_equal(_bits(out), _bits(want[:, order]))
    _assert_same(_snapshot(g), snaps[F], (fs, n, ext))
    g.close()


@pytest.mark.parametrize("fs,n,ext", CONFIGS)
def test_ragged_schedule_equals_the_dense_run_per_stream(aec, fs, n, ext):
    """The schedule of tests/aec_list_cases.py: each tick lists some streams in some order with 0 .. 3 frames each.
    Every listed stream's outputs, state and control plane equal the dense run's at 120 frames; the stream never listed
    is byte-equal to a freshly initialised one; rows nobody was to write keep their sentinel."""
    want, snaps = dense(aec, fs, n, ext, TOTAL)
    far, near = _frames(n, TOTAL)
    g = _batch(aec, fs, ext)
    fresh = _snapshot(g)
    done = np.zeros(S, int)
    for tick, (st, ct) in enumerate(schedule()):
        mf = 3
        fr, nr = np.zeros((mf, len(st), n), np.float32), np.zeros((mf, len(st), n), np.float32)
        for i, (s, c) in enumerate(zip(st, ct)):
            fr[:c, i], nr[:c, i] = far[done[s]:done[s] + c, s], near[done[s]:done[s] + c, s]
        out = _sentinel((mf, len(st), n))
        _, status = g.run_list(st, ct, fr, nr, [DELAYS[s] for s in st], max_frames=mf, out=out)
        assert (status == 0).all(), tick
        for i, (s, c) in enumerate(zip(st, ct)):
            assert np.array_equal(_bits(out[:c, i]), _bits(want[done[s]:done[s] + c, s])), (tick, i, s)
            assert (_bits(out[c:, i]) == SENTINEL).all(), (tick, i, s)
            done[s] += c
    got = _snapshot(g)
    live = [s for s in range(S) if s != IDLE]
    _assert_same(got, snaps[TOTAL], (fs, n, ext), live)
    _assert_same(got, fresh, "idle stream", [IDLE])
    g.close()


@pytest.mark.parametrize("nlist", [1, 5])
def test_short_lists_and_start_up_beside_running_streams(aec, nlist):
    """n == 1 and n == 5 (the second workgroup has one live wave).  The listed streams first run ahead by 40 frames, so
    that in the last call streams past start-up (delays 0 .. 60 ms) sit beside one still in it: stream 8 is
    re-initialised before that call and leaves start-up inside it."""
    fs, n, ext, F = 16000, 160, 0, 48
    want, snaps = dense(aec, fs, n, ext, F)
    far, near = _frames(n, F)
    st = np.array([8, 2, 0, 4, 3][:nlist], np.int32)
    g = _batch(aec, fs, ext)
    d = [DELAYS[s] for s in st]
    out, _ = g.run_list(st, np.full(nlist, 40), far[:40, st], near[:40, st], d)
    assert np.array_equal(_bits(out), _bits(want[:40, st]))
    out, _ = g.run_list(st, np.full(nlist, 8), far[40:, st], near[40:, st], d)
    assert np.array_equal(_bits(out), _bits(want[40:, st]))
    _assert_same(_snapshot(g), snaps[F], nlist, st.tolist())
    if nlist == 5:  # start-up beside running streams in one launch
        g.init_stream(8)
        gd = _batch(aec, fs, ext)   # dense twin: everything by 48 frames, then stream 8 again from its Init
        for f in range(F):
            gd.buffer_farend(far[f])
            gd.process_v(near[f], DELAYS)
        gd.init_stream(8)
        wd = np.empty((8, S, n), np.float32)
        for f in range(8):
            gd.buffer_farend(far[f])
            wd[f], _ = gd.process_v(near[f], DELAYS)
        cnt = np.full(5, 8, np.int32)   # stream 8 leaves start-up at its sixth frame: pass-through, then processing
        assert _control(g, 8)[0] == 1 and all(_control(g, s)[0] == 0 for s in (2, 0, 4, 3))
        out, _ = g.run_list(st, cnt, far[:8, st], near[:8, st], d)
        assert _control(g, 8)[0] == 0
        assert np.array_equal(_bits(out), _bits(wd[:, st]))
        _assert_same(_snapshot(g), _snapshot(gd), "start-up beside running", st.tolist())
        gd.close()
    g.close()


def test_uniform_calls_init_stream_and_process_v_between_list_calls(aec):
    """On one batch, in sequence: lock-step buffer_farend + process frames, list calls, init_stream(5) between two
    list calls, a ProcessV frame, more list calls -- with a delay jump, an out-of-range delay (700: status -1) and a
    negative one at call boundaries.  The dense batch does the same frames with BufferFarend + ProcessV."""
    fs, n, F = 16000, 160, 64
    far, near = _frames(n, F)
    g, gd = _batch(aec, fs, 0), _batch(aec, fs, 0)
    every = np.arange(S, dtype=np.int32)
    pos = [0]

    def dense_frames(count, delays):
        out = np.empty((count, S, n), np.float32)
        st = np.zeros(S, np.int32)
        for k in range(count):
            f = pos[0] + k
            assert gd.buffer_farend(far[f]) == 0
            out[k], s1 = gd.process_v(near[f], delays)
            st |= s1
        return out, st

    def both_equal(what):
        _assert_same(_snapshot(g), _snapshot(gd), what)

    for k in range(6):                                # lock-step frames first, on both
        o1, rc1 = g.frame(far[k], near[k], 30)
        o2, rc2 = gd.frame(far[k], near[k], 30)
        assert rc1 == rc2 == 0 and np.array_equal(_bits(o1), _bits(o2))
    pos[0] = 6
    steps = [("list", 20, list(DELAYS)),
             ("list", 7, [90 if s == 1 else DELAYS[s] for s in range(S)]),            # a delay jump on stream 1
             ("init", 5, None),
             ("list", 9, [700 if s == 4 else DELAYS[s] for s in range(S)]),           # out of range: -1, still processes
             ("v", 1, list(DELAYS)),
             ("list", 12, [-5 if s == 7 else DELAYS[s] for s in range(S)]),           # negative: -1
             ("list", 9, list(DELAYS))]
    for kind, count, delays in steps:
        if kind == "init":
            g.init_stream(count)
            gd.init_stream(count)
            continue
        want, st_want = dense_frames(count, delays)
        f0 = pos[0]
        if kind == "v":
            assert g.buffer_farend(far[f0]) == 0
            out, status = g.process_v(near[f0], delays)
            out = out[None]
        else:
            order = every[::-1] if count % 2 else every
            out_l, st_l = g.run_list(order, np.full(S, count), far[f0:f0 + count][:, order], near[f0:f0 + count][:, order],
                                     [delays[s] for s in order])
            out, status = np.empty_like(want), np.zeros(S, np.int32)
            out[:, order], status[order] = out_l, st_l
        assert np.array_equal(status, st_want), (kind, count, status, st_want)
        assert np.array_equal(_bits(out), _bits(want)), (kind, count)
        pos[0] += count
        both_equal((kind, count))
    assert pos[0] == F
    g.close()
    gd.close()


def test_device_calls_back_to_back_outrun_the_descriptor_ring(aec):
    """Six device-buffer list calls enqueued without a synchronise -- more than the four descriptor slots -- equal the
    same calls with a synchronise after each."""
    from audiosignalprocess_amd.ns import DeviceBuffer

    fs, n, calls, per = 16000, 160, 6, 5
    F = calls * per
    far, near = _frames(n, F)
    order = np.array([3, 0, 8, 5, 1, 7, 2, 6, 4], np.int32)
    d = [DELAYS[s] for s in order]
    outs, snaps = [], []
    for sync_each in (False, True):
        g = _batch(aec, fs, 0)
        dfar, dnear, dout = (DeviceBuffer(F * S * n * 4) for _ in range(3))
        dfar.upload(far[:, order])
        dnear.upload(near[:, order])
        dout.upload(_sentinel((F, S, n)))
        for k in range(calls):
            cnt = np.full(S, per, np.int32)
            cnt[k % S] = per - 2       # a shorter entry: its last rows keep the sentinel
            off = k * per * S * n * 4
            status = g.run_list_device(order, cnt, dfar.ptr + off, dnear.ptr + off, dout.ptr + off, n, per, d)
            assert (status == 0).all()
            if sync_each:
                g.synchronize()
        g.synchronize()
        outs.append(dout.download((F, S, n)))
        snaps.append(_snapshot(g))
        g.close()
        for b in (dfar, dnear, dout):
            b.free()
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert (_bits(outs[0]) == SENTINEL).sum() == calls * 2 * n
    _assert_same(snaps[0], snaps[1], "back to back")


def test_in_place_and_host_memory_equal_separate_device_buffers(aec):
    from audiosignalprocess_amd.ns import DeviceBuffer

    fs, n, F = 16000, 160, 11     # more than one launch
    far, near = _frames(n, F)
    order = np.array([6, 1, 8, 3, 0], np.int32)
    cnt = np.array([11, 4, 0, 9, 11], np.int32)
    d = [DELAYS[s] for s in order]
    fr, nr = np.ascontiguousarray(far[:, order]), np.ascontiguousarray(near[:, order])
    results = {}
    for form in ("device", "device in place", "host", "host in place"):
        g = _batch(aec, fs, 0)
        if form.startswith("device"):
            dfar, dnear, dout = (DeviceBuffer(fr.nbytes) for _ in range(3))
            dfar.upload(fr)
            dnear.upload(nr)
            dout.upload(_sentinel(nr.shape))
            target = dnear if form.endswith("in place") else dout
            g.run_list_device(order, cnt, dfar.ptr, dnear.ptr, target.ptr, n, F, d)
            g.synchronize()
            out = target.download(nr.shape)
            for b in (dfar, dnear, dout):
                b.free()
        elif form == "host":
            out, _ = g.run_list(order, cnt, fr, nr, d, out=_sentinel(nr.shape))
        else:
            buf = nr.copy()
            out, _ = g.run_list(order, cnt, fr, buf, d, out=buf)
            assert out is buf
        results[form] = (out, _snapshot(g))
        g.close()
    ref_out, ref_snap = results["device"]
    written = np.arange(F)[:, None] < cnt[None, :]
    assert (_bits(ref_out)[~written] == SENTINEL).all()
    for form, (out, snap) in results.items():
        assert np.array_equal(_bits(out)[written], _bits(ref_out)[written]), form
        untouched = _bits(nr) if form.endswith("in place") else np.full(nr.shape, SENTINEL, np.uint32)
        assert np.array_equal(_bits(out)[~written], untouched[~written]), form
        _assert_same(snap, ref_snap, form)


def test_refusals_return_the_documented_code_and_leave_the_batch_alone(aec):
    """A refused call changes nothing: the continuation equals that of a batch that never saw it."""
    fs, n, F = 16000, 160, 24
    far, near = _frames(n, F)
    every = np.arange(S, dtype=np.int32)
    g, gd = _batch(aec, fs, 0), _batch(aec, fs, 0)
    for b in (g, gd):
        b.run_list(every, np.full(S, 12), far[:12], near[:12], DELAYS)
    lib, dummy = g.lib, np.zeros((2, 3, n), np.float32)
    z16 = np.zeros(3, np.int16)

    def raw(streams, counts, farp=dummy.ctypes.data, mf=2, h=None):
        st, ct = np.asarray(streams, np.int32), np.asarray(counts, np.int32)
        return lib.AspAecBatch_RunList(h or g.h, st.ctypes.data, ct.ctypes.data, len(st), farp, dummy.ctypes.data,
                                       dummy.ctypes.data, n, mf, z16.ctypes.data, None, 0)

    assert raw([1, 4, 1], [1, 1, 1]) == ASP_ERR_PARAM      # a duplicate stream
    assert raw([1, 4, S], [1, 1, 1]) == ASP_ERR_PARAM      # a stream outside the batch
    assert raw([1, 4, 2], [1, 3, 1]) == ASP_ERR_PARAM      # count > max_frames
    assert raw([1, 4, 2], [1, 1, 1], farp=None) == ASP_ERR_PARAM
    _assert_same(_snapshot(g), _snapshot(gd), "after refusals")
    o1, s1 = g.run_list(every, np.full(S, 12), far[12:], near[12:], DELAYS)
    o2, s2 = gd.run_list(every, np.full(S, 12), far[12:], near[12:], DELAYS)
    assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(s1, s2)
    _assert_same(_snapshot(g), _snapshot(gd), "continuation")
    g.close()
    gd.close()
    # the modes per-stream control refuses
    for fs_, logging in ((16000, 1), (32000, 0)):
        a, b = aec.AecBatch(3, fs_), aec.AecBatch(3, fs_)
        if logging:
            assert a.set_config(1, delay_logging=1) == 0 and b.set_config(1, delay_logging=1) == 0
        assert raw([0, 1, 2], [1, 1, 1], h=a.h) == ASP_ERR_STATE
        if fs_ == 16000:   # the continuation (lock-step frames with delay logging on) equals the untouched batch's
            for k in range(3):
                oa, ra = a.frame(far[k, :3], near[k, :3], 0)
                ob, rb = b.frame(far[k, :3], near[k, :3], 0)
                assert ra == rb and np.array_equal(_bits(oa), _bits(ob))
            assert _state_bytes(a, 1) == _state_bytes(b, 1)
        a.close()
        b.close()


def test_ragged_run_against_one_oracle_per_stream(aec):
    """Four streams x 120 frames through ragged list calls against one OracleAec per stream, with the bars of
    test_free_running_vs_oracle: control plane equal, LINEAR_FIELDS bit-exact, outputs within 1e-5 relative L2."""
    from tests.oracle_lib import OracleAec
    from tests.test_aec_gpu import LINEAR_FIELDS, _rel_l2, _state_report

    n, Sx, F = 160, 4, 120
    far, near = _frames(n, F, Sx)
    delays = [0, 20, 60, 100]
    g = aec.AecBatch(Sx, 16000)
    oras = [OracleAec(16000) for _ in range(Sx)]
    out_o = np.empty((F, Sx, n), np.float32)
    for s in range(Sx):
        for f in range(F):
            out_o[f, s], rc = oras[s].frame(far[f, s], near[f, s], delays[s])
            assert rc == 0
    out_g = np.empty_like(out_o)
    rng = np.random.RandomState(7)
    done = np.zeros(Sx, int)
    while (done < F).any():
        st = rng.permutation([s for s in range(Sx) if done[s] < F]).astype(np.int32)
        ct = np.array([min(int(rng.choice([0, 1, 2, 3, 11])), F - done[s]) for s in st], np.int32)
        mf = max(int(ct.max()), 1)
        fr, nr = np.zeros((mf, len(st), n), np.float32), np.zeros((mf, len(st), n), np.float32)
        for i, (s, c) in enumerate(zip(st, ct)):
            fr[:c, i], nr[:c, i] = far[done[s]:done[s] + c, s], near[done[s]:done[s] + c, s]
        out, status = g.run_list(st, ct, fr, nr, [delays[s] for s in st], max_frames=mf)
        assert (status == 0).all()
        for i, (s, c) in enumerate(zip(st, ct)):
            out_g[done[s]:done[s] + c, s] = out[:c, i]
            done[s] += c
    for s in range(Sx):
        st_o, co = oras[s].export()
        cg = g.control_stream(s)
        for name, _t in cg._fields_:
            assert getattr(cg, name) == getattr(co, name), (s, name)
        rep = _state_report(g.export_state(s), st_o)
        bad = [k for k in LINEAR_FIELDS if not rep[k][0]]
        assert bad == [], (s, {k: rep[k] for k in bad})
        assert _rel_l2(out_g[:, s], out_o[:, s]) <= 1e-5, s
    g.close()
