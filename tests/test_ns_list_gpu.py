"""AspNsBatch_AnalyzeProcessList: SOME streams of an NS batch advance, each by its own number of frames (the list form
of the pair-layout hand-off step, ns_kernels1.hip ns_list1_kernel).  The pin is bitwise: whatever order, grouping and
raggedness the list calls have, every stream's outputs and final state are those of a lock-step batch fed the same
frames per stream; streams that are not listed, and entries with count 0, are untouched; nothing of `out` beyond
counts[i] is written; the hand-off build's counters are left alone, so lock-step calls go on before and after.  One run
against the oracle guards the far end of that chain.  Small batches on purpose: 9 streams are three workgroups, the
last with one live wave."""
import ctypes as C

import numpy as np
import pytest

from audiosignalprocess_amd._abi import MEM_DEVICE, MEM_HOST
from audiosignalprocess_amd.synth import ns_frames
from tests.conftest import state_diff
from tests.ns_list_cases import IDLE, TOTAL, schedule

pytestmark = pytest.mark.gpu

S = 9
PERM = np.array([4, 0, 8, 2, 6, 1, 7, 3, 5], np.int32)
SENTINEL = np.uint32(0x7FC12345)  # a NaN no frame step produces
ERR_PARAM, ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def ns():
    from audiosignalprocess_amd import ns as mod

    assert mod.device_count() >= 1, "GPU tests need a HIP device"
    return mod


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _states(g, streams=None):
    return [g.export_state(s) for s in (range(g.S) if streams is None else streams)]


def _sentinel_like(x):
    out = np.empty(x.shape, x.dtype)
    out.view(np.uint32 if x.dtype == np.float32 else np.uint16)[...] = SENTINEL if x.dtype == np.float32 else 0x7FC1
    return out


# ---------------------------------------------------------------- 1. all streams, permuted
@pytest.fixture(scope="module")
def frames70():
    return {False: ns_frames(S, 70), True: _with_silent(ns_frames(S, 70), 3)}


def _with_silent(x, s):
    x = x.copy()
    x[:, s] = 0.0
    return x


@pytest.fixture(scope="module")
def lockstep70(ns, frames70):
    """Batch A: lock-step analyze_process of the 70 frames (they cross blockInd 50), computed once per input."""
    ref = {}
    for silent, x in frames70.items():
        a = ns.NsBatch(S, policy=1)
        y = a.analyze_process(x)
        ref[silent] = (y, _states(a))
        a.close()
    assert not ref[True][0][:, 3].any() and ref[True][1][3].blockInd == -1 and ref[False][1][3].blockInd == 69
    return ref


@pytest.mark.parametrize("variant", ["plain", "stream3_silent", "steady_off"])
def test_one_list_call_of_all_streams_permuted_equals_lockstep(ns, frames70, lockstep70, variant):
    silent = variant == "stream3_silent"
    x, (want, want_states) = frames70[silent], lockstep70[silent]
    b = ns.NsBatch(S, policy=1)
    if variant == "steady_off":
        b.set_steady(0)
    y = b.analyze_process_list(PERM, None, x[:, PERM])  # 70 frames: launches of 64 + 6
    assert np.array_equal(_u32(y), _u32(want[:, PERM]))
    for s, st in enumerate(_states(b)):
        assert state_diff(st, want_states[s]) == {}, s
    b.close()


# ---------------------------------------------------------------- 2. ragged schedule
def test_ragged_schedule_equals_lockstep_per_stream(ns):
    x = ns_frames(S, TOTAL, stream0=3)
    a = ns.NsBatch(S, policy=1)
    want = a.analyze_process(x)
    want_states = _states(a)
    a.close()
    fresh = ns.NsBatch(S, policy=1)
    fresh_idle = fresh.export_state(IDLE)
    fresh.close()

    b = ns.NsBatch(S, policy=1)
    pos = np.zeros(S, int)
    got = np.zeros_like(want)
    for streams, counts in schedule():
        n = len(streams)
        fr = np.zeros((3, n, 160), np.float32)
        for i, (s, c) in enumerate(zip(streams, counts)):
            fr[:c, i] = x[pos[s]:pos[s] + c, s]
            fr[c:, i] = 12345.0  # frames beyond the count must not be read either: they would change the state
        out = _sentinel_like(fr)
        b.analyze_process_list(streams, counts, fr, out=out)
        for i, (s, c) in enumerate(zip(streams, counts)):
            assert (_u32(out[c:, i]) == SENTINEL).all(), (s, c)
            got[pos[s]:pos[s] + c, s] = out[:c, i]
            pos[s] += c
    for s in range(S):
        if s == IDLE:
            assert state_diff(b.export_state(s), fresh_idle) == {}
            continue
        assert pos[s] == TOTAL
        assert np.array_equal(_u32(got[:, s]), _u32(want[:, s])), s
        assert state_diff(b.export_state(s), want_states[s]) == {}, s
    b.close()


# ---------------------------------------------------------------- 3. mixed with the existing entry points
LIST1 = (np.array([1, 2, 4, 6], np.int32), np.array([2, 1, 3, 0], np.int32))
LIST2 = (np.array([4, 2, 0, 8, 3], np.int32), np.array([2, 3, 1, 2, 0], np.int32))


def _list_frames(x, pos, streams, counts, max_frames):
    fr = np.zeros((max_frames, len(streams), 160), np.float32)
    for i, (s, c) in enumerate(zip(streams, counts)):
        fr[:c, i] = x[pos[s]:pos[s] + c, s]
    return fr


def test_list_calls_between_lockstep_handoff_calls_on_one_batch(ns):
    x = ns_frames(S, 16, stream0=11)
    g = ns.NsBatch(S, policy=1)
    g.set_flow(1)
    pos = np.zeros(S, int)
    got = [[] for _ in range(S)]

    def lockstep(n):
        fr = np.stack([x[pos[s]:pos[s] + n, s] for s in range(S)], axis=1)
        y = g.analyze_process(fr)
        for s in range(S):
            got[s].append(y[:, s])
            pos[s] += n

    def listed(streams, counts):
        out = g.analyze_process_list(streams, counts, _list_frames(x, pos, streams, counts, 3))
        for i, (s, c) in enumerate(zip(streams, counts)):
            got[s].append(out[:c, i])
            pos[s] += c

    lockstep(5)                      # 1. hand-off call, flow on
    listed(*LIST1)                   # 2.
    g.init_stream(2)                 # 3.
    g.set_policy_stream(4, 2)
    listed(*LIST2)                   # 4. includes streams 2 and 4
    lockstep(3)                      # 5. hand-off call again: seq[] is where call 1 left it
    g.synchronize()                  # 6. raises on a hand-off timeout
    states = _states(g)
    g.close()

    # one reference batch per distinct history (frames of list call 1, of list call 2): lock-step calls only, flow off
    c1 = dict(zip(LIST1[0].tolist(), LIST1[1].tolist()))
    c2 = dict(zip(LIST2[0].tolist(), LIST2[1].tolist()))
    groups = {}
    for s in range(S):
        groups.setdefault((c1.get(s, 0), c2.get(s, 0)), []).append(s)
    assert len(groups) >= 5
    for (n1, n2), members in groups.items():
        r = ns.NsBatch(S, policy=1)
        r.set_flow(0)
        at, outs = 0, []
        for k, n in enumerate((5, n1, n2, 3)):
            if k == 2:
                r.init_stream(2)
                r.set_policy_stream(4, 2)
            if n:
                outs.append(r.analyze_process(x[at:at + n]))
                at += n
        y = np.concatenate(outs)
        for s in members:
            assert at == pos[s]
            assert np.array_equal(_u32(np.concatenate(got[s])), _u32(y[:, s])), s
            assert state_diff(states[s], r.export_state(s)) == {}, s
        r.close()


# ---------------------------------------------------------------- 4. back-to-back enqueue
CALLS3 = [(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8], np.int32), np.array([2, 0, 1, 3, 1, 1, 2, 0, 3], np.int32)),
          (np.array([8, 3, 5], np.int32), np.array([1, 3, 2], np.int32)),
          (np.array([6, 0, 7, 2, 8, 1], np.int32), None)]


def _three_device_calls(ns, x, sync_between):
    from audiosignalprocess_amd.ns import DeviceBuffer

    g = ns.NsBatch(S, policy=1)
    pos = np.zeros(S, int)
    bufs, shapes = [], []
    for streams, counts in CALLS3:
        cts = counts if counts is not None else np.full(len(streams), 3, np.int32)
        fr = _list_frames(x, pos, streams, cts, 3)
        pos[streams] += cts
        din, dout = DeviceBuffer(fr.nbytes), DeviceBuffer(fr.nbytes)
        din.upload(fr)
        dout.upload(_sentinel_like(fr))
        bufs.append((din, dout))
        shapes.append(fr.shape)
    for (streams, counts), (din, dout) in zip(CALLS3, bufs):
        # the lists are temporaries that are overwritten right after the call: the batch must have taken its own copy
        st = streams.copy()
        ct = None if counts is None else counts.copy()
        g.analyze_process_list_device(st, ct, din.ptr, dout.ptr, 3)
        st[...] = 0
        if ct is not None:
            ct[...] = 3
        if sync_between:
            g.synchronize()
    g.synchronize()
    outs = [dout.download(shape) for (_, dout), shape in zip(bufs, shapes)]
    states = _states(g)
    g.close()
    return outs, states


def test_three_list_calls_enqueued_back_to_back_each_see_their_own_list(ns):
    x = ns_frames(S, 12, stream0=20)
    outs, states = _three_device_calls(ns, x, sync_between=False)
    want, want_states = _three_device_calls(ns, x, sync_between=True)
    for k in range(3):
        assert np.array_equal(_u32(outs[k]), _u32(want[k])), k
        assert (_u32(outs[k]) != SENTINEL).any()
    counts0 = CALLS3[0][1]
    for i, c in enumerate(counts0):
        assert (_u32(outs[0][c:, i]) == SENTINEL).all() and (_u32(outs[0][:c, i]) != SENTINEL).all(), i
    for s in range(S):
        assert state_diff(states[s], want_states[s]) == {}, s
    assert states[0].blockInd == 2 + 3 - 1 and states[4].blockInd == 0


# ---------------------------------------------------------------- 5. I/O forms
def test_in_place_on_device_and_host_memory_equal_separate_device_buffers(ns):
    from audiosignalprocess_amd.ns import DeviceBuffer

    x = ns_frames(S, 6, stream0=30)
    streams = np.array([7, 2, 5, 0, 3], np.int32)
    counts = np.array([3, 0, 2, 1, 3], np.int32)
    fr = _list_frames(x, np.zeros(S, int), streams, counts, 3)

    def device(in_place):
        g = ns.NsBatch(S, policy=1)
        din, dout = DeviceBuffer(fr.nbytes), DeviceBuffer(fr.nbytes)
        din.upload(fr)
        dout.upload(fr)
        g.analyze_process_list_device(streams, counts, din.ptr, din.ptr if in_place else dout.ptr, 3)
        g.synchronize()
        y = (din if in_place else dout).download(fr.shape)
        st = _states(g)
        g.close()
        return y, st

    sep, sep_states = device(False)
    inp, inp_states = device(True)
    h = ns.NsBatch(S, policy=1)
    host = h.analyze_process_list(streams, counts, fr)  # ASP_MEM_HOST; frames beyond the counts keep the input
    host_states = _states(h)
    h.close()
    assert np.array_equal(_u32(inp), _u32(sep)) and np.array_equal(_u32(host), _u32(sep))
    assert (_u32(sep[0, 0]) != _u32(fr[0, 0])).any() and np.array_equal(_u32(sep[:, 1]), _u32(fr[:, 1]))
    for s in range(S):
        assert state_diff(inp_states[s], sep_states[s]) == {} and state_diff(host_states[s], sep_states[s]) == {}, s


def test_s16_list_form_equals_lockstep_s16(ns):
    pcm = np.rint(ns_frames(S, 14, stream0=50)).astype(np.int16)
    a = ns.NsBatch(S, policy=1)
    want = a.analyze_process_s16(pcm)
    want_states = _states(a)
    a.close()
    b = ns.NsBatch(S, policy=1)
    # two ragged calls: 9 of each stream's 14 frames (fewer for some) in the first, the rest in the second
    first = np.array([9, 3, 0, 9, 5, 1, 9, 7, 2], np.int32)
    pos = np.zeros(S, int)
    got = np.zeros_like(want)
    for counts in (first, 14 - first):
        streams = PERM
        cts = counts[streams]
        fr = np.zeros((14, S, 160), np.int16)
        for i, (s, c) in enumerate(zip(streams, cts)):
            fr[:c, i] = pcm[pos[s]:pos[s] + c, s]
        out = _sentinel_like(fr)
        b.analyze_process_list(streams, cts, fr, out=out)
        for i, (s, c) in enumerate(zip(streams, cts)):
            assert (out[c:, i].view(np.uint16) == 0x7FC1).all(), s
            got[pos[s]:pos[s] + c, s] = out[:c, i]
            pos[s] += c
    assert np.array_equal(got, want)
    for s in range(S):
        assert state_diff(b.export_state(s), want_states[s]) == {}, s
    b.close()


# ---------------------------------------------------------------- 6. the oracle, directly
def test_ragged_run_against_the_oracle(ns):
    """smoke()'s criterion: per-stream relative L2 <= 1e-4 against the oracle with the kernel's association."""
    from tests.oracle_lib import REDUCE_TREE64P, OracleNs

    n, total = 4, 120
    x = ns_frames(n, total, stream0=70)
    ref = OracleNs(n, policy=1, reduce_mode=REDUCE_TREE64P).run(x)
    g = ns.NsBatch(n, policy=1)
    rng = np.random.RandomState(7)
    pos = np.zeros(n, int)
    got = np.zeros_like(ref)
    while (pos < total).any():
        streams = rng.permutation(n).astype(np.int32)
        counts = np.minimum(rng.randint(0, 4, n), total - pos[streams]).astype(np.int32)
        out = g.analyze_process_list(streams, counts, _list_frames(x, pos, streams, counts, 3))
        for i, (s, c) in enumerate(zip(streams, counts)):
            got[pos[s]:pos[s] + c, s] = out[:c, i]
            pos[s] += c
    g.close()
    num = np.sqrt(((got - ref).astype(np.float64) ** 2).sum(axis=(0, 2)))
    den = np.sqrt((ref.astype(np.float64) ** 2).sum(axis=(0, 2)))
    rel = num / den
    print("list form against the oracle, per-stream rel-L2:", rel)
    assert np.isfinite(rel).all() and (rel <= 1e-4).all(), rel


# ---------------------------------------------------------------- 7. refusals
def _raw_call(ns, h, streams, counts, n, in_p, out_p, max_frames, mem, s16=False):
    lib = ns.load_library()
    fn = lib.AspNsBatch_AnalyzeProcessListS16 if s16 else lib.AspNsBatch_AnalyzeProcessList
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = fn(h, p(streams), p(counts), n, p(in_p), p(out_p), max_frames, mem)
    return rc, lib.AspNs_last_error().decode()


I32 = lambda *v: np.array(v, np.int32)  # noqa: E731


def test_refusals_leave_the_batch_as_it_was(ns):
    x = ns_frames(S, 4, stream0=90)
    fr = np.ascontiguousarray(x[:3, :4])
    out = np.zeros_like(fr)
    ok_streams, ok_counts = I32(0, 5, 2, 8), I32(1, 2, 3, 0)
    PROBES = (0, 5)

    def refused(g, want_rc, *args, **kw):
        before = _states(g, PROBES)
        rc, why = _raw_call(ns, g.h, *args, **kw)
        assert rc == want_rc and why, (rc, why, args[2:])
        for p, st0, st1 in zip(PROBES, before, _states(g, PROBES)):
            assert state_diff(st1, st0) == {}, (why, p)

    g = ns.NsBatch(S, policy=1)
    g.analyze_process(x[:2])  # (some history, so that an accidental step shows)
    for args in [
        (None, ok_counts, 4, fr, out, 3, MEM_HOST),                 # null list
        (ok_streams, ok_counts, 4, None, out, 3, MEM_HOST),         # null in
        (ok_streams, ok_counts, 4, fr, None, 3, MEM_HOST),          # null out
        (ok_streams, ok_counts, -1, fr, out, 3, MEM_HOST),          # n < 0
        (np.arange(S + 1, dtype=np.int32), None, S + 1, fr, out, 3, MEM_HOST),  # n > num_streams
        (I32(0, -1, 2, 8), ok_counts, 4, fr, out, 3, MEM_HOST),     # index < 0
        (I32(0, S, 2, 8), ok_counts, 4, fr, out, 3, MEM_HOST),      # index == num_streams
        (I32(0, 5, 2, 5), ok_counts, 4, fr, out, 3, MEM_HOST),      # duplicate
        (ok_streams, I32(1, -1, 3, 0), 4, fr, out, 3, MEM_HOST),    # count < 0
        (ok_streams, I32(1, 2, 4, 0), 4, fr, out, 3, MEM_HOST),     # count > max_frames
        (ok_streams, ok_counts, 4, fr, out, 3, 2),                  # bad mem
    ]:
        refused(g, ERR_PARAM, *args)
        refused(g, ERR_PARAM, *args, s16=True)
    # switches that the list form does not serve
    for kernel in (1, 2):
        g.set_kernel(kernel)
        refused(g, ERR_STATE, ok_streams, ok_counts, 4, fr, out, 3, MEM_HOST)
        g.set_kernel(0)
    g.debug_step_counts(True)
    refused(g, ERR_STATE, ok_streams, ok_counts, 4, fr, out, 3, MEM_HOST)
    g.debug_step_counts(False)
    # a following valid call still works: equal to the same call on a batch that refused nothing
    y = g.analyze_process_list(ok_streams, ok_counts, fr)
    c = ns.NsBatch(S, policy=1)
    c.analyze_process(x[:2])
    want = c.analyze_process_list(ok_streams, ok_counts, fr)
    assert np.array_equal(_u32(y), _u32(want)) and (_u32(y[0, 0]) != _u32(fr[0, 0])).any()
    for s in range(S):
        assert state_diff(g.export_state(s), c.export_state(s)) == {}, s
    c.close()
    # the unpaired representation (after a two-call Analyze / Process): refused as AnalyzeProcessReplay refuses it
    g.analyze(x[3])
    g.process(x[3])
    refused(g, ERR_STATE, ok_streams, ok_counts, 4, fr, out, 3, MEM_HOST)
    g.close()

    # other geometries
    for fs in (8000, 32000, 48000):
        w = ns.NsBatch(S, fs=fs, policy=1)
        refused(w, ERR_STATE, ok_streams, ok_counts, 4, fr, out, 3, MEM_HOST)
        w.close()
    # a batch that was never initialised
    lib = ns.load_library()
    h = C.c_void_p()
    assert lib.AspNsBatch_Create(C.byref(h), S, 0) == 0
    rc, why = _raw_call(ns, h, ok_streams, ok_counts, 4, fr, out, 3, MEM_HOST)
    assert rc == ERR_STATE and why
    lib.AspNsBatch_Free(h)
    # nothing to do is not an error
    g = ns.NsBatch(S, policy=1)
    assert _raw_call(ns, g.h, ok_streams, ok_counts, 0, fr, out, 3, MEM_HOST)[0] == 0
    assert _raw_call(ns, g.h, ok_streams, I32(0, 0, 0, 0), 4, fr, out, 0, MEM_DEVICE)[0] == 0
    g.close()
