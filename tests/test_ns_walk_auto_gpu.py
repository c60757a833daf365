"""The automatic walk length of the NS hand-off build (ns_api.hip, flow_walk_auto): a batch with at least one workgroup
(four streams) per compute unit of its device walks LONG_WALK steps per workgroup, a smaller one 4.  Whatever the length,
outputs and state must equal, bit for bit, what the plain launches (set_flow(0)) of the same kernel give.

1. The long walk, forced on the 5-stream, ring-3, 1030-frame schedule of test_ns_resident_gpu.py (calls of 37, 160,
   301, 501 and 31 frames, one silent stream, one that falls silent): the walks the policy can return that the
   existing files do not force (they cover 1, 2, 3, 4, 7 and 64): 8.  With walks of 8 and more that schedule puts the
   start-up boundaries (frames 50 and 200) and the first window close (frame 499) on MIDDLE steps of a walk and the
   second close (frame 999) on a walk's FIRST step; a close on a walk's LAST step it gives to walks of 2 only (frame
   499 is the second step of its launch).  A second schedule of the same 1030 frames -- calls of 436, 500 and 94 --
   therefore puts both closes on the 64th step of a launch: the last step of a walk of 8, 16 or 32.  Both are
   asserted below with the position arithmetic of test_ns_resident_gpu.py.
2. Auto on a device-filling, ragged batch (4100 streams: 1025 workgroups of four streams, the last one with four live
   waves but the grid padded to 1032), a call of 64 steps and one of 23: bit-equal to the plain launches, and the last
   launch goes out as ceil(23 / W) chunks, W from the published rule (include/asp_ns.h, AspNsBatch_SetFlowWalk; the
   comment above flow_walk_auto in ns_api.hip) evaluated on the device under test.
3. Two such batches enqueued before either is waited for."""
import ctypes as C

import numpy as np
import pytest

from audiosignalprocess_amd.synth import ns_frames
from tests.conftest import state_diff

gpu = pytest.mark.gpu

SHORT_WALK, LONG_WALK, MAX_LAUNCH = 4, 8, 64   # ns_api.hip: kFlowWalkShort, kFlowWalkLong; handoff_host.h: kHandoffMaxSteps
NEW_WALKS = (LONG_WALK,)                        # what the policy can return and no earlier file forces
S, RING = 5, 3
SCHEDULES = {"resident": (37, 160, 301, 501, 31), "closes_last": (436, 500, 94)}
SILENT, FALLS_SILENT, FALLS_FROM_FRAME = 3, 1, 197
WINDOW = 500
CLOSES = (WINDOW - 1, 2 * WINDOW - 1)           # 0-based frames whose step closes a histogram window
STARTUP = (49, 50, 199, 200)                    # the steps around the two start-up boundaries


def auto_walk(streams, compute_units):
    """The published rule (include/asp_ns.h, AspNsBatch_SetFlowWalk): LONG_WALK steps when the batch has at least one
    workgroup (four streams) per compute unit of the device, SHORT_WALK otherwise; a launch shorter than that is one
    walk."""
    return LONG_WALK if (streams + 3) // 4 >= compute_units else SHORT_WALK


def _walk_position(calls, frame, walk):
    """(index inside its walk, walk length) of 0-based `frame` of the run: a call of n steps goes out as launches of up
    to 64 steps, a launch of m steps as chunks of min(walk, m) steps, the last one shorter."""
    base = 0
    for n in calls:
        if frame < base + n:
            k = frame - base
            j = k % MAX_LAUNCH
            m = min(MAX_LAUNCH, n - (k - j))
            w = min(walk, m)
            p = j % w
            return p, min(w, m - (j - p))
        base += n
    raise AssertionError(frame)


def _where(calls, frame, walk):
    p, n = _walk_position(calls, frame, walk)
    assert n >= 2
    return "first" if p == 0 else "last" if p == n - 1 else "middle"


def test_schedules_put_the_boundaries_first_middle_and_last_in_the_long_walks():
    for calls in SCHEDULES.values():
        assert sum(calls) == 1030
    for walk in NEW_WALKS + (16, 32):   # (the arithmetic holds for every walk a later policy might pick)
        a, b = SCHEDULES["resident"], SCHEDULES["closes_last"]
        assert [_where(a, f, walk) for f in CLOSES] == ["middle", "first"], walk
        assert [_where(b, f, walk) for f in CLOSES] == ["last", "last"], walk
        for f in STARTUP:
            assert _where(a, f, walk) == "middle", (walk, f)
    # the schedule of test_ns_resident_gpu.py has a close on a walk's last step for walks of 2 only
    assert _where(SCHEDULES["resident"], CLOSES[0], 2) == "last"


@pytest.fixture(scope="module")
def ns():
    from audiosignalprocess_amd import ns as mod

    assert mod.device_count() >= 1, "GPU tests need a HIP device"
    return mod


def _rings(calls):
    """One ring of three frames per call (step k of a call reads slot k % 3), different from call to call."""
    out, base = [], 0
    for c, n in enumerate(calls):
        x = ns_frames(S, RING, stream0=40, frame0=7 * c)
        x[:, SILENT] = 0.0
        if base >= FALLS_FROM_FRAME:
            x[:, FALLS_SILENT] = 0.0
        out.append(np.ascontiguousarray(x))
        base += n
    return out


class _Run:
    """One batch driven through `calls` = [(ring frames [ring][streams][160], steps), ...] on the replay entry point;
    `sample`: the streams whose state collect() exports after every call."""

    def __init__(self, ns, streams, calls, sample, flow, walk=0):
        from audiosignalprocess_amd.ns import DeviceBuffer

        self.g = ns.NsBatch(streams, policy=1, kernel=3)
        self.g.set_flow(flow)
        self.g.set_split(1)
        self.g.set_flow_walk(walk)
        self.calls, self.sample = calls, sample
        self.bufs = []
        for x, _ in calls:
            din, dout = DeviceBuffer(x.nbytes), DeviceBuffer(x.nbytes)
            din.upload(x)
            self.bufs.append((din, dout))
        self.out, self.states, self.chunks = [], [], []

    def enqueue(self, c):
        din, dout = self.bufs[c]
        self.g.analyze_process_replay(din.ptr, dout.ptr, self.calls[c][0].shape[0], self.calls[c][1])
        n = C.c_int(-1)
        assert self.g.lib.AspNsBatch_DebugFlowChunks(self.g.h, C.byref(n)) == 0
        self.chunks.append(n.value)

    def collect(self, c):
        self.g.synchronize()
        self.out.append(self.bufs[c][1].download(self.calls[c][0].shape))
        self.states.append([self.g.export_state(int(s)) for s in self.sample])

    def run(self):
        for c in range(len(self.calls)):
            self.enqueue(c)
            self.collect(c)
        return self

    def close(self):
        self.g.close()


def _assert_same(run, ref):
    for c in range(len(ref.calls)):
        assert np.array_equal(run.out[c].view(np.uint32), ref.out[c].view(np.uint32)), c
        for i, s in enumerate(ref.sample):
            assert state_diff(run.states[c][i], ref.states[c][i]) == {}, (c, s)


# ---- 1. the long walk over 1030 frames from Init
@pytest.fixture(scope="module", params=sorted(SCHEDULES))
def long_run(request, ns):
    lens = SCHEDULES[request.param]
    calls = list(zip(_rings(lens), lens))
    ref = _Run(ns, S, calls, range(S), flow=0).run()
    done = 0
    for c, n in enumerate(lens):
        done += n
        assert np.isfinite(ref.out[c]).all()
        assert np.abs(ref.out[c][:, 0]).max() > 0 and not ref.out[c][:, SILENT].any()
        st = ref.states[c][0]
        assert st.blockInd == done - 1                           # (WebRtcNs_Init leaves blockInd at -1)
        assert st.modelUpdatePars[3] == WINDOW - done % WINDOW    # the window arithmetic above is the kernel's
        assert ref.states[c][SILENT].blockInd == -1               # the zero-energy exit of every step
    assert ref.states[-1][FALLS_SILENT].blockInd < done - 1
    yield calls, ref
    ref.close()


@gpu
@pytest.mark.parametrize("walk", NEW_WALKS)
def test_long_walks_equal_plain_launches_over_a_long_run(ns, long_run, walk):
    calls, ref = long_run
    run = _Run(ns, S, calls, range(S), flow=1, walk=walk).run()
    m = calls[-1][1] % MAX_LAUNCH or MAX_LAUNCH
    assert run.chunks[-1] == -(-m // min(walk, m))
    _assert_same(run, ref)
    run.close()


# ---- 2. and 3.: auto on a device-filling, ragged batch
BIG_S, BIG_CALLS, TILE = 4100, (64, 23), 16


@pytest.fixture(scope="module")
def big(ns):
    base = ns_frames(TILE, RING, stream0=40)
    base[:, 3] = 0.0
    x = np.ascontiguousarray(base[:, (np.arange(BIG_S) * 7) % TILE])
    calls = [(x, n) for n in BIG_CALLS]
    rng = np.random.default_rng(20)
    sample = sorted(set(range(8)) | set(range(BIG_S - 8, BIG_S)) | set(rng.choice(np.arange(8, BIG_S - 8), 16, replace=False).tolist()))
    assert len(sample) == 32
    ref = _Run(ns, BIG_S, calls, sample, flow=0).run()
    assert np.isfinite(ref.out[1]).all() and np.abs(ref.out[1]).max() > 0
    assert ref.states[-1][0].blockInd == sum(BIG_CALLS) - 1
    yield calls, sample, ref
    ref.close()


@gpu
def test_auto_on_a_device_filling_ragged_batch(ns, big):
    calls, sample, ref = big
    w = auto_walk(BIG_S, ns.device_compute_units(0))
    run = _Run(ns, BIG_S, calls, sample, flow=1, walk=0).run()
    assert run.chunks == [-(-n // min(w, n)) for n in BIG_CALLS], (run.chunks, w)
    _assert_same(run, ref)
    run.close()


@gpu
def test_two_device_filling_batches_enqueued_together(ns, big):
    """Each call of two batches on auto is enqueued before either batch is synchronised: their long walks share the
    chip, and every chunk's wait stays bounded by the spin limit of handoff.h (a timed-out wait would fail the
    synchronising call)."""
    calls, sample, ref = big
    runs = [_Run(ns, BIG_S, calls, sample, flow=1, walk=0) for _ in range(2)]
    for c in range(len(calls)):
        for r in runs:
            r.enqueue(c)
        for r in runs:
            r.collect(c)
    for r in runs:
        _assert_same(r, ref)
        r.close()
