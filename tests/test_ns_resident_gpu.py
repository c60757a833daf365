"""The resident state block of the NS hand-off build (ns_kernels1.hip): a wave keeps its stream's hot state in LDS for
the length of its walk, copies it in once and writes it back once, and seq[stream] advances once per walk.  A long run
from Init -- 1030 frames in five calls of different lengths -- must equal, bit for bit, what the plain launches
(set_flow(0)) of the same kernel give: the outputs of every call and export_state of every stream after every call,
for walks of 1, 2, 3, 4, 7 and 64 steps and the automatic length.

What the run crosses inside walks: frame 50 (the start-up rows V_INITMAGN / V_PARAMNOISE stay in memory and are written
and read back within a walk), frame 200 (the trackers publish, V_QUANT is written), and the histogram window closes
on frames 500 and 1000 (counting from 1).  The call lengths put the second close on the first step of a walk and the
first close on a middle or the last step, depending on the walk; the test derives that from the step arithmetic."""
import ctypes as C

import numpy as np
import pytest

from audiosignalprocess_amd.synth import ns_frames
from tests.conftest import state_diff

gpu = pytest.mark.gpu

S, RING = 5, 3                      # the second workgroup has one live wave
CALLS = (37, 160, 301, 501, 31)     # frames per call: 1030 in all
SILENT, FALLS_SILENT, FALLS_FROM_CALL = 3, 1, 2
WALKS = (1, 2, 3, 4, 7, 64, 0)      # 0: auto
AUTO_WALK, MAX_LAUNCH = 4, 64       # ns_api.hip: kFlowWalkAuto; handoff_host.h: kHandoffMaxSteps
WINDOW = 500                        # modelUpdatePars[1]: frames per histogram window
CLOSES = (WINDOW - 1, 2 * WINDOW - 1)   # 0-based frames whose step closes a window


def _walk_position(frame, walk):
    """(index inside its walk, walk length) of 0-based `frame` of the run: a call of n steps goes out as launches of up
    to 64 steps, a launch of m steps as chunks of min(walk, m) steps, the last one shorter."""
    base = 0
    for n in CALLS:
        if frame < base + n:
            k = frame - base
            j = k % MAX_LAUNCH
            m = min(MAX_LAUNCH, n - (k - j))
            w = min(walk if walk else AUTO_WALK, m)
            p = j % w
            return p, min(w, m - (j - p))
        base += n
    raise AssertionError(frame)


def _last_launch_chunks(n, walk):
    m = n % MAX_LAUNCH or MAX_LAUNCH
    w = min(walk if walk else AUTO_WALK, m)
    return -(-m // w)


def test_call_lengths_put_the_window_closes_first_middle_and_last_in_a_walk():
    assert sum(CALLS) == 1030 and len(set(CALLS)) == len(CALLS) >= 4
    where = set()
    for walk in WALKS:
        for f in CLOSES:
            p, n = _walk_position(f, walk)
            if n >= 2:
                where.add("first" if p == 0 else "last" if p == n - 1 else "middle")
    assert where == {"first", "middle", "last"}, where
    # frames 50 and 200 sit inside a walk (neither its first nor its only step) for some walk as well
    for f in (49, 50, 199, 200):
        assert any(_walk_position(f, w)[0] > 0 for w in WALKS), f


@pytest.fixture(scope="module")
def ns():
    from audiosignalprocess_amd import ns as mod

    assert mod.device_count() >= 1, "GPU tests need a HIP device"
    return mod


@pytest.fixture(scope="module")
def rings():
    """One ring of three frames per call (step k of a call reads slot k % 3), different from call to call."""
    out = []
    for c, _ in enumerate(CALLS):
        x = ns_frames(S, RING, stream0=40, frame0=7 * c)
        x[:, SILENT] = 0.0
        if c >= FALLS_FROM_CALL:
            x[:, FALLS_SILENT] = 0.0
        out.append(np.ascontiguousarray(x))
    return out


class _Run:
    def __init__(self, ns, rings, flow, walk=0, reinit=None):
        from audiosignalprocess_amd.ns import DeviceBuffer

        self.g = ns.NsBatch(S, policy=1, kernel=3)
        self.g.set_flow(flow)
        self.g.set_split(1)
        self.g.set_flow_walk(walk)
        self.reinit = reinit  # (call index, stream): WebRtcNs_Init + another policy for that stream before that call
        self.bufs = []
        for x in rings:
            din, dout = DeviceBuffer(x.nbytes), DeviceBuffer(x.nbytes)
            din.upload(x)
            self.bufs.append((din, dout))
        self.out, self.states = [], []

    def enqueue(self, c):
        if self.reinit is not None and self.reinit[0] == c:
            self.g.init_stream(self.reinit[1])
            self.g.set_policy_stream(self.reinit[1], 2)
        din, dout = self.bufs[c]
        self.g.analyze_process_replay(din.ptr, dout.ptr, RING, CALLS[c])

    def collect(self, c):
        self.g.synchronize()
        self.out.append(self.bufs[c][1].download((RING, S, 160)))
        self.states.append([self.g.export_state(s) for s in range(S)])

    def chunks(self):
        n = C.c_int(-1)
        assert self.g.lib.AspNsBatch_DebugFlowChunks(self.g.h, C.byref(n)) == 0
        return n.value

    def run(self):
        for c in range(len(CALLS)):
            self.enqueue(c)
            self.collect(c)
        return self

    def close(self):
        self.g.close()


def _assert_same(run, ref):
    for c in range(len(CALLS)):
        assert np.array_equal(run.out[c].view(np.uint32), ref.out[c].view(np.uint32)), c
        for s in range(S):
            assert state_diff(run.states[c][s], ref.states[c][s]) == {}, (c, s)


@pytest.fixture(scope="module")
def plain(ns, rings):
    ref = _Run(ns, rings, flow=0).run()
    done = 0
    for c, n in enumerate(CALLS):
        done += n
        assert np.isfinite(ref.out[c]).all()
        assert np.abs(ref.out[c][:, 0]).max() > 0 and not ref.out[c][:, SILENT].any()
        st = ref.states[c][0]
        assert st.blockInd == done - 1                          # (WebRtcNs_Init leaves blockInd at -1)
        assert st.modelUpdatePars[3] == WINDOW - done % WINDOW   # the window arithmetic above is the kernel's
        assert ref.states[c][SILENT].blockInd == -1              # the zero-energy exit of every step
    assert ref.states[-1][FALLS_SILENT].blockInd < done - 1
    yield ref
    ref.close()


@gpu
@pytest.mark.parametrize("walk", WALKS)
def test_resident_walks_equal_plain_launches_over_a_long_run(ns, rings, plain, walk):
    run = _Run(ns, rings, flow=1, walk=walk).run()
    assert run.chunks() == _last_launch_chunks(CALLS[-1], walk)
    _assert_same(run, plain)
    run.close()


@pytest.fixture(scope="module")
def plain_reinit(ns, rings):
    ref = _Run(ns, rings, flow=0, reinit=(3, 2)).run()
    assert ref.states[3][2].blockInd == CALLS[3] - 1 and ref.states[3][0].blockInd == sum(CALLS[:4]) - 1
    yield ref
    ref.close()


@gpu
@pytest.mark.parametrize("walk", (0, 7))
def test_resident_walks_with_a_stream_reinitialised_between_calls(ns, rings, plain_reinit, walk):
    """Stream 2 gets WebRtcNs_Init and policy 2 in front of the fourth call: it runs its start-up (cold rows) while
    its neighbours' walks cross the first window close."""
    run = _Run(ns, rings, flow=1, walk=walk, reinit=(3, 2)).run()
    _assert_same(run, plain_reinit)
    run.close()


@gpu
def test_two_resident_batches_enqueued_together(ns, rings, plain):
    """Each call of two batches is enqueued before either batch is synchronised: their walks share the chip."""
    runs = [_Run(ns, rings, flow=1, walk=w) for w in (0, 3)]
    for c in range(len(CALLS)):
        for r in runs:
            r.enqueue(c)
        for r in runs:
            r.collect(c)
    for r in runs:
        _assert_same(r, plain)
        r.close()
