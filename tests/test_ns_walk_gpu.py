"""The step-walking form of the NS hand-off build (AspNsBatch_SetFlowWalk; ns_kernels1.hip, NsFlowArgs::walk): a
workgroup runs C consecutive frame steps of its four streams in one loop instead of one step.  Whatever C is, the
outputs and the whole state of every stream must equal, bit for bit, what the plain launches (set_flow(0)) of the
same kernel give."""
import numpy as np
import pytest

from audiosignalprocess_amd.synth import ns_frames
from tests.conftest import state_diff

pytestmark = pytest.mark.gpu

WALKS = (1, 2, 3, 7, 64)   # one step per workgroup, lengths that do not divide a launch, the whole launch


@pytest.fixture(scope="module")
def ns():
    from audiosignalprocess_amd import ns as mod

    assert mod.device_count() >= 1, "GPU tests need a HIP device"
    return mod


class _Run:
    """One batch driven through `calls` = [(ring frames [ring][S][160], steps), ...] on the replay entry point
    (step k of a call uses ring slot k % ring); enqueue() is asynchronous, finish() collects each call's ring of
    outputs and keeps the batch for export_state."""

    def __init__(self, ns, S, policy, calls, flow, walk=0):
        from audiosignalprocess_amd.ns import DeviceBuffer

        self.g = ns.NsBatch(S, policy=policy, kernel=3)
        self.g.set_flow(flow)
        self.g.set_split(1)
        self.g.set_flow_walk(walk)
        self.calls = calls
        self.bufs = []
        for x, _ in calls:
            din, dout = DeviceBuffer(x.nbytes), DeviceBuffer(x.nbytes)
            din.upload(x)
            self.bufs.append((din, dout))

    def enqueue(self):
        for (x, steps), (din, dout) in zip(self.calls, self.bufs):
            self.g.analyze_process_replay(din.ptr, dout.ptr, x.shape[0], steps)

    def finish(self):
        self.g.synchronize()
        self.out = [dout.download(x.shape) for (x, _), (_, dout) in zip(self.calls, self.bufs)]
        return self

    def close(self):
        self.g.close()


def _assert_same(run, ref, S):
    for k, (a, b) in enumerate(zip(run.out, ref.out)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    for s_ in range(S):
        assert state_diff(run.g.export_state(s_), ref.g.export_state(s_)) == {}, s_


# ---------------------------------------------------------------------------------------------
# A small ragged batch: S = 5 leaves the second workgroup with one live wave; ring 3; 70 steps = a call of 4 and a
# call of 66 (a launch of 64, crossing blockInd 50, and one of 2); stream 3 is silent throughout (the zero-energy
# exit of every step), stream 1 falls silent from frame 4 (the second call's ring has it zeroed).
def _small_calls():
    S, ring = 5, 3
    x = ns_frames(S, ring, stream0=40)
    x[:, 3] = 0.0
    x2 = x.copy()
    x2[:, 1] = 0.0
    return S, [(np.ascontiguousarray(x), 4), (np.ascontiguousarray(x2), 66)]


@pytest.fixture(scope="module")
def small_ref(ns):
    S, calls = _small_calls()
    ref = _Run(ns, S, 1, calls, flow=0)
    ref.enqueue()
    ref.finish()
    assert np.isfinite(ref.out[1]).all() and np.abs(ref.out[1]).max() > 0
    yield ref
    ref.close()


@pytest.mark.parametrize("walk", WALKS)
def test_walk_small_ragged_batch_equals_plain_launches(ns, small_ref, walk):
    S, calls = _small_calls()
    run = _Run(ns, S, 1, calls, flow=1, walk=walk)
    run.enqueue()
    run.finish()
    _assert_same(run, small_ref, S)
    run.close()


@pytest.mark.parametrize("walk", WALKS)
def test_walk_two_batches_at_once_equal_plain_launches(ns, small_ref, walk):
    """Two walking batches enqueued before either is waited for: their launches share the chip."""
    S, calls = _small_calls()
    runs = [_Run(ns, S, 1, calls, flow=1, walk=walk) for _ in range(2)]
    for r in runs:
        r.enqueue()
    for r in runs:
        r.finish()
    for r in runs:
        _assert_same(r, small_ref, S)
        r.close()


def _chunks(run):
    import ctypes as C

    n = C.c_int(-1)
    assert run.g.lib.AspNsBatch_DebugFlowChunks(run.g.h, C.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("walk,chunks", [(1, 64), (2, 32), (3, 22), (7, 10), (64, 1), (0, 16)])
def test_walk_length_shapes_the_launch(ns, walk, chunks):
    """The setter reaches the launch: 64 steps go out as ceil(64 / C) chunks along grid y (auto, 0: 4 steps each)."""
    S, calls = _small_calls()
    run = _Run(ns, S, 1, [(calls[0][0], 64)], flow=1, walk=walk)
    run.enqueue()
    run.finish()
    assert _chunks(run) == chunks
    run.close()


def test_walk_ragged_last_round_completes_and_matches(ns):
    """S = 4100 is 1032 workgroups along x: on an MI355X (256 CUs x 4 resident workgroups of this kernel) eight more
    than the device holds at once, so with the whole 8-step launch walked by each workgroup (forced) a last, ragged
    round runs after the first one has finished.  (On a device that holds more, the comparison still stands; the
    ragged round is then not exercised.)"""
    S, ring, steps, D = 4100, 3, 8, 16
    base = ns_frames(D, ring, stream0=40)
    base[:, 3] = 0.0
    x = np.ascontiguousarray(base[:, (np.arange(S) * 7) % D])
    ref = _Run(ns, S, 1, [(x, steps)], flow=0)
    run = _Run(ns, S, 1, [(x, steps)], flow=1, walk=8)
    for r in (ref, run):
        r.enqueue()
    for r in (ref, run):
        r.finish()
    assert np.isfinite(ref.out[0]).all() and np.abs(ref.out[0]).max() > 0
    assert _chunks(run) == 1
    _assert_same(run, ref, S)
    run.close()
    ref.close()
