"""The two bodies of the pair-layout NS frame step (ns_kernels1.hip): from the point where a step has read its
wave-uniform scalars, the rest of the step exists as a generic body and as a steady body compiled under
ns_assume_steady(); ns_step_is_steady() chooses per step.  Both must give the same bits: steady on against steady off
(set_steady), and both against the oracle in the kernel's association, so that a predicate that is wrong the same way
in both settings cannot hide.

The long run: 6 streams (two workgroups, the second with two live waves and two clamped ones), 1030 frames from Init in
short uneven calls, so that steady and generic steps mix inside walks and across launches.  It crosses the end of both
start-up windows (frames 50 and 200), every tracker's publish (the counters start at 66 / 133 / 200 and publish every
200 frames, staggered) and the histogram-window close at frames 500 and 1000.

Which body a step takes follows from the frame index alone while every frame has energy (0-based frame f of a stream
run from Init; blockInd of the step is f, `updates` is min(f, 200), tracker s enters the step with its counter at 200
when f % 200 == (0, 134, 67)[s] and at 199 one frame earlier, and the histogram window has 500 - f % 500 frames left).
The conjuncts of NS_STEADY_CONJUNCTS then say: a step is GENERIC iff

    f <= 201                                      (blockInd > NS_END_STARTUP_LONG + 1 fails; covers updates < 200)
    or f % 200 in {199, 0, 133, 134, 66, 67}      (a counter at 199 or 200: not < NS_END_STARTUP_LONG - 1)
    or f % 500 in {498, 499}                      (mup3 <= 2: the window closes in this step or the next)

(updateParsFlag stays 2 and gainmap is 1 under policy 1).  The diagnostic kernels count the steps per body and stream;
the counts must equal this formula exactly."""
import numpy as np
import pytest

from audiosignalprocess_amd.synth import ns_frames
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_TREE64P, OracleNs

pytestmark = pytest.mark.gpu

S, F = 6, 1030
CYCLE = (7, 64, 1, 33, 2, 65, 16, 9, 100, 3)    # frames per call, repeated until F frames are done
VARIANTS = [(1, 1), (1, 3), (1, 8), (0, 0)]     # (set_flow, set_flow_walk): hand-off walks of 1, 3, 8; the plain build


def _calls(total):
    out, k = [], 0
    while total:
        n = min(CYCLE[k % len(CYCLE)], total)
        out.append(n)
        total -= n
        k += 1
    return out


def _generic(f):
    return f <= 201 or f % 200 in (199, 0, 133, 134, 66, 67) or f % 500 in (498, 499)


@pytest.fixture(scope="module")
def ns():
    from audiosignalprocess_amd import ns as mod

    assert mod.device_count() >= 1, "GPU tests need a HIP device"
    return mod


def _run(ns, x, flow, walk, steady, counts=False, reinit=None):
    """-> (outputs [F][S][160], [state of every stream], step counts or None); the frames go in as uneven short calls"""
    n_streams = x.shape[1]
    g = ns.NsBatch(n_streams, policy=1, kernel=3)
    g.set_flow(flow)
    g.set_split(1)
    g.set_flow_walk(walk)
    g.set_steady(steady)
    if counts:
        g.debug_step_counts(True)
    y, f0 = np.empty_like(x), 0
    for n in _calls(x.shape[0]):
        y[f0:f0 + n] = g.analyze_process(x[f0:f0 + n])
        f0 += n
    cnt = g.debug_step_counts(False) if counts else None
    st = [g.export_state(s) for s in range(n_streams)]
    g.close()
    return y, st, cnt


def _assert_same(a, b):
    ya, sa = a[0], a[1]
    yb, sb = b[0], b[1]
    bad = np.nonzero((ya.view(np.uint32) != yb.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (bad[0][:5], bad[1][:5])
    for s in range(len(sa)):
        assert state_diff(sa[s], sb[s]) == {}, s


@pytest.fixture(scope="module")
def frames():
    x = np.ascontiguousarray(ns_frames(S, F, stream0=40))
    assert (np.abs(x).max(axis=2) > 0).all()   # every frame has energy: the formula above counts every step
    x.setflags(write=False)
    return x


def _oracle(x):
    o = OracleNs(x.shape[1], policy=1, reduce_mode=REDUCE_TREE64P)
    y = o.run(x, threads=x.shape[1])
    return y, [o.export_state(s) for s in range(x.shape[1])]


@pytest.fixture(scope="module")
def oracle_long(frames):
    y, st = _oracle(frames)
    assert all(s.blockInd == F - 1 for s in st)
    return y, st


@pytest.fixture(scope="module")
def steady_runs(ns, frames):
    cache = {}

    def get(flow, walk):
        if (flow, walk) not in cache:
            cache[(flow, walk)] = _run(ns, frames, flow, walk, steady=1)
        return cache[(flow, walk)]

    return get


def test_the_schedule_mixes_bodies_inside_walks_and_launches():
    calls = _calls(F)
    assert sum(calls) == F and 1 in calls and max(calls) > 64
    gen = sum(_generic(f) for f in range(F))
    assert 202 < gen < F // 2   # start-up, then a few steps in 200


@pytest.mark.parametrize("flow,walk", VARIANTS)
def test_steady_on_equals_steady_off_bit_for_bit(ns, frames, steady_runs, flow, walk):
    _assert_same(steady_runs(flow, walk), _run(ns, frames, flow, walk, steady=0))


@pytest.mark.parametrize("flow,walk", VARIANTS)
def test_steady_on_equals_the_oracle_bit_for_bit(frames, steady_runs, oracle_long, flow, walk):
    _assert_same(steady_runs(flow, walk), oracle_long)


def test_both_bodies_ran_and_the_generic_count_is_what_the_scalars_dictate(ns, frames, oracle_long):
    run = _run(ns, frames, 1, 3, steady=1, counts=True)
    _assert_same(run, oracle_long)   # the diagnostic kernels compute the same
    cnt = run[2]
    gen = sum(_generic(f) for f in range(F))
    print("steady / generic steps per stream:", cnt.tolist(), "expected generic:", gen)
    assert (cnt > 0).all()
    assert (cnt.sum(axis=1) == F).all()
    assert (cnt[:, 1] == gen).all() and (cnt[:, 0] == F - gen).all()
    off = _run(ns, frames[:300], 1, 3, steady=0, counts=True)[2]
    assert (off[:, 0] == 0).all() and (off[:, 1] == 300).all()


def test_zero_energy_frames_in_steady_state(ns):
    x = np.ascontiguousarray(ns_frames(2, 300, stream0=40))
    quiet = x.copy()
    quiet[250:260, 0] = 0.0
    want = _oracle(quiet)
    # (the first silent frame still has the 96 carried samples in its analysis window: 9 zero-energy steps)
    assert want[1][0].blockInd == 300 - 9 - 1 and want[1][1].blockInd == 299
    for flow, walk in ((1, 3), (0, 0)):
        got = _run(ns, quiet, flow, walk, steady=1)
        _assert_same(got, want)
        # stream 1 is unaffected: its run without the silence
        base = _run(ns, x, flow, walk, steady=1)
        assert np.array_equal(got[0][:, 1].view(np.uint32), base[0][:, 1].view(np.uint32))
        assert state_diff(got[1][1], base[1][1]) == {}


def test_streams_in_different_states_in_one_workgroup(ns):
    """Streams 1 and 3 are silent for their first 150 frames: the zero-energy path leaves blockInd behind (asserted), so
    they run their start-up while streams 0 and 2 of the same workgroup are in steady state."""
    x = np.ascontiguousarray(ns_frames(4, 450, stream0=40))
    x[:150, 1] = 0.0
    x[:150, 3] = 0.0
    want = _oracle(x)
    assert [s.blockInd for s in want[1]] == [449, 299, 449, 299]
    for flow, walk in ((1, 8), (1, 3), (0, 0)):
        _assert_same(_run(ns, x, flow, walk, steady=1), want)


def test_int16_frames_are_refused_while_step_counts_are_on(ns):
    """The diagnostic kernels take float frames: an int16 call is refused by the API with a reason, and works again
    once the counts are switched off."""
    pcm = np.clip(np.rint(ns_frames(4, 3, stream0=40)), -32768, 32767).astype(np.int16)
    g = ns.NsBatch(4, policy=1, kernel=3)
    g.debug_step_counts(True)
    with pytest.raises(ns.AspError, match="float frames"):
        g.analyze_process_s16(pcm)
    g.debug_step_counts(False)
    assert g.analyze_process_s16(pcm).shape == pcm.shape
    g.close()
