"""The inputs of tests/ns_shortdiv_cases.py on the CPU: each reaches what it names -- densities on both sides of 1 (and 1
itself) in every tracker, bin 128 included, while the trackers step; a prior probability that is clamped to 1, one that
is clamped to 0.01 and others between; synthesis tails that are non-zero for every lane that reads them; a zero-energy
step in the middle of a walk; squared magnitudes under 2^-100 beside ordinary ones -- and at these inputs the oracle IS
the reference: OracleNs(REDUCE_SEQ) against the compiled reference, outputs and every state field bit for bit, at
policies 0..3."""
import numpy as np
import pytest

from tests import ns_scalar_row_cases as rc
from tests import ns_shortdiv_cases as sc
from tests import oracle_lib
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_SEQ, REDUCE_TREE64P, OracleNs
from tests.test_ns_guards_oracle import _squared_magnitudes

needs_ref = pytest.mark.skipif(not oracle_lib.have_ref(), reason="oracle/_ref not built here")


@pytest.fixture(scope="module")
def bases():
    cache = {}

    def get(mode, policy=1):
        if (mode, policy) not in cache:
            cache[(mode, policy)] = rc.base_states(OracleNs, mode, sc.S, policy)
        return cache[(mode, policy)]

    return get


@pytest.fixture(scope="module")
def by_frame(bases):
    """name -> (case, outputs, [states in front of frame 0] + [states behind every frame])"""
    cache = {}

    def get(name):
        if name not in cache:
            case = sc.CASES[name](bases(REDUCE_TREE64P))
            states, ops = case
            single = [("run", op[1][f:f + 1]) for op in ops for f in range(len(op[1]))]
            y, ex = sc.play(rc.OracleEngine(OracleNs, len(states), REDUCE_TREE64P), (states, single))
            cache[name] = (case, y, [states] + ex)
        return cache[name]

    return get


def test_densities_lie_on_both_sides_of_one_in_every_tracker_and_in_bin_128(by_frame):
    rows = sc.density_rows()
    one = np.float32(1)
    for s in range(3):
        assert (rows[s, :128] < one).sum() > 40 and (rows[s, :128] > one).sum() > 40 and (rows[s] == one).any()
        # a lane's two bins (i and i + 32 within a group of 64, ns_kernels1.hip) are not always on the same side
        assert ((rows[s, :32] < one) != (rows[s, 32:64] < one)).any() or ((rows[s, :31] < one) != (rows[s, 1:32] < one)).any()
    assert rows[0, 128] < one < rows[1, 128] and rows[2, 128] == one
    _, y, seq = by_frame("mixed")
    assert np.isfinite(y).all()
    for st in sc.DENSITY_STREAMS:
        assert np.array_equal(np.array(seq[0][st].density[:], np.float32), rows.reshape(-1))
        below = above = 0
        for f in range(sc.FRAMES):   # the densities every step divides by, not only the imported ones
            d = np.array(seq[f][st].density[:], np.float32).reshape(3, sc.BINS)
            assert np.isfinite(d).all() and (d > 0).all()
            below += (d < one).sum(axis=1)
            above += (d > one).sum(axis=1)
            # every bin of every tracker takes a step of FACTOR / max(density, 1) in every frame
            lq0, lq1 = (np.array(seq[g][st].lquantile[:], np.float32) for g in (f, f + 1))
            assert (lq0 != lq1).mean() > 0.9
        assert (below > sc.FRAMES).all() and (above > sc.FRAMES).all(), (st, below, above)
        # most steps of these streams take the steady body (its conjuncts do not read a density), a publish takes the other
        assert rc.steady_steps(seq[0][st], [True] * sc.FRAMES) > sc.FRAMES // 2


def test_prior_probability_is_clamped_at_both_ends_and_moves_between_them(by_frame):
    case, _, seq = by_frame("mixed")
    p = np.array([[states[s].priorSpeechProb for s in range(sc.S)] for states in seq], np.float32)
    assert [case[0][s].priorSpeechProb for s in (1, 2)] == [1.5, -0.5]
    # stream 1: the update from 1.5 stays above 1 and is clamped; stream 2: from -0.5 it stays below 0.01 and is clamped
    assert p[1, 1] == np.float32(1.0) and p[1, 2] == np.float32(0.01)
    assert p[0, 4] == np.float32(0.01)
    inside = (p[1:] > np.float32(0.01)) & (p[1:] < np.float32(1.0))
    assert inside.any(axis=0).all() and inside.sum() > sc.FRAMES
    assert (p[1:] >= np.float32(0.01)).all() and (p[1:] <= np.float32(1.0)).all()


def test_synthesis_tails_are_non_zero_for_owners_and_the_lanes_that_drop_them(by_frame):
    _, _, seq = by_frame("mixed")
    for f in (0, 1, 3, 10, 23):   # in front of every call
        for s in range(sc.S):
            if s == sc.ZERO_STREAM and f > sc.ZERO_FRAMES[0]:
                continue
            assert (np.array(seq[f][s].syntBuf[:96], np.float32) != 0).all(), (f, s)


def test_zero_energy_step_sits_in_the_middle_of_a_walk(by_frame):
    _, y, seq = by_frame("mixed")
    s = sc.ZERO_STREAM
    energies = [_squared_magnitudes(seq[f + 1][s])[1] for f in range(sc.FRAMES)]
    assert [f for f, e in enumerate(energies) if e == 0] == [sc.ZERO_STEP]
    start = sum(sc.CALLS[:3])   # the fourth call, 13 frames: walks of 8 and of 3 both start at its first frame
    assert start < sc.ZERO_STEP < start + sc.CALLS[3]
    assert (sc.ZERO_STEP - start) % 8 not in (0, 7) and (sc.ZERO_STEP - start) % 3 == 1
    assert np.isfinite(y).all()


def test_tiny_puts_squared_magnitudes_under_two_to_the_minus_100(by_frame):
    case, y, seq = by_frame("tiny")
    x = np.concatenate([op[1] for op in case[1]])
    s = sc.TINY_STREAM
    assert 0 < np.abs(x[sc.TINY_FRAMES[0], s]).max() <= sc.TINY_AMPLITUDE
    assert np.isfinite(y).all()
    under = np.float32(2.0 ** -100)
    hits = 0
    for f in sc.TINY_FRAMES[1:]:   # the window holds nothing but the small frames from the second of them on
        m2, energy = _squared_magnitudes(seq[f + 1][s])
        assert energy > 0
        hits += int(((m2 > 0) & (m2 < under)).sum())
    assert hits > 100
    # its neighbours in the workgroup analyse ordinary frames in the same steps: the wave-level test is per wave
    m2, _ = _squared_magnitudes(seq[sc.TINY_FRAMES[1] + 1][0])
    assert (m2 >= under).all()
    # and the first small frame still shares its window with ordinary samples
    m2, _ = _squared_magnitudes(seq[sc.TINY_FRAMES[0] + 1][s])
    assert (m2 >= under).all()


def _assert_bitwise(got, want, what):
    (ya, ea), (yb, eb) = got, want
    bad = np.nonzero((ya.view(np.uint32) != yb.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, "first differing frame / stream", bad[0][:3], bad[1][:3])
    for k, (a, b) in enumerate(zip(ea, eb)):
        for s in range(len(a)):
            assert state_diff(a[s], b[s], skip=set()) == {}, (what, "export", k, "stream", s)


@needs_ref
@pytest.mark.parametrize("policy", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_oracle_equals_reference(bases, name, policy):
    case = sc.CASES[name](bases(REDUCE_SEQ, policy))
    want = sc.play(rc.RefEngine(oracle_lib.RefNs, sc.S, policy), case)
    assert np.isfinite(want[0]).all()
    got = sc.play(rc.OracleEngine(OracleNs, sc.S, REDUCE_SEQ, policy), case)
    _assert_bitwise(got, want, (name, policy))
