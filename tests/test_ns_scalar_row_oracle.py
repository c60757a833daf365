"""The inputs of tests/ns_scalar_row_cases.py on the CPU: each case reaches the branch it names (asserted from the
oracle's exported states), and at these inputs the oracle IS the reference -- OracleNs(REDUCE_SEQ) against the compiled
reference, outputs and every state field bit for bit, at policies 0..3."""
import numpy as np
import pytest

from tests import ns_scalar_row_cases as rc
from tests import oracle_lib
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_SEQ, REDUCE_TREE64P, OracleNs

needs_ref = pytest.mark.skipif(not oracle_lib.have_ref(), reason="oracle/_ref not built here")
CASES = {"uneven": rc.uneven_calls, "zero": rc.zero_energy, "generic": rc.generic_inside_walk,
         "between": rc.scalars_between_launches, "full": rc.full_workgroups}


@pytest.fixture(scope="module")
def bases():
    cache = {}

    def get(mode, n_streams=rc.S, policy=1):
        key = (mode, n_streams, policy)
        if key not in cache:
            cache[key] = rc.base_states(OracleNs, mode, n_streams, policy)
        return cache[key]

    return get


def _oracle(case, mode, policy=1):
    return rc.play(rc.OracleEngine(OracleNs, len(case[0]), mode, policy), case)


def test_the_base_state_is_steady(bases):
    for st in bases(REDUCE_TREE64P):
        assert st.blockInd == rc.BASE_FRAMES - 1 and st.updates == 200 and st.gainmap == 1
        assert st.modelUpdatePars[0] == 2 and st.modelUpdatePars[3] == 500 - rc.BASE_FRAMES
        assert all(0 <= c < 170 for c in st.counter)
        assert rc.steady_steps(st, [True] * 24) == 24
        # (tracker 2 reaches its publish 37 frames on: the 40-frame case has two generic steps of its own)
        assert rc.steady_steps(st, [True] * 40) == 38


def test_uneven_calls_export_behind_every_call(bases):
    case = rc.uneven_calls(bases(REDUCE_TREE64P))
    y, ex = _oracle(case, REDUCE_TREE64P)
    assert y.shape == (40, rc.S, 160) and len(ex) == 5
    assert [e[0].blockInd - (rc.BASE_FRAMES - 1) for e in ex] == [1, 3, 10, 23, 40]
    # every float scalar the step commits moves from call to call
    for a, b in zip(ex, ex[1:]):
        assert any(a[s].priorSpeechProb != b[s].priorSpeechProb for s in range(rc.S))
        for s in range(rc.S):
            assert a[s].featureData[0] != b[s].featureData[0] and a[s].featureData[3] != b[s].featureData[3]
            assert a[s].featureData[4] != b[s].featureData[4] and a[s].signalEnergy != b[s].signalEnergy


def test_zero_energy_steps_fall_where_the_case_says(bases):
    states, ops = rc.zero_energy(bases(REDUCE_TREE64P))
    x = ops[0][1]
    o = rc.OracleEngine(OracleNs, rc.S, REDUCE_TREE64P)
    for s, st in enumerate(states):
        o.import_state(s, st)
    before = rc.BASE_FRAMES - 1
    for f in range(x.shape[0]):
        o.run(x[f:f + 1])
        st = o.export_state(1)
        assert (st.blockInd == before) == (f in rc.ZERO_STEPS), f   # a zero-energy step leaves blockInd behind
        before = st.blockInd
        assert o.export_state(0).blockInd == rc.BASE_FRAMES + f    # the neighbours carry signal
    assert {f % 8 for f in rc.ZERO_STEPS} >= {0, 4, 7} and {f % 3 for f in rc.ZERO_STEPS} == {0, 1, 2}


def test_generic_steps_fall_inside_a_walk_with_steady_ones_behind_them(bases):
    states, ops = rc.generic_inside_walk(bases(REDUCE_TREE64P))
    x = ops[0][1]
    o = rc.OracleEngine(OracleNs, rc.S, REDUCE_TREE64P)
    for s, st in enumerate(states):
        o.import_state(s, st)
    steady = {s: [] for s in range(rc.S)}
    quant0 = np.array(states[0].quantile[:])
    pars2 = list(states[2].priorModelPars)
    for f in range(x.shape[0]):
        before = [o.export_state(s) for s in range(rc.S)]
        o.run(x[f:f + 1])
        for s in range(rc.S):
            steady[s].append(rc.steady_steps(before[s], [True]) == 1)
        if f == 3:   # the tracker published: the quantile row changed in this step and in no earlier one
            assert not np.array_equal(np.array(o.export_state(0).quantile[:]), quant0)
        if f == 2:
            assert np.array_equal(np.array(o.export_state(0).quantile[:]), quant0)
        if f == 3:
            assert list(o.export_state(2).priorModelPars) == pars2 and o.export_state(2).modelUpdatePars[3] == 1
        if f == 4:   # the window closed: new prior model, the window reopened
            assert list(o.export_state(2).priorModelPars) != pars2 and o.export_state(2).modelUpdatePars[3] == 500
    assert steady[0][:6] == [True, True, False, False, True, True] and all(steady[0][4:8])
    assert steady[2][:8] == [True, True, True, False, False, True, True, True]
    assert steady[4][:8] == [True, True, False, False, False, True, True, True]
    assert all(steady[1]) and all(steady[3])


def test_the_scalars_change_between_the_two_calls(bases):
    case = rc.scalars_between_launches(bases(REDUCE_TREE64P))
    _, ex = _oracle(case, REDUCE_TREE64P)
    first, last = ex
    assert first[2].overdrive == 1.0 and last[2].overdrive == np.float32(1.25)
    assert first[2].denoiseBound == 0.25 and last[2].denoiseBound == np.float32(0.09)
    assert last[2].blockInd == rc.BASE_FRAMES + 17
    assert last[3].blockInd == 8 and last[3].gainmap == 0 and last[3].denoiseBound == 0.5   # a fresh stream, 9 frames old
    assert last[1].overdrive == 1.0 and last[1].blockInd == rc.BASE_FRAMES + 17


def test_full_workgroups_mix_bodies(bases):
    states, _ = rc.full_workgroups(bases(REDUCE_TREE64P, 8))
    counts = [rc.steady_steps(st, [True] * 16) for st in states]
    assert counts[0] == 16 and counts[2] == 16 and all(0 < counts[s] < 16 for s in (1, 3, 5, 6))


def _assert_bitwise(got, want, what):
    (ya, ea), (yb, eb) = got, want
    bad = np.nonzero((ya.view(np.uint32) != yb.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, "first differing frame / stream", bad[0][:3], bad[1][:3])
    for k, (a, b) in enumerate(zip(ea, eb)):
        for s in range(len(a)):
            assert state_diff(a[s], b[s], skip=set()) == {}, (what, "export", k, "stream", s)


@needs_ref
@pytest.mark.parametrize("policy", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_reference(bases, name, policy):
    n = 8 if name == "full" else rc.S
    case = CASES[name](bases(REDUCE_SEQ, n, policy))
    want = rc.play(rc.RefEngine(oracle_lib.RefNs, n, policy), case)
    _assert_bitwise(_oracle(case, REDUCE_SEQ, policy), want, (name, policy))
