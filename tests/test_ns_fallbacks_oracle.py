"""The inputs of tests/ns_fallbacks_cases.py on the CPU: each new case reaches what it names -- a window really closes
in the steps the case lists, the recorded features fall both inside and outside their histograms' ranges and the
histograms count exactly the ones inside, a stream with modelUpdatePars[0] = 0 never adds -- and at these inputs the
oracle IS the reference: OracleNs(REDUCE_SEQ) against the compiled reference, outputs and every state field bit for
bit, at policies 0..3.  (The cases shared with the earlier modules are asserted in those modules' own oracle tests.)"""
import numpy as np
import pytest

from tests import ns_cases
from tests import ns_fallbacks_cases as fc
from tests import ns_scalar_row_cases as rc
from tests import oracle_lib
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_SEQ, REDUCE_TREE64P, OracleNs

needs_ref = pytest.mark.skipif(not oracle_lib.have_ref(), reason="oracle/_ref not built here")


@pytest.fixture(scope="module")
def bases():
    cache = {}

    def get(mode, policy=1):
        if (mode, policy) not in cache:
            cache[(mode, policy)] = rc.base_states(OracleNs, mode, fc.S, policy)
        return cache[(mode, policy)]

    return get


def _frame_by_frame(case, mode=REDUCE_TREE64P):
    """the frames of a case's "run" operations one at a time: -> [(states in front of frame f, states behind it)]; an
    imported state is what its stream has in front of the next frame"""
    states, ops = case
    eng = rc.OracleEngine(OracleNs, len(states), mode)
    for s, st in enumerate(states):
        eng.import_state(s, st)
    cur, pairs = list(states), []
    for op in ops:
        if op[0] == "import":
            eng.import_state(op[1], op[2])
            cur[op[1]] = op[2]
            continue
        assert op[0] == "run"
        for f in range(len(op[1])):
            eng.run(op[1][f:f + 1])
            nxt = [eng.export_state(s) for s in range(len(states))]
            pairs.append((cur, nxt))
            cur = list(nxt)
    return pairs


def test_closes_close_where_the_case_says_with_steady_steps_between(bases):
    case = fc.closes(bases(REDUCE_TREE64P))
    pairs = _frame_by_frame(case)
    n = sum(fc.CLOSE_CALLS)
    assert len(pairs) == n
    for s in range(fc.S):
        # a close re-opens the window: the frames left go back to the window's length and the histograms are cleared
        closed = [f for f in range(n) if pairs[f][1][s].modelUpdatePars[3] == 500]
        assert closed == fc.CLOSE_STEPS[s], (s, closed)
        steady = [rc.steady_steps(pairs[f][0][s], [True]) == 1 for f in range(n)]
        for f in range(n):
            before, after = fc.hist_sums(pairs[f][0][s]), fc.hist_sums(pairs[f][1][s])
            if f in closed:
                assert after == [0, 0, 0] and sum(before) > 0, (s, f)
                # it rewrites the prior model; it and the two steps in front of it are generic, the one behind it steady
                assert list(pairs[f][0][s].priorModelPars[:]) != list(pairs[f][1][s].priorModelPars[:]), (s, f)
                assert not steady[f] and (f + 1 >= n or steady[f + 1])
            else:
                assert all(0 <= a - b <= 1 for a, b in zip(after, before)) and sum(after) > sum(before), (s, f)
        assert 0 < sum(steady) < n
    flat = sorted(set(sum(fc.CLOSE_STEPS.values(), [])))
    # a walk's first, a middle and its last step for walks of 8 and of 3 (calls of 8: a walk starts with every call)
    assert {f % 8 for f in flat} >= {0, 4, 7} and {(f % 8) % 3 for f in flat} >= {0, 1, 2}
    # one stream closes in two consecutive calls
    assert any(b // 8 == a // 8 + 1 for st in fc.CLOSE_STEPS.values() for a, b in zip(st, st[1:]))


def _in_range(v, bw):
    return np.float32(0) <= np.float32(v) < np.float32(ns_cases.HIST) * np.float32(bw)


def test_out_of_range_records_features_inside_and_outside_the_histograms(bases):
    case = fc.out_of_range(bases(REDUCE_TREE64P))
    pairs = _frame_by_frame(case)
    inside, outside = [0, 0, 0], [0, 0, 0]
    for s in range(fc.S):
        assert rc.steady_steps(pairs[0][0][s], [True] * fc.OUT_FRAMES) == fc.OUT_FRAMES   # every step records
        for f in range(fc.OUT_FRAMES):
            before, after = pairs[f][0][s], pairs[f][1][s]
            # what the step counts: the previous frame's average LRT, the new flatness and difference features
            feats = (before.featureData[3], after.featureData[0], after.featureData[4])
            for k, (field, (_, bw)) in enumerate(zip(fc.HIST_FIELDS, fc.HIST_FEATURES)):
                hb, ha = np.array(getattr(before, field)[:]), np.array(getattr(after, field)[:])
                ok = bool(_in_range(feats[k], bw))
                assert int((ha - hb).sum()) == int(ok) and (ha >= hb).all(), (s, f, field)
                inside[k] += ok
                outside[k] += not ok
                if s in fc.OUT_STREAMS and k == 2:
                    assert not ok, (s, f, feats[k])
    assert all(v > 0 for v in inside) and outside[2] >= len(fc.OUT_STREAMS) * fc.OUT_FRAMES, (inside, outside)


def test_no_update_stream_never_adds_and_its_neighbours_do(bases):
    case = fc.no_update(bases(REDUCE_TREE64P))
    pairs = _frame_by_frame(case)
    seq = [pairs[0][0]] + [p[1] for p in pairs]
    s = fc.NO_UPDATE_STREAM
    assert rc.steady_steps(seq[0][s], [True] * 24) == 0
    for f in range(24):
        assert fc.hist_sums(seq[f + 1][s]) == fc.hist_sums(seq[0][s])
        assert seq[f + 1][s].modelUpdatePars[3] == seq[0][s].modelUpdatePars[3]
    for t in range(fc.S):
        if t != s:
            assert sum(fc.hist_sums(seq[24][t])) > sum(fc.hist_sums(seq[0][t])) + 24
            assert rc.steady_steps(seq[0][t], [True] * 24) == 24


def _assert_bitwise(got, want, what):
    (ya, ea), (yb, eb) = got, want
    bad = np.nonzero((ya.view(np.uint32) != yb.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, "first differing frame / stream", bad[0][:3], bad[1][:3])
    for k, (a, b) in enumerate(zip(ea, eb)):
        for s in range(len(a)):
            assert state_diff(a[s], b[s], skip=set()) == {}, (what, "export", k, "stream", s)


@needs_ref
@pytest.mark.parametrize("policy", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(fc.NEW_CASES))
def test_oracle_equals_reference(bases, name, policy):
    case = fc.NEW_CASES[name](bases(REDUCE_SEQ, policy))
    want = fc.play(rc.RefEngine(oracle_lib.RefNs, fc.S, policy), case)
    assert np.isfinite(want[0]).all()
    got = fc.play(rc.OracleEngine(OracleNs, fc.S, REDUCE_SEQ, policy), case)
    _assert_bitwise(got, want, (name, policy))
