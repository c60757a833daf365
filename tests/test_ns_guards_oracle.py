"""The inputs of tests/ns_guards_cases.py on the CPU: each new case reaches what it names (asserted from the oracle's
outputs and exported states), the reference stays finite wherever its input is, and at these inputs the oracle IS the
reference -- OracleNs(REDUCE_SEQ) against the compiled reference, outputs and every state field bit for bit, at policies
0..3.  (The three cases shared with tests/ns_scalar_row_cases.py and tests/ns_carry_cases.py are asserted in those
modules' own oracle tests.)"""
import numpy as np
import pytest

from tests import ns_guards_cases as gc
from tests import ns_scalar_row_cases as rc
from tests import oracle_lib
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_SEQ, REDUCE_TREE64P, OracleNs

needs_ref = pytest.mark.skipif(not oracle_lib.have_ref(), reason="oracle/_ref not built here")
FLOAT_ROWS = ("density", "lquantile", "quantile", "smooth", "noisePrev", "magnPrevAnalyze", "logLrtTimeAvg",
              "magnAvgPause", "featureData", "priorModelPars", "syntBuf", "analyzeBuf")


@pytest.fixture(scope="module")
def bases():
    cache = {}

    def get(mode, policy=1):
        if (mode, policy) not in cache:
            cache[(mode, policy)] = rc.base_states(OracleNs, mode, gc.S, policy)
        return cache[(mode, policy)]

    return get


def _frame_by_frame(case, mode=REDUCE_TREE64P):
    """the frames of a case's "run" operations one at a time: -> (outputs [F][S][160], [[state of every stream]
    behind every frame]); the other operations are played where they stand"""
    states, ops = case
    single = []
    for op in ops:
        single += [("run", op[1][f:f + 1]) for f in range(len(op[1]))] if op[0] == "run" else [op]
    return gc.play(rc.OracleEngine(OracleNs, len(states), mode), (states, single))


def test_saturate_leaves_the_int16_range_on_every_sample_on_one_lane_and_downwards_only(bases):
    y, _ = gc.play(rc.OracleEngine(OracleNs, gc.S, REDUCE_TREE64P), gc.saturate(bases(REDUCE_TREE64P)))
    assert y.shape[0] == gc.SAT_FRAMES
    # (a sample that left the range is seen as the bound it was set to: 32767 or -32768, ns_core.c:1352-1356)
    assert (y[gc.SAT_FROM:, 0] == 32767).all()
    f, n = np.nonzero(np.abs(y[:, 1]) >= 32767)
    assert len(f) >= 1 and len(set(f)) == 1 and len(set(n // 2)) == 1, (f, n)  # one lane's pair of one store block
    assert f[0] == gc.SPIKE_AT[0]
    assert (y[:, 2] == -32768).any() and y[:, 2].max() < 32767
    assert np.abs(y[:, 3:]).max() < 32767


def test_clip16_overshoots_int16_inputs_on_both_signs(bases):
    case = gc.clip16(bases(REDUCE_TREE64P))
    x = case[1][0][1]
    assert np.array_equal(x, np.clip(np.rint(x), -32768, 32767))
    y, _ = gc.play(rc.OracleEngine(OracleNs, gc.S, REDUCE_TREE64P), case)
    for s in range(gc.S):
        assert (y[:, s] == 32767).any() and (y[:, s] == -32768).any(), s
    assert (np.abs(y) < 32767).any(axis=2).all()   # no frame saturates throughout: waves take both paths


def _squared_magnitudes(st):
    """the 129 squared magnitudes of the frame the state has just analysed, as the step forms them (float32, product
    and sum unfused) from the exported analysis buffer, and that frame's energy"""
    w = oracle_lib.oracle_table("window", 256)
    a = np.array(st.analyzeBuf[:], np.float32) * w
    energy = np.float32(0)
    for v in a:
        energy += v * v
    spec = OracleNs(1).rdft256(a[None, :], 1)[0]
    re, im = spec[0::2].copy(), spec[1::2].copy()
    r128 = im[0]
    im[0] = 0
    m2 = np.concatenate([re * re + im * im, [r128 * r128]]).astype(np.float32)
    return m2, energy


def test_tiny_runs_the_squared_magnitudes_through_normal_subnormal_and_zero(bases):
    case = gc.tiny(bases(REDUCE_TREE64P))
    x = np.concatenate([op[1] for op in case[1]])
    assert np.abs(x[0]).max() <= 2.0 ** -40 and np.abs(x[-1]).max() <= 2.0 ** -75 and (x[-1] != 0).any()
    y, ex = _frame_by_frame(case)
    assert np.isfinite(y).all()
    tiny_f = np.float32(2.0 ** -126)
    seen = {"normal": 0, "below 2^-100": 0, "subnormal": 0, "zero": 0}
    zero_energy = np.zeros((len(ex), gc.S), bool)
    for f, states in enumerate(ex):
        for s, st in enumerate(states):
            m2, energy = _squared_magnitudes(st)
            zero_energy[f, s] = energy == 0
            if energy == 0:
                continue   # the step leaves before the transform (ns_core.c:1239-1264)
            seen["normal"] += int((m2 >= tiny_f).sum())
            seen["below 2^-100"] += int(((m2 > 0) & (m2 < np.float32(2.0 ** -100))).sum())
            seen["subnormal"] += int(((m2 > 0) & (m2 < tiny_f)).sum())
            seen["zero"] += int((m2 == 0).sum())
    assert all(v > 0 for v in seen.values()), seen
    # ... and the energy is exactly zero in some stream while another still has some
    assert (zero_energy.any(axis=1) & ~zero_energy.all(axis=1)).any()
    assert (zero_energy.any(axis=0)).sum() >= 2


@pytest.mark.parametrize("name", ["nan", "inf"])
def test_poisoned_stream_goes_non_finite_and_its_neighbours_do_not(bases, name):
    y, ex = gc.play(rc.OracleEngine(OracleNs, gc.S, REDUCE_TREE64P), gc.CASES[name](bases(REDUCE_TREE64P)))
    p = gc.POISONED[name]
    assert np.isfinite(y[:gc.POISON_FRAME]).all()
    assert not np.isfinite(y[gc.POISON_FRAME:, p]).any()
    assert np.isfinite(np.delete(y, p, axis=1)).all()


def test_publish_changes_the_quantile_in_the_named_steps_with_steady_steps_around(bases):
    case = gc.publish(bases(REDUCE_TREE64P))
    assert {tuple(sorted(cs.values())) for cs in gc.PUBLISH_COUNTERS.values()} >= {(198, 199, 200)}
    _, ex = _frame_by_frame(case)
    for s in range(gc.S):
        q = [np.array(case[0][s].quantile[:])] + [np.array(states[s].quantile[:]) for states in ex]
        changed = [f for f in range(gc.PUBLISH_FRAMES) if not np.array_equal(q[f], q[f + 1])]
        assert changed == gc.publish_steps(s), (s, changed)
        before = [case[0][s]] + [states[s] for states in ex[:-1]]
        steady = [rc.steady_steps(st, [True]) == 1 for st in before]
        for f in changed:   # the publish itself is a generic step
            assert not steady[f]
        assert any(steady) and steady[-1]
    walk8 = lambda f: f // 8
    # a publish in a walk's first, a middle and its last step (walks of 8 and of 3), two in consecutive steps, and a steady
    # step in front of a publish in the same walk of 8
    steps = sorted(set(sum((gc.publish_steps(s) for s in range(gc.S)), [])))
    assert {f % 8 for f in steps} >= {0, 4, 7} and {f % 3 for f in steps} == {0, 1, 2}
    assert any(b == a + 1 for s in range(gc.S) for a, b in zip(gc.publish_steps(s), gc.publish_steps(s)[1:]))
    s = 1
    f = gc.publish_steps(s)[0]
    before = [case[0][s]] + [states[s] for states in ex[:-1]]
    assert any(rc.steady_steps(before[g], [True]) == 1 for g in range(8 * walk8(f), f))


def test_policy_makes_the_middle_call_generic_and_the_others_steady(bases):
    case = gc.policy_inside(bases(REDUCE_TREE64P))
    _, (first, middle, last) = gc.play(rc.OracleEngine(OracleNs, gc.S, REDUCE_TREE64P), case)
    for s in (1, 4):
        assert rc.steady_steps(case[0][s], [True] * 9) == 9
        assert first[s].gainmap == 1 and middle[s].gainmap == 0 and last[s].gainmap == 1
    assert middle[0].gainmap == 1


def _assert_bitwise(got, want, what, poisoned=None):
    (ya, ea), (yb, eb) = got, want
    if poisoned is not None:   # non-finite outputs as a mask; its state holds NaNs, whose payloads are not compared
        assert np.array_equal(np.isfinite(ya[:, poisoned]), np.isfinite(yb[:, poisoned])), what
        ya, yb = np.where(np.isfinite(ya), ya, 0), np.where(np.isfinite(yb), yb, 0)
    bad = np.nonzero((ya.view(np.uint32) != yb.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, "first differing frame / stream", bad[0][:3], bad[1][:3])
    for k, (a, b) in enumerate(zip(ea, eb)):
        for s in range(len(a)):
            if s != poisoned:
                assert state_diff(a[s], b[s], skip=set()) == {}, (what, "export", k, "stream", s)


@needs_ref
@pytest.mark.parametrize("policy", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(gc.NEW_CASES))
def test_oracle_equals_reference_and_the_reference_stays_finite(bases, name, policy):
    case = gc.NEW_CASES[name](bases(REDUCE_SEQ, policy))
    want = gc.play(rc.RefEngine(oracle_lib.RefNs, gc.S, policy), case)
    p = gc.POISONED.get(name)
    for s in range(gc.S):   # the reference on its finite inputs
        if s != p:
            assert np.isfinite(want[0][:, s]).all(), (name, s)
            for states in want[1]:
                for field in FLOAT_ROWS:
                    assert np.isfinite(np.array(getattr(states[s], field)[:])).all(), (name, s, field)
    got = gc.play(rc.OracleEngine(OracleNs, gc.S, REDUCE_SEQ, policy), case)
    _assert_bitwise(got, want, (name, policy), p)
