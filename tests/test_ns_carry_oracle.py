"""The inputs of tests/ns_carry_cases.py on the CPU: each case reaches what it names (asserted from the oracle's exported
states; the four cases shared with tests/ns_scalar_row_cases.py are asserted in tests/test_ns_scalar_row_oracle.py), the
table of counter terms the kernels read is the arithmetic they used to do, and at these inputs the oracle IS the
reference -- OracleNs(REDUCE_SEQ) against the compiled reference, outputs and every state field bit for bit, at
policies 0..3."""
import ctypes as C

import numpy as np
import pytest

from tests import ns_carry_cases as cc
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
            cache[(mode, policy)] = rc.base_states(OracleNs, mode, cc.S, policy)
        return cache[(mode, policy)]

    return get


def _engine(case, mode=REDUCE_TREE64P, policy=1):
    o = rc.OracleEngine(OracleNs, len(case[0]), mode, policy)
    for s, st in enumerate(case[0]):
        o.import_state(s, st)
    return o


def test_the_shared_cases_put_zero_energy_steps_first_middle_and_last_in_walks_of_2_3_and_8():
    assert {f % 8 for f in rc.ZERO_STEPS} >= {0, 4, 7} and {f % 3 for f in rc.ZERO_STEPS} == {0, 1, 2}
    assert {f % 2 for f in rc.ZERO_STEPS} == {0, 1}   # (a walk of 2 has no middle)


def test_between_launches_rewrites_what_the_first_call_left(bases):
    base = bases(REDUCE_TREE64P)
    case = cc.between_launches(base)
    _, (first, last) = cc.play(rc.OracleEngine(OracleNs, cc.S, REDUCE_TREE64P), case)
    # the import: stream 1 goes on from stream 0's base state, whose three rows are not the ones its own first call left
    for field in ("smooth", "magnPrevAnalyze", "noisePrev"):
        assert not np.array_equal(np.array(getattr(first[1], field)[:]), np.array(getattr(base[0], field)[:])), field
    assert last[1].blockInd == rc.BASE_FRAMES - 1 + 9
    assert last[0].blockInd == rc.BASE_FRAMES - 1 + 18
    # ... and computes, on stream 1's frames, what a batch that never ran the first call computes from that state
    x = case[1][-1][1]
    alone = rc.OracleEngine(OracleNs, cc.S, REDUCE_TREE64P)
    for s in range(cc.S):
        alone.import_state(s, base[0])
    alone.run(x)
    assert state_diff(alone.export_state(1), last[1]) == {}
    assert last[2].overdrive == np.float32(1.25) and last[2].denoiseBound == np.float32(0.09)
    assert last[3].blockInd == 8 and last[3].gainmap == 0


def test_counter_laps_read_every_table_entry_and_wrap_each_counter_once(bases):
    case = cc.counter_laps(bases(REDUCE_TREE64P))
    x = case[1][0][1]
    assert x.shape[0] == cc.LAP_FRAMES
    o = _engine(case)
    seen = [[], [], []]
    steady = []
    for f in range(cc.LAP_FRAMES):
        st = o.export_state(0)
        for k in range(3):
            seen[k].append(st.counter[k])
        steady.append(rc.steady_steps(st, [True]) == 1)
        o.run(x[f:f + 1])
    assert sorted(set(seen[0])) == list(range(201))
    for k in range(3):
        assert sum(b < a for a, b in zip(seen[k], seen[k][1:])) == 1, k   # one wrap
        assert max(seen[k]) == 200 and min(seen[k]) >= 0
    # generic: the step that enters with a counter at 199 and the one at 200 (the publish); steady steps consume both
    assert [f for f, s in enumerate(steady) if not s] == [66, 67, 132, 133, 199, 200]


def test_startup_streams_stay_inside_the_window_then_leave_it(bases):
    case = cc.startup(bases(REDUCE_TREE64P))
    _, (first, last) = cc.play(rc.OracleEngine(OracleNs, cc.S, REDUCE_TREE64P), case)
    for s in range(cc.S):
        assert first[s].blockInd == cc.STARTUP_CALLS[0] - 1 < 49
        assert last[s].blockInd == sum(cc.STARTUP_CALLS) - 1 > 50
        assert rc.steady_steps(first[s], [True] * cc.STARTUP_CALLS[1]) == 0


def test_counter_terms_table_is_the_arithmetic_it_replaces(built_lib):
    """NsTables::cnt_terms, the last member: entry n = {(float)n, (float)(n + 1), 1.0f / (float)(n + 1), 0}"""
    lib = C.CDLL(built_lib)
    lib.AspNs_host_tables_size.restype = C.c_size_t
    lib.AspNs_host_tables.argtypes = [C.c_void_p, C.c_size_t]
    n = lib.AspNs_host_tables_size()
    buf = np.zeros(n // 4, np.float32)
    assert lib.AspNs_host_tables(buf.ctypes.data, n) == 0
    t = buf[-201 * 4:].reshape(201, 4)
    k = np.arange(201, dtype=np.float32)
    assert np.array_equal(t[:, 0], k) and np.array_equal(t[:, 1], k + np.float32(1))
    assert np.array_equal(t[:, 2].view(np.uint32), (np.float32(1) / (k + np.float32(1))).view(np.uint32))
    assert not t[:, 3].any()


def _assert_bitwise(got, want, what):
    (ya, ea), (yb, eb) = got, want
    bad = np.nonzero((ya.view(np.uint32) != yb.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, "first differing frame / stream", bad[0][:3], bad[1][:3])
    for k, (a, b) in enumerate(zip(ea, eb)):
        for s in range(len(a)):
            assert state_diff(a[s], b[s], skip=set()) == {}, (what, "export", k, "stream", s)


@needs_ref
@pytest.mark.parametrize("policy", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_oracle_equals_reference(bases, name, policy):
    case = cc.CASES[name](bases(REDUCE_SEQ, policy))
    want = cc.play(rc.RefEngine(oracle_lib.RefNs, cc.S, policy), case)
    got = cc.play(rc.OracleEngine(OracleNs, cc.S, REDUCE_SEQ, policy), case)
    _assert_bitwise(got, want, (name, policy))
