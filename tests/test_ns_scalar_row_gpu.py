"""The scalar row of the pair-layout NS frame step (ns_kernels1.hip, ScalarRow): in the hand-off build's product kernels
the float scalars and most bin-128 row tails have their master copy in the wave's LDS image, the integer scalars and
the trackers' tails on the lanes of a register that goes back to the image at a walk's end.  What can go wrong is a
stale copy: a register lane written over the image, a step that reads a value its predecessor wrote through the other
copy, a scalar the host changed between two launches.

Every case of tests/ns_scalar_row_cases.py (asserted to reach what it names in tests/test_ns_scalar_row_oracle.py) runs
from imported steady-state states for tens of frames; outputs and every exported state array -- the whole scalar row
included -- are compared bit for bit with OracleNs in the kernel's association (REDUCE_TREE64P), behind every call, with
the hand-off build on (walks of 1, 3 and 8) and off, the steady body on and off, float and int16 frames."""
import numpy as np
import pytest

from tests import ns_scalar_row_cases as rc
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_TREE64P, OracleNs

pytestmark = pytest.mark.gpu

# (hand-off build, steps per walk, steady body, int16 frames)
VARIANTS = [(flow, walk, steady, s16) for flow, walk in ((1, 1), (1, 3), (1, 8), (0, 0)) for steady in (1, 0)
            for s16 in (False, True)]
CASES = {"uneven": rc.uneven_calls, "zero": rc.zero_energy, "generic": rc.generic_inside_walk,
         "between": rc.scalars_between_launches}


@pytest.fixture(scope="module")
def ns():
    from audiosignalprocess_amd import ns as mod

    assert mod.device_count() >= 1, "GPU tests need a HIP device"
    return mod


class GpuEngine:
    """NsBatch (kernel 3) behind play()'s five methods"""

    def __init__(self, ns, n_streams, flow, walk, steady, s16=False, counts=False):
        self.g = ns.NsBatch(n_streams, policy=1, kernel=3)
        self.g.set_flow(flow)
        self.g.set_split(1)
        self.g.set_flow_walk(walk)
        self.g.set_steady(steady)
        if counts:
            self.g.debug_step_counts(True)
        self.s16 = s16
        self.import_state, self.export_state = self.g.import_state, self.g.export_state
        self.set_policy_stream, self.init_stream = self.g.set_policy_stream, self.g.init_stream

    def run(self, x):
        if self.s16:
            return self.g.analyze_process_s16(x.astype(np.int16)).astype(np.float32)
        return self.g.analyze_process(x)


def _s16(y):
    """FloatS16ToS16 of a float output: the kernel's int16 store (ns_pair_fft.h, store2p)"""
    pos = np.where(y >= np.float32(32766.5), 32767, (y + np.float32(0.5)).astype(np.int32))
    neg = np.where(y <= np.float32(-32767.5), -32768, (y - np.float32(0.5)).astype(np.int32))
    return np.where(y > 0, pos, neg).astype(np.int16).astype(np.float32)


@pytest.fixture(scope="module")
def wanted():
    """name -> (case, oracle outputs, oracle exports); computed once, shared by every variant"""
    cache, bases = {}, {}

    def get(name):
        if name not in cache:
            n = 8 if name == "full" else rc.S
            if n not in bases:
                bases[n] = rc.base_states(OracleNs, REDUCE_TREE64P, n)
            case = (rc.full_workgroups if name == "full" else CASES[name])(bases[n])
            y, ex = rc.play(rc.OracleEngine(OracleNs, n, REDUCE_TREE64P), case)
            y.setflags(write=False)
            cache[name] = (case, y, ex)
        return cache[name]

    return get


def _assert_same(got, y_want, ex_want, s16, what):
    y, ex = got
    yw = _s16(y_want) if s16 else y_want
    bad = np.nonzero((y.view(np.uint32) != yw.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, "first differing frame / stream", bad[0][:3], bad[1][:3])
    assert len(ex) == len(ex_want)
    for k, (a, b) in enumerate(zip(ex, ex_want)):
        for s in range(len(b)):
            assert state_diff(a[s], b[s]) == {}, (what, "export", k, "stream", s)


@pytest.mark.parametrize("flow,walk,steady,s16", VARIANTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_oracle_bit_for_bit(ns, wanted, name, flow, walk, steady, s16):
    case, y_want, ex_want = wanted(name)
    eng = GpuEngine(ns, rc.S, flow, walk, steady, s16)
    got = rc.play(eng, case)
    eng.g.close()
    _assert_same(got, y_want, ex_want, s16, (name, flow, walk, steady, s16))


def test_full_workgroups_split_step_counts_and_outputs(ns, wanted):
    """8 streams, walks of 8, 16 frames: the diagnostic kernels count, per stream, the steps each body took -- what
    the imported scalars dictate -- and compute what the oracle computes; so do the product kernels."""
    case, y_want, ex_want = wanted("full")
    expect = [rc.steady_steps(st, [True] * 16) for st in case[0]]
    eng = GpuEngine(ns, 8, 1, 8, 1, counts=True)
    got = rc.play(eng, case)
    cnt = eng.g.debug_step_counts(False)
    eng.g.close()
    print("steady / generic steps per stream:", cnt.tolist(), "expected steady:", expect)
    _assert_same(got, y_want, ex_want, False, "full, diagnostic kernels")
    assert (cnt.sum(axis=1) == 16).all()
    assert cnt[:, 0].tolist() == expect
    eng = GpuEngine(ns, 8, 1, 8, 1)
    got = rc.play(eng, case)
    eng.g.close()
    _assert_same(got, y_want, ex_want, False, "full, product kernels")


def test_zero_energy_steps_take_neither_body(ns, wanted):
    case, y_want, ex_want = wanted("zero")
    live = [[not (s == 1 and f in rc.ZERO_STEPS) for f in range(24)] for s in range(rc.S)]
    expect = [rc.steady_steps(st, live[s]) for s, st in enumerate(case[0])]
    eng = GpuEngine(ns, rc.S, 1, 8, 1, counts=True)
    got = rc.play(eng, case)
    cnt = eng.g.debug_step_counts(False)
    eng.g.close()
    _assert_same(got, y_want, ex_want, False, "zero, diagnostic kernels")
    assert cnt.sum(axis=1).tolist() == [24, 24 - len(rc.ZERO_STEPS), 24, 24, 24]
    assert cnt[:, 0].tolist() == expect
