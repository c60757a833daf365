"""What the hand-off build of the pair-layout NS frame step (ns_kernels1.hip) carries in registers across the steps of
a walk: the previous-frame SNR estimate (step t's gq1 * gain is step t + 1's magnPrev / (noisePrev + 0.0001f) * smooth),
valid only behind a step of the same walk that set it; and the trackers' counter terms, which every ns_frame1 kernel now
reads from NsTables::cnt_terms.

Every case of tests/ns_carry_cases.py (asserted to reach what it names in tests/test_ns_carry_oracle.py) runs five
streams -- a full workgroup and a partial one -- from imported steady-state states; outputs and every exported state
array are compared bit for bit with OracleNs in the kernel's association (REDUCE_TREE64P), behind every call, with the
hand-off build on (walks of 1, 2, 3 and 8) and off, the steady body on and off, float and int16 frames."""
import numpy as np
import pytest

from tests import ns_carry_cases as cc
from tests import ns_scalar_row_cases as rc
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_TREE64P, OracleNs

pytestmark = pytest.mark.gpu

# (hand-off build, steps per walk, steady body, int16 frames)
VARIANTS = [(flow, walk, steady, s16) for flow, walk in ((1, 1), (1, 2), (1, 3), (1, 8), (0, 0)) for steady in (1, 0)
            for s16 in (False, True)]


@pytest.fixture(scope="module")
def ns():
    from audiosignalprocess_amd import ns as mod

    assert mod.device_count() >= 1, "GPU tests need a HIP device"
    return mod


class GpuEngine:
    """NsBatch (kernel 3) behind play()'s methods"""

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
    cache, base = {}, []

    def get(name):
        if name not in cache:
            if not base:
                base.append(rc.base_states(OracleNs, REDUCE_TREE64P, cc.S))
            case = cc.CASES[name](base[0])
            y, ex = cc.play(rc.OracleEngine(OracleNs, cc.S, REDUCE_TREE64P), case)
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
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_case_equals_the_oracle_bit_for_bit(ns, wanted, name, flow, walk, steady, s16):
    case, y_want, ex_want = wanted(name)
    eng = GpuEngine(ns, cc.S, flow, walk, steady, s16)
    got = cc.play(eng, case)
    eng.g.close()
    _assert_same(got, y_want, ex_want, s16, (name, flow, walk, steady, s16))


@pytest.mark.parametrize("name", ["generic", "zero", "laps"])
def test_the_diagnostic_kernels_carry_too(ns, wanted, name):
    """The diagnostic hand-off kernel is the same text with the same carry (it did not need the product kernels'
    exemption): walks of 8, the step counts on, the same bits."""
    case, y_want, ex_want = wanted(name)
    eng = GpuEngine(ns, cc.S, 1, 8, 1, counts=True)
    got = cc.play(eng, case)
    cnt = eng.g.debug_step_counts(False)
    eng.g.close()
    _assert_same(got, y_want, ex_want, False, (name, "diagnostic kernels"))
    if name == "laps":   # the three publishes and their neighbours are the only generic steps
        assert (cnt.sum(axis=1) == cc.LAP_FRAMES).all()
        assert cnt[:, 0].tolist() == [rc.steady_steps(st, [True] * cc.LAP_FRAMES) for st in case[0]]
