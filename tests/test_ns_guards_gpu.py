"""The wave-level guards of the pair-layout NS frame step (ns_kernels1.hip): emitted samples saturated only where some
lane of the wave holds one outside the int16 range, the square root's pass-through of zero and +inf only where some lane
holds such an argument, and -- hand-off build, steady body -- the refined reciprocal of quant + 0.0001f kept from one
steady step of a walk to the next, until a generic step (every publish is one) or the walk ends.

Every case of tests/ns_guards_cases.py (asserted to reach what it names in tests/test_ns_guards_oracle.py) runs five
streams -- a full workgroup and a partial one -- from imported steady-state states; outputs and every exported state
array are compared bit for bit with OracleNs in the kernel's association (REDUCE_TREE64P), behind every call, with the
hand-off build on (walks of 1, 3 and 8) and off, the steady body on and off, float and int16 frames (the cases whose
frames are no int16 values: float only).  In the two cases with a NaN or +inf sample, the stream that holds it is
compared on its outputs alone -- where they are finite, bit for bit, and as a mask where they are not -- because the CPU
and the device need not agree on a NaN's payload; its four neighbours are compared in full.

The guards themselves go through a test seam, function 24 of AspNs_debug_compare: over EVERY float bit pattern, 64
consecutive patterns to a wave, the sample a wave emits equals sat16p of it and fsqrt_wave equals sqrtf."""
import ctypes as C

import numpy as np
import pytest

from tests import ns_guards_cases as gc
from tests import ns_scalar_row_cases as rc
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_TREE64P, OracleNs
from tests.test_ns_carry_gpu import GpuEngine, _s16

pytestmark = pytest.mark.gpu

# (hand-off build, steps per walk, steady body, int16 frames)
VARIANTS = [(flow, walk, steady, s16) for flow, walk in ((1, 1), (1, 3), (1, 8), (0, 0)) for steady in (1, 0)
            for s16 in (False, True)]
RUNS = [(name,) + v for name in sorted(gc.CASES) for v in VARIANTS if not (v[3] and name in gc.FLOAT_ONLY)]


@pytest.fixture(scope="module")
def ns():
    from audiosignalprocess_amd import ns as mod

    assert mod.device_count() >= 1, "GPU tests need a HIP device"
    return mod


@pytest.fixture(scope="module")
def wanted():
    """name -> (case, oracle outputs, oracle exports); computed once, shared by every variant"""
    cache, base = {}, []

    def get(name):
        if name not in cache:
            if not base:
                base.append(rc.base_states(OracleNs, REDUCE_TREE64P, gc.S))
            case = gc.CASES[name](base[0])
            y, ex = gc.play(rc.OracleEngine(OracleNs, gc.S, REDUCE_TREE64P), case)
            y.setflags(write=False)
            cache[name] = (case, y, ex)
        return cache[name]

    return get


def _assert_same(got, y_want, ex_want, s16, what, poisoned=None):
    y, ex = got
    yw = _s16(y_want) if s16 else y_want
    if poisoned is not None:
        assert np.array_equal(np.isfinite(y[:, poisoned]), np.isfinite(yw[:, poisoned])), (what, "non-finite outputs")
        y, yw = np.where(np.isfinite(y), y, np.float32(0)), np.where(np.isfinite(yw), yw, np.float32(0))
    bad = np.nonzero((y.view(np.uint32) != yw.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, "first differing frame / stream", bad[0][:3], bad[1][:3])
    assert len(ex) == len(ex_want)
    for k, (a, b) in enumerate(zip(ex, ex_want)):
        for s in range(len(b)):
            if s != poisoned:
                assert state_diff(a[s], b[s]) == {}, (what, "export", k, "stream", s)


@pytest.mark.parametrize("name,flow,walk,steady,s16", RUNS)
def test_case_equals_the_oracle_bit_for_bit(ns, wanted, name, flow, walk, steady, s16):
    case, y_want, ex_want = wanted(name)
    eng = GpuEngine(ns, gc.S, flow, walk, steady, s16)
    got = gc.play(eng, case)
    eng.g.close()
    _assert_same(got, y_want, ex_want, s16, (name, flow, walk, steady, s16), gc.POISONED.get(name))


def test_guards_exhaustive():
    from audiosignalprocess_amd import ns

    assert ns.device_count() >= 1, "GPU tests need a HIP device"
    lib = ns.load_library()
    lib.AspNs_debug_compare.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.c_float, C.c_int]
    total, examples = 0, []
    step = 1 << 28
    for start in range(0, 1 << 32, step):
        n_bad, bad = C.c_uint32(0), (C.c_uint32 * 64)()
        assert lib.AspNs_debug_compare(24, 9, start, step, C.byref(n_bad), bad, 0.0, 0) == 0
        total += n_bad.value
        examples += list(bad[:min(n_bad.value, 64)])
    assert total == 0, (total, [hex(b) for b in examples[:8]])
    # the seam exists beside sqrtf (and sat16p) only
    n_bad, bad = C.c_uint32(0), (C.c_uint32 * 64)()
    assert lib.AspNs_debug_compare(24, 10, 0, 256, C.byref(n_bad), bad, 0.0, 0) != 0
