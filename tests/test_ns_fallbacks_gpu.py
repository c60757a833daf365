"""What the steady step of the pair-layout NS frame kernel (ns_kernels1.hip) no longer does per lane or per step: the
libm fallbacks of its lean fp64 logarithms, exponentials and tanh sit behind one wave-level test each, quotients with the
numerator 1 take the reciprocal chain (frcp / frcp2), and -- hand-off build -- the histogram increments of a walk's
steady steps are recorded per step and counted once per walk.

Every case of tests/ns_fallbacks_cases.py (asserted to reach what it names in tests/test_ns_fallbacks_oracle.py) runs
five streams -- a full workgroup and a partial one -- from imported steady-state states; outputs and every exported state
array, the three histograms among them, are compared bit for bit with OracleNs in the kernel's association
(REDUCE_TREE64P) behind every call, i.e. directly behind a launch: nothing may be left pending.  Hand-off build on (walks
of 1, 3, 8, and 13, which reuses its slots) and off, the steady body on and off.

The arithmetic goes through a test seam, function 25 of AspNs_debug_compare, which sweeps on the device: every 32-bit
low word through the two-instruction rounding test and the one it replaces; every float bit pattern through frcp and
frcp2 against fdiv(1.f, x), bit for bit; every float through the wave-level log and exp forms against the one-argument
forms, alone on one lane of a wave among benign arguments (each lane in turn) and on all lanes.  A wave of positive
normal / in-range patterns is flagged in about 2 cases of 10 000, a wave of negative or NaN patterns always: both sides
of the wave-level branch are met in every arrangement."""
import ctypes as C

import numpy as np
import pytest

from tests import ns_fallbacks_cases as fc
from tests import ns_scalar_row_cases as rc
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_TREE64P, OracleNs
from tests.test_ns_carry_gpu import GpuEngine

pytestmark = pytest.mark.gpu

# (hand-off build, steps per walk, steady body)
VARIANTS = [(flow, walk, steady) for flow, walk in ((1, 1), (1, 3), (1, 8), (1, 13), (0, 0)) for steady in (1, 0)]
RUNS = [(name,) + v for name in sorted(fc.CASES) for v in VARIANTS]


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
                base.append(rc.base_states(OracleNs, REDUCE_TREE64P, fc.S))
            case = fc.CASES[name](base[0])
            y, ex = fc.play(rc.OracleEngine(OracleNs, fc.S, REDUCE_TREE64P), case)
            y.setflags(write=False)
            cache[name] = (case, y, ex)
        return cache[name]

    return get


@pytest.mark.parametrize("name,flow,walk,steady", RUNS)
def test_case_equals_the_oracle_bit_for_bit(ns, wanted, name, flow, walk, steady):
    case, y_want, ex_want = wanted(name)
    eng = GpuEngine(ns, fc.S, flow, walk, steady)
    y, ex = fc.play(eng, case)
    eng.g.close()
    what = (name, flow, walk, steady)
    bad = np.nonzero((y.view(np.uint32) != y_want.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, "first differing frame / stream", bad[0][:3], bad[1][:3])
    assert len(ex) == len(ex_want)
    for k, (a, b) in enumerate(zip(ex, ex_want)):
        for s in range(len(b)):
            assert state_diff(a[s], b[s]) == {}, (what, "export", k, "stream", s)
            for field in fc.HIST_FIELDS:   # (named: the counts are what this module is about)
                assert np.array_equal(np.array(getattr(a[s], field)[:]), np.array(getattr(b[s], field)[:])), \
                    (what, "export", k, "stream", s, field)


# what function 25 sweeps (its fn_b)
SWEEPS = {0: "rounding test, every low word", 1: "frcp / frcp2 against fdiv(1.f, x)", 2: "log, alone on a lane",
          3: "log, all lanes", 4: "exp, alone on a lane", 5: "exp, all lanes"}


@pytest.mark.parametrize("what", sorted(SWEEPS))
def test_sweep_every_bit_pattern(ns, what):
    lib = ns.load_library()
    lib.AspNs_debug_compare.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.c_float, C.c_int]
    total, examples = 0, []
    step = 1 << 28
    for start in range(0, 1 << 32, step):
        n_bad, bad = C.c_uint32(0), (C.c_uint32 * 64)()
        assert lib.AspNs_debug_compare(25, what, start, step, C.byref(n_bad), bad, 0.0, 0) == 0
        total += n_bad.value
        examples += list(bad[:min(n_bad.value, 64)])
    assert total == 0, (SWEEPS[what], total, [hex(b) for b in examples[:8]])


def test_sweep_seam_refuses_what_it_does_not_know(ns):
    lib = ns.load_library()
    lib.AspNs_debug_compare.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.c_float, C.c_int]
    n_bad, bad = C.c_uint32(0), (C.c_uint32 * 64)()
    assert lib.AspNs_debug_compare(25, 6, 0, 256, C.byref(n_bad), bad, 0.0, 0) != 0
