"""The short division chains of the pair-layout NS frame kernel (ns_kernels1.hip): the trackers' FACTOR / max(density, 1)
without the reciprocal's refinement (fdiv40 / fdiv40_2), gainPrior with one quotient correction (fdiv_1c), the sums
divided by the bin count two at a time (div_by_uniform2), the logarithm's reduced argument in one instruction
(log_reduced_bits_mad), the square root with one correction instead of a refinement and a correction, and its
tiny-argument test as one compare per argument for the wave.

The arithmetic goes through a test seam, function 26 of AspNs_debug_compare, which runs each new form beside the form it
replaces on every 32-bit pattern of its one free operand -- 64 consecutive patterns to a wave -- and counts the patterns
whose bits differ (NaN on both sides counts as equal): all 2^32 patterns through max(., 1) and both divisions by it, +inf
and NaNs included; all 2^32 patterns as priorSpeechProb through ns_prior_update's clamps and both divisions; all 2^32
patterns through both argument reductions and both table logarithms; all 2^32 patterns through the packed and the plain
division by 129; every non-negative float and every NaN through the square root with one correction and the one that
refines first.  Zero differences are asserted for each.  (The square root's equality with one correction holds for the
reciprocal square root instruction of this device, not for every 1-ulp seed: the sweep is the proof and runs with the
suite.  Function 24, tests/test_ns_guards_gpu.py, sweeps the same square root and its wave-level tiny-argument test
against sqrtf on every float; function 25, tests/test_ns_fallbacks_gpu.py, the wave-level logarithm, which now reduces
its argument in one instruction.)

The step: the cases of tests/ns_shortdiv_cases.py (asserted to reach what they name in tests/test_ns_shortdiv_oracle.py)
run five streams from imported steady-state states in calls of 1, 2, 7, 13 and 17 frames; outputs and every exported
state array are compared bit for bit with OracleNs in the kernel's association (REDUCE_TREE64P) behind every call.
Hand-off build on (walks of 1, 3 and 8) and off, the steady body on and off, float and int16 frames."""
import ctypes as C

import numpy as np
import pytest

from tests import ns_scalar_row_cases as rc
from tests import ns_shortdiv_cases as sc
from tests.conftest import state_diff
from tests.oracle_lib import REDUCE_TREE64P, OracleNs
from tests.test_ns_carry_gpu import GpuEngine, _s16

pytestmark = pytest.mark.gpu

# (hand-off build, steps per walk, steady body, int16 frames)
VARIANTS = [(flow, walk, steady, s16) for flow, walk in ((1, 1), (1, 3), (1, 8), (0, 0)) for steady in (1, 0)
            for s16 in (False, True)]
RUNS = [(name,) + v for name in sorted(sc.CASES) for v in VARIANTS if not (v[3] and name in sc.FLOAT_ONLY)]


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
                base.append(rc.base_states(OracleNs, REDUCE_TREE64P, sc.S))
            case = sc.CASES[name](base[0])
            y, ex = sc.play(rc.OracleEngine(OracleNs, sc.S, REDUCE_TREE64P), case)
            y.setflags(write=False)
            cache[name] = (case, y, ex)
        return cache[name]

    return get


@pytest.mark.parametrize("name,flow,walk,steady,s16", RUNS)
def test_case_equals_the_oracle_bit_for_bit(ns, wanted, name, flow, walk, steady, s16):
    case, y_want, ex_want = wanted(name)
    eng = GpuEngine(ns, sc.S, flow, walk, steady, s16)
    y, ex = sc.play(eng, case)
    eng.g.close()
    what = (name, flow, walk, steady, s16)
    yw = _s16(y_want) if s16 else y_want
    bad = np.nonzero((y.view(np.uint32) != yw.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, "first differing frame / stream", bad[0][:3], bad[1][:3])
    assert len(ex) == len(ex_want) == len(sc.CALLS)
    for k, (a, b) in enumerate(zip(ex, ex_want)):
        for s in range(len(b)):
            assert state_diff(a[s], b[s]) == {}, (what, "export", k, "stream", s)


# what function 26 sweeps (its fn_b) for the forms the step uses
SWEEPS = {0: "fdiv40 / fdiv40_2 against fdiv(FACTOR, max(x, 1))",
          1: "gainPrior: fdiv_1c against fdiv behind the clamps",
          2: "the logarithm's reduced argument and the table logarithm behind it",
          3: "div_by_uniform2 against div_by_uniform, divisor 129",
          4: "fsqrt_wave (one correction) against fsqrt, non-negative floats and NaNs"}
# candidates the step does not use (profiles/README.md records their counts): nothing is asserted of them
CANDIDATES = {5: "phase-8 quotient with one correction", 6: "square root with h unrefined"}


def _sweep(lib, what):
    lib.AspNs_debug_compare.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.c_float, C.c_int]
    total, examples = 0, []
    step = 1 << 28
    for start in range(0, 1 << 32, step):
        n_bad, bad = C.c_uint32(0), (C.c_uint32 * 64)()
        assert lib.AspNs_debug_compare(26, what, start, step, C.byref(n_bad), bad, 0.0, 0) == 0
        total += n_bad.value
        examples += list(bad[:min(n_bad.value, 64)])
    return total, examples


@pytest.mark.parametrize("what", sorted(SWEEPS))
def test_sweep_every_bit_pattern(ns, what):
    total, examples = _sweep(ns.load_library(), what)
    print("function 26, %d (%s): %d patterns differ" % (what, SWEEPS[what], total))
    assert total == 0, (SWEEPS[what], total, [hex(b) for b in examples[:8]])


def test_sweep_seam_refuses_what_it_does_not_know(ns):
    lib = ns.load_library()
    lib.AspNs_debug_compare.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.c_float, C.c_int]
    n_bad, bad = C.c_uint32(0), (C.c_uint32 * 64)()
    assert lib.AspNs_debug_compare(26, len(SWEEPS) + len(CANDIDATES), 0, 256, C.byref(n_bad), bad, 0.0, 0) != 0
    assert lib.AspNs_debug_compare(26, -1, 0, 256, C.byref(n_bad), bad, 0.0, 0) != 0
