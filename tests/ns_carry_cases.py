"""Inputs for tests/test_ns_carry_oracle.py (CPU) and tests/test_ns_carry_gpu.py: what a wave of the hand-off build of
ns_kernels1.hip keeps in registers from one step of its walk to the next -- the previous-frame SNR estimate
magnPrev / (noisePrev + 0.0001f) * smooth, which the next step would otherwise divide out again from the three rows this
step stores -- and the trackers' counter terms, read from a table by the counters' values.  What can go wrong is a carry
that outlives its walk (the host, InitStream or an import rewrote the rows behind it), one that is used although no step
of this walk set it, and a table entry that is not what the step used to compute.  No tests in here.

A case is what tests/ns_scalar_row_cases.py calls one, with a fourth operation:

    ("import", stream, state)       import_state of one stream between two calls

Four cases are that module's own (uneven calls, zero-energy steps as a walk's first, middle and last, generic steps
inside a walk with steady ones behind them); the others are below."""
import numpy as np

from tests import ns_cases
from tests import ns_scalar_row_cases as rc

S = rc.S
BASE_FRAMES = rc.BASE_FRAMES
COUNTERS0 = (0, 67, 133)   # where the three trackers start in the 210-frame case: one lap of each, every table entry read
LAP_FRAMES = 210
STARTUP_CALLS = (30, 34)   # a fresh stream's first 64 frames: blockInd passes END_STARTUP_SHORT (50) in the second call


def between_launches(base):
    """set_policy of stream 2 (mode 3), Init of stream 3 and an import into stream 1 (the state stream 0 started from,
    230 frames of another signal) between two calls: nothing a wave held at the first call's end may reach the second"""
    x = rc._frames(len(base), 18, BASE_FRAMES)
    ops = [("run", x[:9]), ("policy", 2, 3), ("init", 3), ("import", 1, ns_cases.copy_state(base[0])), ("run", x[9:])]
    return [ns_cases.copy_state(b) for b in base], ops


def counter_laps(base):
    """210 frames in one call with the trackers at 0, 67 and 133: counter 0 takes every value 0 .. 200, each tracker
    publishes and wraps once (steps 200, 133 and 67, generic with their neighbours; every other step is steady)"""
    states = [ns_cases.copy_state(b) for b in base]
    for st in states:
        for k, c in enumerate(COUNTERS0):
            st.counter[k] = c
    return states, [("run", rc._frames(len(base), LAP_FRAMES, BASE_FRAMES))]


def startup(base):
    """every stream Init'ed, then its first 64 frames in two calls: the start-up noise model and the blended gain
    (ns_core.c:1268-1301) -- the carried product is gq1 times the BLENDED gain, which is what `smooth` holds"""
    x = rc._frames(len(base), sum(STARTUP_CALLS), 0)
    ops = [("init", s) for s in range(len(base))]
    ops += [("run", x[:STARTUP_CALLS[0]]), ("run", x[STARTUP_CALLS[0]:])]
    return [ns_cases.copy_state(b) for b in base], ops


CASES = {"uneven": rc.uneven_calls, "zero": rc.zero_energy, "generic": rc.generic_inside_walk,
         "between": between_launches, "laps": counter_laps, "startup": startup}


def play(engine, case):
    """rc.play with the "import" operation"""
    states, ops = case
    for s, st in enumerate(states):
        engine.import_state(s, st)
    ys, exports = [], []
    for op in ops:
        if op[0] == "run":
            ys.append(engine.run(op[1]))
            exports.append([engine.export_state(s) for s in range(len(states))])
        elif op[0] == "policy":
            engine.set_policy_stream(op[1], op[2])
        elif op[0] == "import":
            engine.import_state(op[1], op[2])
        else:
            engine.init_stream(op[1])
    return np.concatenate(ys), exports
