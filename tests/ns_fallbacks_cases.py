"""Inputs for tests/test_ns_fallbacks_oracle.py (CPU) and tests/test_ns_fallbacks_gpu.py: the histogram increments that
the hand-off build of ns_kernels1.hip no longer issues in every steady step -- a step records its three feature values in
a slot of the wave's LDS, and the bin arithmetic and the atomic adds run once per walk (hist_flush), in front of a
generic step's own histogram work and in front of a record that would reuse a slot.  What can go wrong is a count that
is lost or made twice (a walk's end, a slot reused, a flush with empty slots), a window that closes over histograms whose
pending counts have not arrived, a count left pending when the host reads, rewrites or re-initialises the state, and a
feature outside its histogram's range that is counted after all.  No tests in here.

A case is what tests/ns_carry_cases.py calls one; `play` is that module's."""
import numpy as np

from tests import ns_cases
from tests import ns_carry_cases as cc
from tests import ns_guards_cases as gc
from tests import ns_scalar_row_cases as rc

S = rc.S
BASE_FRAMES = rc.BASE_FRAMES
play = cc.play

CLOSE_CALLS = (8, 8, 8)
# stream -> frames left in its feature window on entry: it closes in step (that - 1) of the 24
CLOSE_LEFT = {0: 1,   # step 0: the first step of every walk length
              1: 5,   # step 4: a middle step of a walk of 8 and of a walk of 3
              2: 8,   # step 7: the last step of a walk of 8 (and of the first call)
              3: 3,   # step 2: the last step of a walk of 3
              4: 9}   # step 8: the first step of the second call (alone in its workgroup)
# (stream, frames left) imported in front of the second and the third call: stream 0 closes again in step 9 -- a close
# in two consecutive calls -- and stream 3 in step 18
CLOSE_AGAIN = ((0, 2), (3, 3))
CLOSE_STEPS = {0: [0, 9], 1: [4], 2: [7], 3: [2, 18], 4: [8]}


def _closing(b, left):
    return ns_cases.copy_state(dict(ns_cases.close_cases(b, close_step=left))["peaks_ascending"])


def closes(base):
    """three calls of 8 frames, a window close in the places CLOSE_STEPS lists: every close is over the
    `peaks_ascending` histograms of ns_cases plus what the steps in front of it counted, and rewrites priorModelPars.
    The two steps in front of a close and the close are generic, the others steady.  The second and third close of the
    batch's streams come from a state imported between the calls (the window is the reference's 500 frames)."""
    states = [_closing(b, CLOSE_LEFT[s]) for s, b in enumerate(base)]
    x = rc._frames(len(base), sum(CLOSE_CALLS), BASE_FRAMES)
    ops, f0 = [], 0
    for c, n in enumerate(CLOSE_CALLS):
        if c > 0:
            s, left = CLOSE_AGAIN[c - 1]
            ops.append(("import", s, _closing(base[s], left)))
        ops.append(("run", x[f0:f0 + n]))
        f0 += n
    return states, ops


NO_UPDATE_STREAM = 3


def no_update(base):
    """stream 3 with modelUpdatePars[0] = 0: it never adds to a histogram and never closes (every step of it is
    generic); its four neighbours add in every step.  Calls of 8 and 16 frames."""
    states = [ns_cases.copy_state(b) for b in base]
    states[NO_UPDATE_STREAM].modelUpdatePars[0] = 0
    x = rc._frames(len(base), 24, BASE_FRAMES)
    return states, [("run", x[:8]), ("run", x[8:])]


OUT_FRAMES = 19
OUT_STREAMS = (0, 2, 4)


def out_of_range(base):
    """streams 0, 2 and 4 open their window behind a quiet history (the `quiet_history` entry of ns_cases:
    featureData[5] = 1, the spectral difference is normalised by it and lands far beyond its histogram's 100), with 400
    frames left: every step is steady and records a difference feature that must not be counted, beside an LRT and a
    flatness feature that must.  Calls of 3 and 16 frames (16: two walks of 8; a walk of 13 reuses its first slots)."""
    states = [ns_cases.copy_state(b) for b in base]
    for s in OUT_STREAMS:
        states[s] = ns_cases.copy_state(dict(ns_cases.close_cases(base[s], close_step=400))["quiet_history"])
    x = rc._frames(len(base), OUT_FRAMES, BASE_FRAMES)
    return states, [("run", x[:3]), ("run", x[3:])]


NEW_CASES = {"closes": closes, "no_update": no_update, "out_of_range": out_of_range}
# with the cases of the earlier modules that name what else the deferral must survive: calls of 1, 2, 7, 13 and 17;
# zero-energy steps as a walk's first, middle and last; generic steps (a publish, a window close) with steady ones behind
# them in the same walk; set_policy_stream (every later step generic) and back; InitStream and an import between launches
CASES = dict(NEW_CASES, uneven=rc.uneven_calls, zero=rc.zero_energy, generic=rc.generic_inside_walk,
             policy=gc.policy_inside, between=cc.between_launches)

HIST_FIELDS = ("histLrt", "histSpecFlat", "histSpecDiff")
# (feature index in featureData, bin width) of the three histograms, in HIST_FIELDS order; 1000 bins each
HIST_FEATURES = ((3, 0.1), (0, 0.05), (4, 0.1))


def hist_sums(state):
    return [int(np.array(getattr(state, f)[:]).sum()) for f in HIST_FIELDS]
