"""Inputs for tests/test_ns_guards_oracle.py (CPU) and tests/test_ns_guards_gpu.py: the cases that the frame step of
ns_kernels1.hip guards on every value and meets in no ordinary frame, now each behind one wave-level test -- an emitted
sample outside the int16 range (sat16p), a squared magnitude of exactly zero or +inf under the square root
(fsqrt_n_wave), and a published quantile behind the carried reciprocal of quant + 0.0001f.  What can go wrong is a wave
that takes the fast path although one of its lanes needed the slow one, a slow path that changes a lane that did not,
and a reciprocal that outlives the quantile it was formed from.  No tests in here.

A case is what tests/ns_carry_cases.py calls one (states to import, then "run" / "policy" / "init" / "import"
operations); `play` is that module's.  Frames of the cases in FLOAT_ONLY cannot be stated as int16."""
import numpy as np

from tests import ns_cases
from tests import ns_carry_cases as cc
from tests import ns_scalar_row_cases as rc

S = rc.S
BASE_FRAMES = rc.BASE_FRAMES
play = cc.play

SAT_FRAMES = 12
SAT_FROM = 2            # stream 0 saturates on every sample from this frame of the call on (the DC has filled the window)
SPIKE_AT = (5, 37)      # stream 1: the frame and the sample of its one spike
SPIKE = 150000.0


def saturate(base):
    """Float frames past the int16 range.  Stream 0: a DC level of 5e6 under its signal -- the filter keeps at least
    denoiseBound of it, every emitted sample is far above 32767.  Stream 1: its ordinary signal (a quiet stationary
    noise) with ONE sample of 150000: the emitted samples leave the range around the spike only.  Stream 2: its signal
    with a DC level of -2e6 in frames 3..6: negative excursions only.  Streams 3 and 4: ordinary neighbours."""
    x = rc._frames(len(base), SAT_FRAMES, BASE_FRAMES)
    x[:, 0] += np.float32(5e6)
    x[SPIKE_AT[0], 1, SPIKE_AT[1]] = np.float32(SPIKE)
    x[3:7, 2] = np.float32(-2e6)
    return [ns_cases.copy_state(b) for b in base], [("run", x[:5]), ("run", x[5:])]


def clip16(base):
    """int16 frames whose output leaves the int16 range: every stream plays the full-scale square wave of ns_cases
    (clipped to int16 on both signs) at another phase of its on / off blocks; the filter's ringing overshoots"""
    n = 10
    sq = ns_cases.family_frames(100 + n + len(base))[100:, ns_cases.FAMILY_G]
    x = np.stack([sq[s:s + n] for s in range(len(base))], axis=1)
    x = np.ascontiguousarray(np.clip(np.rint(x), -32768, 32767).astype(np.float32))
    return [ns_cases.copy_state(b) for b in base], [("run", x)]


TINY_FRAMES = 36        # amplitudes 2^-40 .. 2^-75, one step per frame


def tiny(base):
    """White noise in [-1, 1) times 2^-(40 + f + s) in frame f of stream s, held at 2^-75: the squared magnitudes run
    through normal floats, subnormals and exact zeros (the square root's tiny-argument branch, then its pass-through of
    zero), and the frame energy reaches exactly zero in the later streams first"""
    n = rc._frames(len(base), TINY_FRAMES, BASE_FRAMES) / np.float32(32768.0)
    e = np.minimum(40 + np.arange(TINY_FRAMES)[:, None] + np.arange(len(base))[None, :], 75)
    x = np.ascontiguousarray((n * np.exp2(-e.astype(np.float64))[:, :, None]).astype(np.float32))
    return [ns_cases.copy_state(b) for b in base], [("run", x[:20]), ("run", x[20:])]


POISON_STREAM, POISON_FRAME, POISON_SAMPLE = 2, 3, 77


def _poisoned(base, value):
    x = rc._frames(len(base), 10, BASE_FRAMES)
    x[POISON_FRAME, POISON_STREAM, POISON_SAMPLE] = value
    return [ns_cases.copy_state(b) for b in base], [("run", x)]


def nan_frame(base):
    """one NaN sample in frame 3 of stream 2: everything that stream computes from then on is a NaN"""
    return _poisoned(base, np.float32(np.nan))


def inf_frame(base):
    """one +inf sample in frame 3 of stream 2 (inf times the window's zero end is a NaN, the square root meets +inf
    or a NaN)"""
    return _poisoned(base, np.float32(np.inf))


PUBLISH_FRAMES = 16
# stream -> {tracker: counter on entry}; a tracker that enters with counter c publishes in step 200 - c of the call
PUBLISH_COUNTERS = {0: {0: 200},             # step 0: the first step of every walk length
                    1: {1: 196},             # step 4: a middle step of a walk of 8 and of 3
                    2: {2: 193, 0: 192},     # steps 7 and 8: the last step of a walk of 8, then the first of the next
                    #                          (and the last of a walk of 3): two publishes in consecutive steps
                    3: {0: 198, 1: 199, 2: 200},   # steps 2, 1, 0: three in a row
                    4: {1: 189, 2: 188}}     # steps 11 and 12 (alone in its workgroup)


def publish_steps(stream):
    return sorted(200 - c for c in PUBLISH_COUNTERS[stream].values())


def publish(base):
    """a tracker publishes its quantile inside a walk: see PUBLISH_COUNTERS; the steps around a publish are generic,
    the others steady, so every publish has a steady step (which formed and kept a reciprocal) in front of it in the
    same walk of 8 -- except the ones in step 0 -- and steady steps behind it"""
    states = [ns_cases.copy_state(b) for b in base]
    for s, cs in PUBLISH_COUNTERS.items():
        for k, c in cs.items():
            states[s].counter[k] = c
    return states, [("run", rc._frames(len(base), PUBLISH_FRAMES, BASE_FRAMES))]


def policy_inside(base):
    """set_policy_stream of streams 1 and 4 (mode 0: gainmap off, every later step of theirs generic) between two calls
    and back to mode 2 between the next two: generic steps between steady ones, across launches"""
    x = rc._frames(len(base), 27, BASE_FRAMES)
    ops = [("run", x[:9]), ("policy", 1, 0), ("policy", 4, 0), ("run", x[9:18]), ("policy", 1, 2), ("policy", 4, 2),
           ("run", x[18:])]
    return [ns_cases.copy_state(b) for b in base], ops


# new here
NEW_CASES = {"saturate": saturate, "clip16": clip16, "tiny": tiny, "nan": nan_frame, "inf": inf_frame,
             "publish": publish, "policy": policy_inside}
# with the cases of the two earlier modules that the issue names again: calls of 1, 2, 7, 13, 17; a window close between
# steady steps; set_policy_stream, InitStream and an import between two launches
CASES = dict(NEW_CASES, uneven=rc.uneven_calls, generic=rc.generic_inside_walk, between=cc.between_launches)
FLOAT_ONLY = ("saturate", "tiny", "nan", "inf")
POISONED = {"nan": POISON_STREAM, "inf": POISON_STREAM}
