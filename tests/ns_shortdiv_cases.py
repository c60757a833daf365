"""Inputs for tests/test_ns_shortdiv_oracle.py (CPU) and tests/test_ns_shortdiv_gpu.py: the frame step of ns_kernels1.hip
forms three kinds of quotient through shorter chains than the generic division -- the trackers' FACTOR / max(density, 1),
gainPrior = (1 - priorSpeechProb) / (priorSpeechProb + 0.0001) and the sums divided by the bin count two at a time --
reduces the logarithm's argument in one instruction and finds the square root's tiny arguments with one compare per
argument for the wave.  What can go wrong is a quotient that is a last bit off in some part of its domain (a density
below, at or above 1; a prior probability at either clamp), a packed pair whose halves are swapped or share a divisor
they should not, and a wave that misses a tiny squared magnitude on one lane.  No tests in here.

A case is what tests/ns_scalar_row_cases.py calls one; `play` is that module's."""
import numpy as np

from tests import ns_cases
from tests import ns_scalar_row_cases as rc

S = rc.S
BASE_FRAMES = rc.BASE_FRAMES
play = rc.play
BINS = 129

CALLS = (1, 2, 7, 13, 17)             # 40 frames: calls start at frames 0, 1, 3, 10 and 23
FRAMES = sum(CALLS)
DENSITY_STREAMS = (0, 4)              # 4: alone in its workgroup
PRIOR = {1: 1.5, 2: -0.5, 4: 0.01}    # imported priorSpeechProb: above the upper clamp, below the lower one, on it
ZERO_STREAM, ZERO_FRAMES, ZERO_STEP = 3, (13, 14), 14   # digital silence; the second frame is the zero-energy step:
#                                       the fifth step of the fourth call (a walk of 8 or of 3 starts at its frame 10)
TINY_STREAM, TINY_FRAMES, TINY_AMPLITUDE = 3, (27, 28, 29), 2.0 ** -60   # inside the fifth call


def density_rows():
    """[3][129] densities on both sides of 1: bin i of tracker s below 1 where (i + s) is even, above 1 otherwise, with
    1 itself, its two neighbours among the floats and a few extremes in fixed bins; bin 128 (the trackers' tails, which
    the kernel steps on three lanes of one instruction) below, above and at 1"""
    rng = np.random.default_rng(16)
    d = np.empty((3, BINS), np.float32)
    for s in range(3):
        below = rng.uniform(0.02, 0.999, BINS).astype(np.float32)
        above = np.exp2(rng.uniform(0.001, 9.0, BINS)).astype(np.float32)
        d[s] = np.where((np.arange(BINS) + s) % 2 == 0, below, above)
        one = np.float32(1.0)
        d[s, 10:17] = [one, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), 1e-6, 3.0, 129.0, 5e4]
    d[0, 128], d[1, 128], d[2, 128] = 0.37, 23.75, 1.0
    return d


def _states(base):
    states = [ns_cases.copy_state(b) for b in base]
    rows = density_rows().reshape(-1)
    for s in DENSITY_STREAMS:
        states[s].density[:] = rows.tolist()
    for s, p in PRIOR.items():
        states[s].priorSpeechProb = p
    return states


def _mixed_frames(n_streams):
    x = rc._frames(n_streams, FRAMES, BASE_FRAMES)
    for f in ZERO_FRAMES:
        x[f, ZERO_STREAM] = 0.0
    return x


def _ops(x):
    ops, f0 = [], 0
    for n in CALLS:
        ops.append(("run", x[f0:f0 + n]))
        f0 += n
    return ops


def mixed(base):
    """40 integer-valued frames in calls of 1, 2, 7, 13 and 17: streams 0 and 4 enter with density_rows(), streams 1, 2
    and 4 with the prior probabilities of PRIOR, stream 3 meets a zero-energy step in the middle of a walk"""
    return _states(base), _ops(_mixed_frames(len(base)))


def tiny(base):
    """the same, with white noise of amplitude 2^-60 in three consecutive frames of stream 3: the analysis window is
    filled with it from the second of them on, and the squared magnitudes fall under 2^-100 (float frames only)"""
    x = _mixed_frames(len(base))
    for f in TINY_FRAMES:
        x[f, TINY_STREAM] = (x[f, TINY_STREAM] / np.float32(32768.0)) * np.float32(TINY_AMPLITUDE)
    return _states(base), _ops(x)


CASES = {"mixed": mixed, "tiny": tiny}
FLOAT_ONLY = ("tiny",)
