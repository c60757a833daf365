"""The ragged schedule of tests/test_ns_list_gpu.py (list calls of the NS batch): which streams a tick lists, in which
order, and with how many frames each.  Kept apart from the GPU test so that the CPU suite checks its shape
(tests/test_ns_list_schedule.py)."""
import numpy as np

S = 9
TOTAL, IDLE = 520, 7  # every stream but IDLE ends at 520 frames (the histogram window closes at 500); IDLE is never listed


def schedule():
    """[(streams, counts)] per tick, fixed seed: each listed stream gets 0..3 frames, the order changes from tick to tick."""
    rng = np.random.RandomState(20240611)
    left = {s: TOTAL for s in range(S) if s != IDLE}
    ticks = [(np.array([5], np.int32), np.array([1], np.int32))]  # a tick with n == 1
    left[5] -= 1
    while any(left.values()):
        streams, counts = [], []
        for s in rng.permutation([s for s in left if left[s]]):
            c = min(int(rng.choice([0, 1, 1, 1, 2, 3])), left[s])
            if c == 0 and rng.rand() < 0.5:
                continue  # no frame: sometimes not listed, sometimes listed with count 0
            streams.append(s)
            counts.append(c)
            left[s] -= c
        if streams:
            ticks.append((np.array(streams, np.int32), np.array(counts, np.int32)))
    return ticks
