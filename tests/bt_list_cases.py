"""The ragged schedule of tests/test_bt_list_gpu.py (list calls of the BT batch): which stream-channels a tick lists, in
which order, and with how many macroblocks each.  Kept apart from the GPU test so that the CPU suite checks its shape
(tests/test_bt_list_schedule.py)."""
import numpy as np

S = 9
TOTAL, IDLE = 6, 7  # every stream but IDLE ends at 6 macroblocks; IDLE is never listed
MAX_BLOCKS = 3      # counts are 0 .. 3 per tick
SILENT, WIDE = 3, 6  # digital silence (the reference's 0 / 0 path); wide-segment noise (0.5 * standard_normal)

# The first ticks are written out: the shapes the 256-sample kernel's groups of four can go wrong at.
HEAD = [
    ([5], [1]),                                          # n == 1
    ([8, 6, 3, 1], [2, 0, 3, 1]),                        # one group: four different counts, descending, non-adjacent
    ([1, 8, 3, 6], [1, 1, 0, 2]),                        # the same streams in another order
    ([0, 2, 4, 5, 6, 8, 1], [3, 1, 2, 0, 1, 0, 1]),      # two groups, the second one short of an entry
    ([4, 0, 2, 5, 3], [1, 0, 2, 3, 1]),                  # a group and one entry more
    ([2, 0, 4], [1, 2, 0]),                              # less than a group
]


def schedule():
    """[(streams, counts)] per tick: HEAD, then (fixed seed) each listed stream gets 0 .. 3 macroblocks and the order
    changes from tick to tick, until every stream but IDLE has had TOTAL."""
    rng = np.random.RandomState(20240917)
    left = {s: TOTAL for s in range(S) if s != IDLE}
    ticks = []
    for st, ct in HEAD:
        ticks.append((np.array(st, np.int32), np.array(ct, np.int32)))
        for s, c in zip(st, ct):
            left[s] -= c
    assert min(left.values()) >= 0
    while any(left.values()):
        streams, counts = [], []
        for s in rng.permutation([s for s in left if left[s]]):
            c = min(int(rng.choice([0, 1, 1, 2, 3])), left[s])
            if c == 0 and rng.rand() < 0.5:
                continue  # no macroblock: sometimes not listed, sometimes listed with count 0
            streams.append(s)
            counts.append(c)
            left[s] -= c
        if streams:
            ticks.append((np.array(streams, np.int32), np.array(counts, np.int32)))
    return ticks
