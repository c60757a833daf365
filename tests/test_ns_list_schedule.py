"""The schedule the ragged list-call test runs (tests/ns_list_cases.py) has the shapes the kernel can go wrong at: a
tick with one entry, an explicit count-0 entry beside live ones, list lengths that are no multiple of a workgroup's
four waves, more than one workgroup, the same streams in another order from tick to tick, every stream but the idle one
at the same total beyond the 500-frame histogram window.  Needs no GPU."""
import numpy as np

from tests.ns_list_cases import IDLE, TOTAL, S, schedule


def test_schedule_has_the_shapes_the_kernel_can_go_wrong_at():
    ticks = schedule()
    got = np.zeros(S, int)
    for st, ct in ticks:
        assert len(set(st.tolist())) == len(st) and IDLE not in st and ct.min() >= 0 and ct.max() <= 3
        got[st] += ct
    assert all(got[s] == (0 if s == IDLE else TOTAL) for s in range(S)), got
    assert any(len(st) == 1 for st, _ in ticks)
    assert any((ct == 0).any() and (ct > 0).any() for _, ct in ticks)
    assert any(len(st) % 4 for st, _ in ticks) and any(len(st) > 4 for st, _ in ticks)
    assert any(len(a[0]) == len(b[0]) and sorted(a[0]) == sorted(b[0]) and (a[0] != b[0]).any()
               for a, b in zip(ticks, ticks[1:]))  # the same streams in another order, tick to tick
