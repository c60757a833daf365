"""The schedule the ragged BT list-call test runs (tests/bt_list_cases.py) has the shapes the kernels can go wrong at: a
tick with one entry, an explicit count-0 entry beside live ones, list lengths around the 256-sample kernel's groups of
four, a group whose four counts all differ, the same streams in another order from tick to tick, descending and
non-adjacent stream numbers inside one group.  Needs no GPU."""
import numpy as np

from tests.bt_list_cases import IDLE, MAX_BLOCKS, S, TOTAL, schedule


def _groups(st, ct):
    """the groups of four consecutive entries a 256-sample list launch forms (the last one may be short)"""
    return [(st[i:i + 4], ct[i:i + 4]) for i in range(0, len(st), 4)]


def test_schedule_has_the_shapes_the_kernels_can_go_wrong_at():
    ticks = schedule()
    got = np.zeros(S, int)
    for st, ct in ticks:
        assert len(st) == len(ct) >= 1
        assert len(set(st.tolist())) == len(st) and IDLE not in st and ct.min() >= 0 and ct.max() <= MAX_BLOCKS
        got[st] += ct
    assert all(got[s] == (0 if s == IDLE else TOTAL) for s in range(S)), got
    assert any(len(st) == 1 for st, _ in ticks)
    assert any((ct == 0).any() and (ct > 0).any() for _, ct in ticks)
    lengths = {len(st) for st, _ in ticks}
    assert {1, 3, 4, 5, 7} <= lengths, lengths  # no multiple of four, exactly four, more than one group
    full = [(g, c) for st, ct in ticks for g, c in _groups(st, ct) if len(g) == 4]
    assert any(sorted(c.tolist()) == [0, 1, 2, 3] for _, c in full)  # four different counts in one workgroup
    assert any(len(a[0]) == len(b[0]) and sorted(a[0]) == sorted(b[0]) and (a[0] != b[0]).any()
               for a, b in zip(ticks, ticks[1:]))  # the same streams in another order, tick to tick
    assert any((np.diff(g) < 0).all() and (np.abs(np.diff(g)) > 1).all() for g, _ in full)  # descending, non-adjacent


def test_schedule_is_fixed():
    a, b = schedule(), schedule()
    assert len(a) == len(b) and all((x[0] == y[0]).all() and (x[1] == y[1]).all() for x, y in zip(a, b))
