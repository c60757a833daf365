"""The schedule the ragged AEC list-call tests run (tests/aec_list_cases.py) has the shapes the kernel can go wrong at:
a tick with one entry, an explicit count-0 entry beside live ones, list lengths that are no multiple of a workgroup's
four waves, more than one workgroup, the same streams in another order from tick to tick, every stream but the idle one
at the same total.  On a control-only handle it also shows that the total reaches past every stream's start-up phase
and that a single call crosses the end of one.  Needs the built library, no GPU."""
import numpy as np
import pytest

from tests.aec_list_cases import CONFIGS, DELAYS, IDLE, TOTAL, S, control_fields, control_lib, control_only, \
    run_list_control, schedule

STARTUP = 0  # AspAecControl's first field


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
    assert len(DELAYS) == S


@pytest.mark.parametrize("fs,n,ext", CONFIGS)
def test_every_listed_stream_leaves_start_up_and_one_call_crosses_its_end(built_lib, fs, n, ext):
    """Every listed stream has left the start-up phase by its own frame 60: the buffer-size check ends after at most
    50 frames (echo_cancellation.c:696-703), and the far buffer then holds more than the at most kMaxBufSizeStart = 62
    partitions start-up waits for, or reaches them within ten frames more (10 ms frames: 1.25 / 2.5 partitions each).
    And at least one entry with two or more frames starts a call in start-up and ends it past it: the kernel meets a
    pass-through frame and a processed one of the same stream in one launch."""
    lib = control_lib()
    h = control_only(lib, fs, ext)
    done = np.zeros(S, int)
    left_at = {}
    crossed = 0
    for st, ct in schedule():
        before = {int(s): control_fields(lib, h, int(s))[STARTUP] for s in st}
        assert run_list_control(lib, h, st, ct, n, [DELAYS[s] for s in st]) == 0
        for s, c in zip(st.tolist(), ct.tolist()):
            done[s] += c
            after = control_fields(lib, h, s)[STARTUP]
            if before[s] == 1 and after == 0:
                left_at[s] = done[s]
                crossed += c >= 2
    assert lib.AspAecBatch_Free(h) == 0
    assert sorted(left_at) == [s for s in range(S) if s != IDLE], left_at
    assert max(left_at.values()) <= 60, left_at
    assert crossed >= 1
