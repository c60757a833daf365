"""The fixed-point noise suppressor's edge runs (tests/nsx_runs.EDGE_RUNS, tests/golden/nsx_edges_golden.npz) on the GPU,
through the batch API with ProcessFrames cut at the snapshot frames.  Seven streams, one wave each: stream s carries
run s mod K of the K edge runs of one rate (a batch call fixes the frame length and the band count), each with its own
policy; a stream whose run has ended gets zero frames.  Every stream must equal its golden in outputs and in the
exported state at its snapshot frames.  The seeded cases go through ImportState on stream 1 of 3 beside two streams
on a golden run."""
import os

import numpy as np
import pytest

from audiosignalprocess_amd.nsx import AspNsxState, NsxBatch, state_dict
from tests import nsx_runs
from tests.edge_pack import unpack_state
from tests.nsx_runs import EDGE_RUNS, RUNS, SEEDED, inputs, schedule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "nsx_golden.npz"))
EDGES = np.load(os.path.join(ROOT, "tests", "golden", "nsx_edges_golden.npz"))
S = 7


def state_diff(st, packed):
    want = state_dict(unpack_state(AspNsxState, packed))
    return [n for n, v in state_dict(st).items() if not np.array_equal(v, want[n])]


@pytest.mark.parametrize("fs", [8000, 16000])
def test_edge_runs_side_by_side_equal_their_goldens(fs):
    group = [i for i, sp in enumerate(EDGE_RUNS) if sp["fs"] == fs]
    assert len(group) >= 2 and len({i for i, sp in enumerate(EDGE_RUNS) if sp["fs"] not in (8000, 16000)}) == 0
    runs = [group[s % len(group)] for s in range(S)]
    specs = [EDGE_RUNS[i] for i in runs]
    for sp in specs:   # what this test's one Init and set_policy per stream relies on
        assert all(ev["init"] is None and ev["mode"] is None for ev in schedule(sp)[1:])
    n = 80 if fs == 8000 else 160
    xs = {i: inputs(EDGE_RUNS[i]) for i in group}
    b = NsxBatch(S)
    assert b.init(fs) == 0
    for s, sp in enumerate(specs):
        assert b.set_policy(sp["mode"], s) == 0
    F = max(sp["frames"] for sp in specs)
    cuts = sorted({0, F} | {f + 1 for sp in specs for f in sp["snaps"]})
    out = np.zeros((F, S, n), np.int16)
    bad = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        x = np.zeros((e - a, 1, S, n), np.int16)
        for s, (i, sp) in enumerate(zip(runs, specs)):
            for f in range(a, min(e, sp["frames"])):
                x[f - a, 0, s] = xs[i][f][0]
        out[a:e] = b.process_frames(x)[:, 0]
        for s, (i, sp) in enumerate(zip(runs, specs)):
            if e - 1 in sp["snaps"]:
                bad += [(s, i, e - 1, nm) for nm in state_diff(b.export_state(s), EDGES["e%d_s%d" % (i, e - 1)])]
    b.close()
    assert not bad, "state fields differ at (stream, run, frame, field): %r" % bad[:8]
    for s, (i, sp) in enumerate(zip(runs, specs)):
        msg = nsx_runs.compare_outputs(sp, out[:sp["frames"], s], EDGES["e%d_keep" % i], EDGES["e%d_blocks" % i])
        assert msg is None, "stream %d, edge run %d: %s" % (s, i, msg)


@pytest.mark.parametrize("k", range(len(SEEDED)))
def test_seeded_case_through_import_state(k):
    case = SEEDED[k]
    base, side = RUNS[case["base"]], RUNS[5]   # both 16 kHz, one band
    assert base["fs"] == side["fs"] == 16000
    F = case["frames"]
    b = NsxBatch(3)
    assert b.init(16000) == 0 and b.set_policy(side["mode"]) == 0
    assert b.import_state(1, unpack_state(AspNsxState, EDGES["sd%d_in" % k])) == 0
    x = np.zeros((F, 1, 3, 160), np.int16)
    seeded, plain = nsx_runs.seeded_inputs(case), inputs(side)
    for f in range(F):
        x[f, 0, 0] = x[f, 0, 2] = plain[f][0]
        x[f, 0, 1] = seeded[f][0]
    y = b.process_frames(x)
    bad = state_diff(b.export_state(1), EDGES["sd%d_s" % k])
    b.close()
    assert np.array_equal(y[:, 0, 1].reshape(-1), EDGES["sd%d_out" % k])
    assert not bad, "state fields differ after the seeded frames: %r" % bad
    for s in (0, 2):
        assert np.array_equal(y[:, 0, s].reshape(-1), GOLDEN["r5_out"][:160 * F])
