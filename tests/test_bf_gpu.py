"""GPU suite of the batched beamformer (include/asp_bf.h), through the C ABI: the kernel against the golden of the
reference compiled in place, bit for bit.  The batches load the golden's Initialize tables with
AspBfBatch_SetTables, so the kernel's pin does not depend on this machine's libm; one test runs the library's own
tables."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from audiosignalprocess_amd import bf
from audiosignalprocess_amd.build import LIBDIR
from audiosignalprocess_amd.ns import DeviceBuffer
from tests.bf_runs import ARRAYS, CHUNKS, RUNS, geometry, inputs, state_scalars
from tests.conftest import check_free_running, parity_note, rel_l2_per_stream
from tests.test_bf_host import same, table_key

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = (0, 1, 2, 3, 4)   # the runs that share one geometry


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "bf_golden.npz")))


@pytest.fixture(scope="module")
def gold_tables():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "bf_tables_golden.npz")))


def make_batch(S, spec, gold_tables):
    """A batch with the run's geometry and, unless gold_tables is None, the golden's tables."""
    b = bf.BfBatch(S)
    assert b.initialize(geometry(spec)) == 0
    if gold_tables is not None:
        for which, name in enumerate(bf.TABLES):
            assert b.set_table(which, gold_tables[table_key(spec) + "_" + name]) == 0
    return b


def stacked(runs):
    """(input [F][S][M][160], high [F][S][M][160] or None) with stream s replaying runs[s]."""
    xs, his = zip(*(inputs(RUNS[r]) for r in runs))
    return (np.ascontiguousarray(np.stack(xs, axis=1)),
            None if his[0] is None else np.ascontiguousarray(np.stack(his, axis=1)))


def check_outputs(gold, runs, y, hy, tp, f0=0):
    for s, r in enumerate(runs):
        sl = slice(f0, f0 + y.shape[0])
        bad = np.nonzero((y[:, s].view(np.uint32) != gold["r%d_out" % r][sl].view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, "stream %d (run %d): outputs differ first at chunk %d" % (s, r, f0 + bad[0])
        if hy is not None:
            assert same(hy[:, s], gold["r%d_high_out" % r][sl]), "stream %d: high band" % s
        assert np.array_equal(tp[:, s], gold["r%d_target_present" % r][sl]), "stream %d: is_target_present" % s


def check_state(gold, b, s, r, f):
    st, buf = b.get_state(s)
    assert np.array_equal(state_scalars(st), gold["r%d_scalars" % r][f]), "scalars of run %d after chunk %d" % (r, f)
    if f in RUNS[r]["snaps"]:
        snap = bf.state_dict(st, buf)
        for k in ARRAYS:
            assert same(snap[k], gold["r%d_s%d_%s" % (r, f, k)]), "state %s of run %d at chunk %d" % (k, r, f)
    return st, buf


@pytest.fixture(scope="module")
def five_by_one(gold, gold_tables):
    """Five streams, each a different golden run, one chunk per call; checked as it goes."""
    x, hi = stacked(FIVE)
    b = make_batch(5, RUNS[0], gold_tables)
    ys, hys, tps = [], [], []
    for f in range(CHUNKS):
        rc, y, hy, tp = b.process_chunks(x[f:f + 1], hi[f:f + 1], single=True)
        assert rc == 0
        ys.append(y)
        hys.append(hy)
        tps.append(tp)
        for s, r in enumerate(FIVE):
            if f in RUNS[r]["snaps"]:
                check_state(gold, b, s, r, f)
    final = [b.get_state(s) for s in range(5)]
    b.close()
    return np.concatenate(ys), np.concatenate(hys), np.concatenate(tps), final


def test_five_runs_in_one_batch_one_chunk_per_call(gold, five_by_one):
    y, hy, tp, final = five_by_one
    check_outputs(gold, FIVE, y, hy, tp)
    for s, r in enumerate(FIVE):
        assert np.array_equal(state_scalars(final[s][0]), gold["r%d_scalars" % r][CHUNKS - 1])


def test_seven_chunks_per_call_equal_one_chunk_per_call(gold, gold_tables, five_by_one):
    """F = 7 is no multiple of the Blocker's 4-chunk cycle: outputs and the final state equal the F = 1 run's."""
    x, hi = stacked(FIVE)
    b = make_batch(5, RUNS[0], gold_tables)
    ys, hys, tps = [], [], []
    for f0 in range(0, CHUNKS, 7):
        rc, y, hy, tp = b.process_chunks(x[f0:f0 + 7], hi[f0:f0 + 7])
        assert rc == 0
        ys.append(y)
        hys.append(hy)
        tps.append(tp)
    y, hy, tp = np.concatenate(ys), np.concatenate(hys), np.concatenate(tps)
    y1, hy1, tp1, final1 = five_by_one
    assert same(y, y1) and same(hy, hy1) and np.array_equal(tp, tp1)
    check_outputs(gold, FIVE, y, hy, tp)
    for s in range(5):
        st, buf = b.get_state(s)
        assert bytes(st) == bytes(final1[s][0]) and same(buf, final1[s][1])
    b.close()


@pytest.mark.parametrize("r", (5, 6, 7))
def test_two_three_and_eight_microphones(gold, gold_tables, r):
    """M = 2 (no high band), 3 (high band) and 8 (no high band): two streams replay the run, one launch up to each
    snapshot chunk."""
    spec = RUNS[r]
    x, hi = stacked((r, r))
    b = make_batch(2, spec, gold_tables)
    f0 = 0
    for f1 in sorted(set(f + 1 for f in spec["snaps"]) | {CHUNKS}):
        rc, y, hy, tp = b.process_chunks(x[f0:f1], None if hi is None else hi[f0:f1])
        assert rc == 0 and (hy is None) == (not spec["high"])
        check_outputs(gold, (r, r), y, hy, tp, f0)
        check_state(gold, b, 1, r, f1 - 1)
        f0 = f1
    b.close()


def test_initialize_stream_in_mid_run(gold, gold_tables):
    """InitializeStream of stream 1 after 30 chunks: the others go on untouched; stream 1, fed the run from its
    start again, gives the run's first 50 chunks."""
    x, hi = stacked((0, 0, 0))
    x[30:, 1], hi[30:, 1] = x[:50, 0].copy(), hi[:50, 0].copy()
    b = make_batch(3, RUNS[0], gold_tables)
    rc, y0, hy0, tp0 = b.process_chunks(x[:30], hi[:30])
    assert rc == 0 and b.initialize(None, stream=1) == 0
    assert b.lib.AspBfBatch_InitializeStream(b.h, 3) < 0
    rc, y1, hy1, tp1 = b.process_chunks(x[30:], hi[30:])
    assert rc == 0
    y, hy, tp = np.concatenate([y0, y1]), np.concatenate([hy0, hy1]), np.concatenate([tp0, tp1])
    check_outputs(gold, (0,), y[:, 0:1], hy[:, 0:1], tp[:, 0:1])
    check_outputs(gold, (0,), y[:, 2:3], hy[:, 2:3], tp[:, 2:3])
    check_outputs(gold, (0,), y[:30, 1:2], hy[:30, 1:2], tp[:30, 1:2])
    check_outputs(gold, (0,), y[30:, 1:2], hy[30:, 1:2], tp[30:, 1:2])   # chunks 0..49 of the run
    check_state(gold, b, 2, 0, CHUNKS - 1)
    b.close()


def test_state_round_trip_into_a_fresh_batch(gold, gold_tables):
    x, hi = stacked((3,))
    a = make_batch(1, RUNS[3], gold_tables)
    rc, y0, hy0, tp0 = a.process_chunks(x[:41], hi[:41])
    assert rc == 0
    st, buf = a.get_state(0)
    a.close()
    b = make_batch(2, RUNS[3], gold_tables)
    assert b.set_state(1, st, buf) == 0
    x2, hi2 = np.repeat(x[41:], 2, axis=1), np.repeat(hi[41:], 2, axis=1)
    rc, y1, hy1, tp1 = b.process_chunks(x2, hi2)
    assert rc == 0
    check_outputs(gold, (3,), np.concatenate([y0, y1[:, 1:2]]), np.concatenate([hy0, hy1[:, 1:2]]),
                  np.concatenate([tp0, tp1[:, 1:2]]))
    check_state(gold, b, 1, 3, CHUNKS - 1)
    # a state this batch cannot reach is refused: the kernel indexes its buffers with these
    for field, value in (("frame_offset", 100), ("frame_offset", 128), ("current_block_ix", 2), ("previous_block_ix", -2),
                         ("num_mics", 5)):
        bad = bf.AspBfState.from_buffer_copy(bytes(st))
        setattr(bad, field, value)
        assert b.set_state(0, bad, buf) < 0, field
    b.close()


def device_run(b, x, hi):
    """One ProcessChunks call on device buffers, not synchronised: returns the buffers to download later."""
    F, S = x.shape[:2]
    bufs = dict(x=DeviceBuffer(x.nbytes), y=DeviceBuffer(F * S * 160 * 4), tp=DeviceBuffer(F * S))
    bufs["x"].upload(x)
    if hi is not None:
        bufs["hi"], bufs["hy"] = DeviceBuffer(hi.nbytes), DeviceBuffer(F * S * 160 * 4)
        bufs["hi"].upload(hi)
    rc = b.lib.AspBfBatch_ProcessChunks(b.h, F, bufs["x"].ptr, bufs["hi"].ptr if hi is not None else None, bufs["y"].ptr,
                                        bufs["hy"].ptr if hi is not None else None, bufs["tp"].ptr, bf.MEM_DEVICE)
    assert rc == 0
    return bufs


def device_results(b, bufs, F, S):
    assert b.synchronize() == 0
    y = bufs["y"].download((F, S, 160))
    hy = bufs["hy"].download((F, S, 160)) if "hy" in bufs else None
    tp = bufs["tp"].download((F, S), np.uint8)
    for d in bufs.values():
        d.free()
    return y, hy, tp


def test_device_buffers_give_what_host_buffers_give(gold, gold_tables, five_by_one):
    x, hi = stacked(FIVE)
    b = make_batch(5, RUNS[0], gold_tables)
    y, hy, tp = device_results(b, device_run(b, x, hi), CHUNKS, 5)
    b.close()
    assert same(y, five_by_one[0]) and same(hy, five_by_one[1]) and np.array_equal(tp, five_by_one[2])
    check_outputs(gold, FIVE, y, hy, tp)


def test_4100_streams_cover_the_grid_tail(gold, gold_tables):
    """4100 streams (no multiple of 64, 256 or 1024) tiled from the five runs, 8 chunks in one launch."""
    S, F = 4100, 8
    x5, hi5 = stacked(FIVE)
    reps = S // 5
    x, hi = np.tile(x5[:F], (1, reps, 1, 1)), np.tile(hi5[:F], (1, reps, 1, 1))
    b = make_batch(S, RUNS[0], gold_tables)
    rc, y, hy, tp = b.process_chunks(x, hi)
    assert rc == 0
    want = np.stack([gold["r%d_out" % r][:F] for r in FIVE], axis=1)
    want_hi = np.stack([gold["r%d_high_out" % r][:F] for r in FIVE], axis=1)
    want_tp = np.stack([gold["r%d_target_present" % r][:F] for r in FIVE], axis=1)
    assert same(y, np.tile(want, (1, reps, 1))) and same(hy, np.tile(want_hi, (1, reps, 1)))
    assert np.array_equal(tp, np.tile(want_tp, (1, reps)))
    check_state(gold, b, S - 1, FIVE[(S - 1) % 5], F - 1)
    b.close()


def test_two_batches_at_once_on_two_hip_streams(gold, gold_tables):
    """Each batch launches on its own non-blocking HIP stream: both are in flight before either is waited for."""
    a, b = make_batch(2, RUNS[6], gold_tables), make_batch(3, RUNS[7], gold_tables)
    xa, hia = stacked((6, 6))
    xb, hib = stacked((7, 7, 7))
    ra = device_run(a, xa, hia)
    rb = device_run(b, xb, hib)
    yb, hyb, tpb = device_results(b, rb, CHUNKS, 3)
    ya, hya, tpa = device_results(a, ra, CHUNKS, 2)
    check_outputs(gold, (6, 6), ya, hya, tpa)
    check_outputs(gold, (7, 7, 7), yb, hyb, tpb)
    a.close()
    b.close()


def test_refusals_through_the_abi():
    b = bf.BfBatch(2)
    lib = b.lib
    x = np.zeros((1, 2, 4, 160), np.float32)
    y = np.zeros((1, 2, 160), np.float32)
    assert lib.AspBfBatch_ProcessChunk(b.h, x.ctypes.data, None, y.ctypes.data, None, None, bf.MEM_HOST) == -4
    for rate in (8000, 32000, 48000):
        assert b.initialize(bf.linear_geometry(4, 0.04), 10, rate) == -1
        assert "16000" in lib.AspNs_last_error().decode()
    assert b.initialize(bf.linear_geometry(4, 0.04), 20, 16000) == -1
    assert b.initialize(bf.linear_geometry(9, 0.04)) == -1 and "2 to 8" in lib.AspNs_last_error().decode()
    g = bf.linear_geometry(4, 0.04)
    g[3, 0] += 0.01
    assert b.initialize(g) == -1 and "uniform linear array" in lib.AspNs_last_error().decode()
    assert lib.AspBfBatch_state_floats(b.h) == -1
    assert b.initialize(bf.linear_geometry(4, 0.04)) == 0 and lib.AspBfBatch_state_floats(b.h) == 5 * 384
    assert lib.AspBfBatch_ProcessChunk(b.h, x.ctypes.data, x.ctypes.data, y.ctypes.data, None, None, bf.MEM_HOST) == -1
    assert b.set_table(0, np.zeros(255, np.float32)) == -1 and b.set_table(10, np.zeros(1, np.float32)) == -1
    b.close()


def test_cpp_class_from_a_compiled_client(tmp_path):
    """webrtc::Beamformer (include/webrtc_beamformer.h) driven by tests/bf_client.cpp, in place (output[0] is
    input[0]), against a batch of one with the same (library-made) tables."""
    exe = str(tmp_path / "bf_client")
    subprocess.run(["g++", "-O1", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "bf_client.cpp"), "-L" + LIBDIR, "-lasp_amd", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    spec, F = RUNS[0], 24
    x, hi = inputs(spec)
    x, hi = x[:F], hi[:F]
    x.tofile(tmp_path / "in.f32")
    hi.tofile(tmp_path / "hi.f32")
    r = subprocess.run([exe, str(spec["mics"]), "%.9g" % spec["spacing"], str(F), "1", str(tmp_path / "in.f32"),
                        str(tmp_path / "hi.f32"), str(tmp_path / "out.f32"), str(tmp_path / "hout.f32"),
                        str(tmp_path / "log")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    b = make_batch(1, spec, None)
    rc, y, hy, tp = b.process_chunks(x[:, None], hi[:, None])
    b.close()
    assert rc == 0
    log = (tmp_path / "log").read_text().split("\n")
    assert log[:2] == ["-1", "0"] and log[2 + F] == "-1"
    assert [l.split() for l in log[2:2 + F]] == [["0", str(int(t))] for t in tp[:, 0]]
    assert same(np.fromfile(tmp_path / "out.f32", np.float32).reshape(F, 160), y[:, 0])
    assert same(np.fromfile(tmp_path / "hout.f32", np.float32).reshape(F, 160), hy[:, 0])


def test_the_librarys_own_tables(gold, gold_tables):
    """Initialize's tables as this machine's libm and complex runtime make them.  Equal to the golden's bit for bit:
    the outputs equal the golden bit for bit.  Otherwise the count of differing entries is recorded and the
    outputs are held to the project's bar for a free-running comparison."""
    x, hi = stacked(FIVE)
    b = make_batch(5, RUNS[0], None)
    differing = 0
    for which, name in enumerate(bf.TABLES):
        want = gold_tables[table_key(RUNS[0]) + "_" + name]
        differing += int((b.get_table(which).view(np.uint32) != want.view(np.uint32)).sum())
    rc, y, hy, tp = b.process_chunks(x, hi)
    b.close()
    assert rc == 0
    if differing == 0:
        check_outputs(gold, FIVE, y, hy, tp)
        return
    parity_note("bf: %d entries of the library's own Initialize tables differ from the golden's" % differing)
    want = np.stack([gold["r%d_out" % r] for r in FIVE], axis=1)
    want_hi = np.stack([gold["r%d_high_out" % r] for r in FIVE], axis=1)
    check_free_running(rel_l2_per_stream(y, want), "bf low band, own tables")
    check_free_running(rel_l2_per_stream(hy, want_hi), "bf high band, own tables")
