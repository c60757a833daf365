"""CPU suite: the CPU build of csrc/bf_core.h (lib/libbf_restate.so, the source the kernel runs) equals the golden of
the reference beamformer compiled in place bit for bit -- outputs of both bands, is_target_present, the state
scalars after every chunk and the full state at the snapshot chunks -- and its own Initialize tables equal the
golden's tables bit for bit on this machine; the core's hypotf is the host libm's; the Blocker schedule; and every
refusal."""
import ctypes as C
import ctypes.util
import hashlib
import os

import numpy as np
import pytest

from audiosignalprocess_amd import bf
from audiosignalprocess_amd.synth import bf_chunks
from tests.bf_runs import ARRAYS, CHUNKS, RUNS, geometry, hypot_operands, inputs, replay, state_scalars, table_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(autouse=True, scope="module")
def _built(built_lib):
    return built_lib


@pytest.fixture(scope="module")
def gold(built_lib):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "bf_golden.npz")))


@pytest.fixture(scope="module")
def gold_tables(built_lib):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "bf_tables_golden.npz")))


class Cpu:
    """bf_runs.replay's interface on the CPU build."""

    def __init__(self, tables=None):
        self.r, self.snaps, self.tables = bf.Restate(), {}, tables

    def initialize(self, g):
        rc = self.r.initialize(g)
        if rc == 0 and self.tables is not None:
            for which, t in enumerate(self.tables):
                assert self.r.set_table(which, t) == 0
        return rc

    def process(self, x, hi):
        return self.r.process_chunk(x, hi)

    def scalars(self):
        return state_scalars(self.r.state)

    def snapshot(self, f):
        self.snaps[f] = bf.state_dict(self.r.state, self.r.buffers)


@pytest.mark.parametrize("r", range(len(RUNS)))
def test_cpu_build_equals_the_golden(gold, r):
    spec = RUNS[r]
    x, hi = inputs(spec)
    h = hashlib.sha256(np.ascontiguousarray(x).tobytes())
    if hi is not None:
        h.update(np.ascontiguousarray(hi).tobytes())
    assert h.hexdigest() == str(gold["r%d_inputs_sha256" % r]), "the regenerated input is the golden's"
    cpu = Cpu()
    y, hy, tp, sc = replay(spec, cpu)
    assert same(y, gold["r%d_out" % r])
    assert (hy is None) == (("r%d_high_out" % r) not in gold)
    if hy is not None:
        assert same(hy, gold["r%d_high_out" % r])
    assert np.array_equal(tp, gold["r%d_target_present" % r])
    assert np.array_equal(sc, gold["r%d_scalars" % r])
    assert set(cpu.snaps) == set(spec["snaps"])
    for f, snap in cpu.snaps.items():
        for k in ARRAYS:
            assert same(snap[k], gold["r%d_s%d_%s" % (r, f, k)]), (f, k)


def test_golden_covers_the_scope(gold):
    assert int(gold["num_runs"][0]) == len(RUNS) and int(gold["chunks"][0]) == CHUNKS
    assert {s["mics"] for s in RUNS} >= {2, 3, 4, 8} and {s["high"] for s in RUNS} == {True, False}
    assert len({s["spacing"] for s in RUNS}) >= 2
    assert sum(1 for s in RUNS if (s["mics"], s["spacing"], s["high"]) == (4, 0.04, True)) >= 5
    tp = np.concatenate([gold["r%d_target_present" % r] for r in range(len(RUNS))])
    assert set(tp) == {0, 1}
    offsets = np.concatenate([gold["r%d_scalars" % r][:, 0] for r in range(len(RUNS))])
    assert set(offsets) == {0, 32, 64, 96}


@pytest.mark.parametrize("key", sorted({table_key(s) for s in RUNS}))
def test_initialize_tables_equal_the_golden(gold_tables, key):
    spec = next(s for s in RUNS if table_key(s) == key)
    cpu = bf.Restate()
    assert cpu.initialize(geometry(spec)) == 0
    for which, name in enumerate(bf.TABLES):
        assert same(cpu.get_table(which), gold_tables[key + "_" + name]), name
    assert np.array_equal(cpu.params(), gold_tables[key + "_ints"])   # bins 4, 6, 64, 112 and 31 blocks
    assert list(cpu.params()) == [4, 6, 64, 112, 31]
    assert np.float32(cpu.L.BfRestate_MicSpacing(cpu.h)) == gold_tables[key + "_mic_spacing"][0]


def test_hypotf_is_the_host_libms():
    """bf_core.h's bf_hypotf (fp64, one rounding) against libm's hypotf: 2^20 random pairs over the whole exponent
    range, 2^20 in the audio range, and an edge set (zeros, denormals, equal components, infinities)."""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.hypotf.restype = C.c_float
    libm.hypotf.argtypes = [C.c_float, C.c_float]
    x, y, edges = hypot_operands()
    got = np.zeros(x.size, np.float32)
    bf.Restate.lib().BfRestate_hypotf(x.ctypes.data, y.ctypes.data, got.ctypes.data, x.size)
    assert x.size >= 1000000
    # libm through numpy: np.hypot on float32 calls hypotf; spot-check that against ctypes
    with np.errstate(over="ignore"):
        want = np.hypot(x, y)
    for i in list(range(0, x.size, 50021)) + list(edges):
        assert np.float32(libm.hypotf(float(x[i]), float(y[i]))).view(np.uint32) == want[i].view(np.uint32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad[:5], x[bad[:5]], y[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_blocker_schedule():
    """Initial delay 224, frame_offset_ cycles 0, 96, 64, 32, that is 2, 1, 1, 1 blocks per chunk: seen in the
    state (an off-axis source keeps the mask median below the threshold, so interference_blocks_count_ counts
    every block) and in the output, which stays exactly zero for the 224 samples of delay less the block overlap."""
    M, F = 4, 12
    x, _ = bf_chunks(1, F, M, seed=9, broadside=(), offaxis=((0, F),), silent=())
    cpu = bf.Restate()
    assert cpu.initialize(bf.linear_geometry(M, 0.04)) == 0
    assert cpu.state.frame_offset == 0 and cpu.state.previous_block_ix == -1 and cpu.state.interference_blocks_count == 31
    offsets, counts, outs = [], [], []
    for f in range(F):
        y, _, _ = cpu.process_chunk(x[f, 0])
        offsets.append(cpu.state.frame_offset)
        counts.append(cpu.state.interference_blocks_count)
        outs.append(y)
    assert offsets == [96, 64, 32, 0] * 3
    assert list(np.diff([31] + counts)) == [2, 1, 1, 1] * 3
    assert cpu.state.current_block_ix == 15 % 2 and cpu.state.previous_block_ix == 0
    assert cpu.buffers.size == (M + 1) * 384
    # the newest 160 samples sit behind 224 samples of delay in the input buffer
    assert same(cpu.buffers[:M * 384].reshape(M, 384)[:, 64:224], x[F - 1, 0])
    # a unit pulse on every microphone at sample 0 of a fresh stream: buffer position 224, inside the first block
    # only from its sample 224 on; the second block (128..383) holds it at 96.  The window is power-complementary
    # and the normalised delay-and-sum weights are 1 / sqrt(M) each, so the pulse comes out at sqrt(M) times its height
    p = np.zeros((M, 160), np.float32)
    p[:, 0] = 1000
    cpu = bf.Restate()
    cpu.initialize(bf.linear_geometry(M, 0.04))
    y0, _, _ = cpu.process_chunk(p)
    y1, _, _ = cpu.process_chunk(np.zeros((M, 160), np.float32))
    y = np.concatenate([y0, y1])
    assert np.abs(y).argmax() == 224 and abs(y[224] - 1000 * np.sqrt(M)) < 1.0


@pytest.mark.parametrize("rate", (8000, 32000, 48000, 44100))
def test_other_rates_are_refused(rate):
    cpu = bf.Restate()
    assert cpu.initialize(bf.linear_geometry(4, 0.04), 10, rate) == -1
    assert "16000" in cpu.why and "high_frequency_upper_bin_bound_" in cpu.why
    with pytest.raises(ValueError):
        cpu.process_chunk(np.zeros((4, 160), np.float32))


def test_other_chunk_sizes_and_microphone_counts_are_refused():
    cpu = bf.Restate()
    assert cpu.initialize(bf.linear_geometry(4, 0.04), 20, 16000) == -1 and "10 ms" in cpu.why
    for M in (0, 1, 9):
        assert cpu.initialize(bf.linear_geometry(max(M, 1), 0.04), num_mics=M) == -1 and "2 to 8" in cpu.why
    assert cpu.initialize(bf.linear_geometry(2, 0.05)) == 0 and cpu.initialize(bf.linear_geometry(8, 0.02)) == 0


def test_a_non_uniform_geometry_is_refused_where_the_reference_checks():
    """MicSpacingFromGeometry CHECKs g[j] - g[j-1] - (g[1] - g[0]) < 1e-6 per axis: one-sided, as the reference."""
    cpu = bf.Restate()
    g = bf.linear_geometry(4, 0.04)
    g[3, 0] += 0.01
    assert cpu.initialize(g) == -1 and "uniform linear array" in cpu.why
    g = bf.linear_geometry(3, 0.04)
    g[2, 1] = 0.001
    assert cpu.initialize(g) == -1
    g = bf.linear_geometry(4, 0.04)
    g[:, 1] = np.arange(4) * 0.03   # uniform along a diagonal: spacing 0.05
    assert cpu.initialize(g) == 0
    assert abs(float(cpu.L.BfRestate_MicSpacing(cpu.h)) - 0.05) < 1e-6
