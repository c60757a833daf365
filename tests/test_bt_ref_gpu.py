"""GPU parity suite for BlockThresholding against the reference build (-m gpu): the HIP kernels through the batch
C-ABI and the blockThreshold_* exports of libasp_amd.so against tests/golden/bt_golden_<window>.npz, which
tests/golden/make_bt_golden.py wrote from the reference's audioDenoiseBlockTreshold.c compiled in place
(tests/bt_runs.py describes the runs and the arrays).  Everything is equality, NaNs compared by position.  The golden
files are the only reference read here: nothing from oracle/."""
import ctypes as C

import numpy as np
import pytest

from tests import bt_runs as R

pytestmark = pytest.mark.gpu

_golden = {}


def golden(n):
    if n not in _golden:
        g = R.load_golden(n)
        g["x"] = R.inputs_from_grid(g["q"])
        _golden[n] = g
    return _golden[n]


@pytest.fixture(scope="module")
def bt():
    from audiosignalprocess_amd import bt as mod
    from audiosignalprocess_amd import ns

    assert ns.device_count() >= 1
    return mod


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def first_diff(a, b):
    """(flat index, got, want) of the first differing sample, NaNs compared by position; None when equal."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    bad = np.nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))[0]
    return None if bad.size == 0 else (int(bad[0]), float(a[bad[0]]), float(b[bad[0]]))


def tails(g, s, half):
    st = g.export_state(s)
    return np.ctypeslib.as_array(st.inbuf_tail)[:half].copy(), np.ctypeslib.as_array(st.out_tail)[:half].copy()


def check_batch_against_golden(bt, n, S):
    """K macroblocks through BtBatch.run, the state left behind, then the flush with FLUSH_HOPS pending hops."""
    G = golden(n)
    idx = R.tile_streams(S)
    macro, half = 4 * n, n // 2
    g = bt.BtBatch(S, n)
    with np.errstate(all="ignore"):
        y = g.run(G["x"][idx, :R.K * macro])
    for s in range(S):
        assert same(y[s], G["out"][idx[s]]), (s, R.STREAM_NAMES[idx[s]], first_diff(y[s], G["out"][idx[s]]))
        it, ot = tails(g, s, half)
        assert same(it, G["in_tail"][idx[s]]) and same(ot, G["out_tail"][idx[s]]), (s, R.STREAM_NAMES[idx[s]])
    fl = g.flush(G["x"][idx, R.K * macro:], R.FLUSH_HOPS)
    for s in range(S):
        assert same(fl[s], G["flush"][idx[s]]), (s, R.STREAM_NAMES[idx[s]], first_diff(fl[s], G["flush"][idx[s]]))
    g.close()


@pytest.mark.parametrize("n", R.GOLDEN_WINDOWS)
def test_batch_run_equals_reference_golden(bt, n):
    check_batch_against_golden(bt, n, 8)


def test_batch_run_256_groups_of_four_and_plain_kernel(bt, monkeypatch):
    """13 streams at 256 samples: three workgroups of four stream-channels (Q4) and one left-over stream through the
    plain kernel; then every stream through the plain kernel (ASP_BT_OLD_KERNEL)."""
    check_batch_against_golden(bt, 256, 13)
    monkeypatch.setenv("ASP_BT_OLD_KERNEL", "1")
    check_batch_against_golden(bt, 256, 13)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("n,S", [(1024, 1), (1024, 3), (256, 4), (256, 8)])
def test_handoff_build_small_batches_equal_reference_golden(bt, n, S, K):
    """AspBtBatch_DenoiseBlocks with the hand-off build forced on, at the smallest batches: the first and the last
    step of a stream-channel are co-resident, the shape in which the last step's carry of the input tail into the
    state must stay behind the first step's read of it.  K macroblocks in one launch (K = 2: the third through a
    plain Denoise call): outputs and state equal the golden.  Then the same blocks once more in a second hand-off
    launch -- its first step reads the tails the previous launch left in the state -- against a batch that takes one
    launch per macroblock."""
    G = golden(n)
    idx = R.tile_streams(S)
    macro, half = 4 * n, n // 2
    x = np.ascontiguousarray(G["x"][idx, :R.K * macro].reshape(S, R.K, macro).transpose(1, 0, 2))   # [K][S][macro]
    runs = []
    for flow in (1, 0):
        g = bt.BtBatch(S, n)
        g.set_flow(flow)
        with np.errstate(all="ignore"):
            y = g.denoise_blocks(x[:K])
            if K < R.K:
                y = np.concatenate([y, g.denoise(x[K])[None]])
            t1 = [tails(g, s, half) for s in range(S)]
            y2 = g.denoise_blocks(x[:K])
            t2 = [tails(g, s, half) for s in range(S)]
        runs.append((y, t1, y2, t2))
        g.close()
    for y, t1, _, _ in runs:
        for s in range(S):
            want = G["out"][idx[s]].reshape(R.K, macro)
            assert same(y[:, s], want), (s, R.STREAM_NAMES[idx[s]], first_diff(y[:, s], want))
            assert same(t1[s][0], G["in_tail"][idx[s]]) and same(t1[s][1], G["out_tail"][idx[s]]), s
    assert same(runs[0][2], runs[1][2]), first_diff(runs[0][2], runs[1][2])
    for s in range(S):
        assert same(runs[0][3][s][0], runs[1][3][s][0]) and same(runs[0][3][s][1], runs[1][3][s][1]), s
        assert same(runs[0][3][s][0], x[K - 1, s, -half:])      # the input tail IS the last half window fed


def _layer1(built_lib):
    lib = C.CDLL(built_lib)
    lib.blockThreshold_init.restype = C.c_void_p
    lib.blockThreshold_init.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    for name in ("denoise_float", "output_float", "flush_float", "denoise_int16", "output_int16", "flush_int16"):
        getattr(lib, "blockThreshold_" + name).argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.blockThreshold_free.argtypes = [C.c_void_p]
    lib.blockThreshold_max_output.argtypes = [C.c_void_p]
    lib.blockThreshold_samples_per_time.argtypes = [C.c_void_p]
    return lib


@pytest.mark.parametrize("n", R.GOLDEN_WINDOWS)
def test_layer1_exports_equal_reference_golden(bt, built_lib, n):
    """blockThreshold_* of libasp_amd.so, one handle per golden stream, hop by hop: the float path, the int16 path and
    the flush with FLUSH_HOPS pending hops of both.  int16 samples whose float value is NaN are left out: the
    reference's cast is undefined there."""
    lib = _layer1(built_lib)
    G = golden(n)
    macro, half = 4 * n, n // 2
    nfl = R.FLUSH_HOPS * half
    err = C.c_int32(-1)
    for s in range(8):
        name = R.STREAM_NAMES[s]
        for pcm in (False, True):
            h = lib.blockThreshold_init(*R.GOLDEN_INIT[n], C.byref(err))
            assert h and err.value == 0
            assert lib.blockThreshold_max_output(h) == macro and lib.blockThreshold_samples_per_time(h) == half
            src = G["q"][s] if pcm else G["x"][s]
            dt = np.int16 if pcm else np.float32
            denoise = lib.blockThreshold_denoise_int16 if pcm else lib.blockThreshold_denoise_float
            output = lib.blockThreshold_output_int16 if pcm else lib.blockThreshold_output_float
            flush = lib.blockThreshold_flush_int16 if pcm else lib.blockThreshold_flush_float
            out = []
            for k in range(R.K * 8 + R.FLUSH_HOPS):
                hop = np.ascontiguousarray(src[k * half:(k + 1) * half])
                rc = denoise(h, hop.ctypes.data, half)
                assert rc == (0x20 if k % 8 == 7 and k < R.K * 8 else 0x10), (name, k, rc)
                if rc == 0x20:
                    y = np.zeros(macro, dt)
                    assert output(h, y.ctypes.data, macro - 1) == 0
                    assert output(h, y.ctypes.data, macro) == macro
                    out.append(y)
            out = np.concatenate(out)
            fl = np.zeros(nfl, dt)
            assert flush(h, fl.ctypes.data, nfl - 1) == -1
            assert flush(h, fl.ctypes.data, nfl) == nfl
            lib.blockThreshold_free(h)
            if pcm:
                keep, keep_fl = G["out16_undef"][s] == 0, G["flush16_undef"][s] == 0
                assert same(out[keep], G["out16"][s][keep]), (name, first_diff(out[keep], G["out16"][s][keep]))
                assert same(fl[keep_fl], G["flush16"][s][keep_fl]), name
            else:
                assert same(out, G["out"][s]), (name, first_diff(out, G["out"][s]))
                assert same(fl, G["flush"][s]), (name, first_diff(fl, G["flush"][s]))


@pytest.mark.parametrize("n,S", [(1024, 1100), (256, 2052), (1024, 3)])
def test_device_buffers_that_overlap(bt, n, S):
    """AspBtBatch_DenoiseBlocks / TimedSteps on device memory with out == in, and with out one macroblock below / above
    in, hand-off build forced on, 7 macroblocks.  The hand-off build reads a step's input tail from the previous
    macroblock's input slot, so a call whose buffers overlap must take one launch per macroblock; the plain kernels
    read a macroblock's input ahead of their first output store.  (1024, 1100) and (256, 2052): more than 2 x 256
    workgroups per step, a step's workgroups are not all resident beside the previous step's; (1024, 3): all are.
    Results: those of the run with separate buffers and one launch per macroblock, which in its first K macroblocks is
    the tiled golden."""
    from audiosignalprocess_amd.ns import DeviceBuffer

    G = golden(n)
    idx = R.tile_streams(S)
    macro, half, NB = 4 * n, n // 2, 7
    blocks = np.arange(NB) % R.K                                   # the golden's K macroblocks, over and over
    x = np.ascontiguousarray(G["x"][idx, :R.K * macro].reshape(S, R.K, macro).transpose(1, 0, 2)[blocks])  # [NB][S][macro]
    per = S * macro * 4                                            # bytes per macroblock slot
    buf = DeviceBuffer((2 * NB + 1) * per)
    spot = sorted({0, 1, S // 2, S - 1})

    def run(flow, in_slot, out_slot, timed=False):
        g = bt.BtBatch(S, n)
        g.set_flow(flow)
        assert buf.lib.AspNs_MemcpyH2D(C.c_void_p(buf.ptr + in_slot * per), C.c_void_p(x.ctypes.data), x.nbytes) == 0
        if timed:
            g.timed_steps(buf.ptr + in_slot * per, buf.ptr + out_slot * per, NB, NB)
        else:
            g.denoise_blocks_device(buf.ptr + in_slot * per, buf.ptr + out_slot * per, NB)
        g.synchronize()
        y = np.empty_like(x)
        assert buf.lib.AspNs_MemcpyD2H(C.c_void_p(y.ctypes.data), C.c_void_p(buf.ptr + out_slot * per), y.nbytes) == 0
        st = [tails(g, s, half) for s in spot]
        g.close()
        return y, st

    def equal(a, b, what):
        assert same(a[0], b[0]), (what, first_diff(a[0], b[0]))
        for (ai, ao), (bi, bo) in zip(a[1], b[1]):
            assert same(ai, bi) and same(ao, bo), what

    with np.errstate(all="ignore"):
        base = run(0, 0, NB + 1)                                   # separate buffers, one launch per macroblock
        for s in range(min(S, 16)):
            want = G["out"][idx[s]].reshape(R.K, macro)
            assert same(base[0][:R.K, s], want), (s, first_diff(base[0][:R.K, s], want))
        equal(run(1, 0, 0), base, "DenoiseBlocks in place")
        equal(run(1, 0, 0, timed=True), base, "TimedSteps in place")
        equal(run(1, 1, 0), base, "out one macroblock below in")
        # out one macroblock above in: every macroblock but the first reads what its predecessor wrote -- defined by
        # the launch order of the plain path, whatever the hand-off setting
        equal(run(1, 0, 1), run(0, 0, 1), "out one macroblock above in")
    buf.free()
