#!/usr/bin/env python3
"""Generates tests/golden/bt_golden_<window>.npz from the REFERENCE BlockThresholding build
(oracle/_ref/libbt_ref.so: the reference's audioDenoiseBlockTreshold.c compiled in place, its kiss_fft calls
forwarded to the oracle's FFT; oracle/ref_probe_bt.c).  Build-container only.  The runs, the inputs and the
layout of the files are those of tests/bt_runs.py; every array comes out of the reference's own entry points."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import bt_runs as R  # noqa: E402
from tests.oracle_lib import RefBt, have_bt_ref  # noqa: E402

CAN_OUTPUT = 0x20


def _init(n):
    r = RefBt(*R.GOLDEN_INIT[n])
    assert r.err == 0 and r.win == n
    return r


def _segments_of_first_macroblock(n, x):
    """(seg_time, seg_freq) per macro-column of macroblock 0: frame t of a stream's first macroblock is the window over
    [hop t - 1 | hop t] (zeros ahead of hop 0), which a fresh handle transforms when fed just those hops; the eight
    spectra then go through the reference's blockThreshold_adaptive_block (ref_bt_core)."""
    r = _init(n)
    hops = x[:r.macro].reshape(8, r.half)
    coef = np.empty((8, n // 2 + 1), np.complex64)
    for t in range(8):
        r.reset()
        for hop in hops[max(t - 1, 0):t + 1]:
            r.denoise_float(hop)
        coef[t] = r.coef(r.have() - 1)
    with np.errstate(all="ignore"):
        return r.core(coef)[2]


def one_window(n):
    q = R.golden_grid(n)
    x = R.inputs_from_grid(q)
    half, macro = n // 2, 4 * n
    a = {k: [] for k in ("out", "in_tail", "out_tail", "flush", "out16", "out16_undef", "flush16", "flush16_undef", "seg")}
    for s in range(8):
        # float path
        r = _init(n)
        out = []
        for k, hop in enumerate(x[s, :R.K * macro].reshape(-1, half)):
            rc = r.denoise_float(hop)
            assert rc == (CAN_OUTPUT if k % 8 == 7 else 0x10)
            if rc == CAN_OUTPUT:
                got, y = r.output_float()
                assert got == macro
                out.append(y)
        a["out"].append(np.concatenate(out))
        a["in_tail"].append(r.inbuf()[half:])
        a["out_tail"].append(r.outbuf()[macro:])
        for hop in x[s, R.K * macro:].reshape(R.FLUSH_HOPS, half):
            assert r.denoise_float(hop) == 0x10
        got, y = r.flush_float(R.FLUSH_HOPS * half)
        assert got == R.FLUSH_HOPS * half
        a["flush"].append(y)
        a["seg"].append(_segments_of_first_macroblock(n, x[s]))
        # int16 path
        r = _init(n)
        out, undef = [], []
        for hop in q[s, :R.K * macro].reshape(-1, half):
            if r.denoise_int16(hop) == CAN_OUTPUT:
                undef.append(np.isnan(r.output_float()[1]))
                got, y = r.output_int16()
                assert got == macro
                out.append(y)
        a["out16"].append(np.concatenate(out))
        a["out16_undef"].append(np.concatenate(undef).astype(np.int16))
        for hop in q[s, R.K * macro:].reshape(R.FLUSH_HOPS, half):
            assert r.denoise_int16(hop) == 0x10
        got, y = r.flush_int16(R.FLUSH_HOPS * half)
        assert got == R.FLUSH_HOPS * half
        a["flush16"].append(y)
        a["flush16_undef"].append(np.isnan(r.outbuf()[:got]).astype(np.int16))
    a = {k: np.stack(v) for k, v in a.items()}
    a["q"] = q
    a["seg"] = a["seg"].astype(np.int32)
    assert not a["seg"][R.LOUD].any(), "the loud-noise stream is there for the 8 x 16 block in every macro-column"
    assert np.isnan(a["out"][1]).all(), "digital silence is there for the 0 / 0 gains"
    for k, v in a.items():
        assert v.dtype in (np.float32, np.int16, np.int32), (k, v.dtype)
    return a


def main():
    assert have_bt_ref(), "build oracle/_ref first (make -C oracle)"
    for n in R.GOLDEN_WINDOWS:
        a = one_window(n)
        path = R.golden_path(n)
        np.savez_compressed(path, **a)
        print("wrote", path, os.path.getsize(path), "bytes;", "segmentations in use:",
              len({(int(t), int(f)) for t, f in a["seg"].reshape(-1, 2)}))


if __name__ == "__main__":
    main()
