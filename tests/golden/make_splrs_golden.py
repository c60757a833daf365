"""Writes tests/golden/splrs_golden.npz from the reference resampler compiled in place:

    R=<reference>/WebRtc_AMP_Port; A=$R/webrtc/common_audio
    gcc -O2 -fPIC -I$R -c $A/signal_processing/resample_by_2.c $A/signal_processing/resample_48khz.c \
        $A/signal_processing/resample.c $A/signal_processing/resample_by_2_internal.c \
        $A/signal_processing/resample_fractional.c
    g++ -O2 -fPIC -I$R -c $A/resampler/resampler.cc tests/golden/splrs_ref_shim.cc
    g++ -shared -o libsplrs_ref.so *.o
    python tests/golden/make_splrs_golden.py libsplrs_ref.so

Each run of tests/splrs_runs.py drives webrtc::Resampler (Reset / ResetIfNeeded / Push) through the shim on
inputs regenerated from synth.  The golden stores no audio input, only a sha256 of it, and per run every
output sample plus, at the run's snapshot frames, state1_ .. state3_ as int32 [3][32] (zero beyond what Reset
allocated) -- of the instance itself, or of both slaves for a stereo run.  The recorded return values are
[Reset rc, Push rc] per case of splrs_runs.RETURNS.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.splrs_runs import RETURNS, RUNS, STAGE_WORDS, SYNC, SYNC_STEREO, inputs  # noqa: E402


def main():
    L = C.CDLL(sys.argv[1])
    P = C.c_void_p
    L.splrs_ref_create.restype = P
    L.splrs_ref_free.argtypes = [P]
    L.splrs_ref_reset.argtypes = [P, C.c_int, C.c_int, C.c_int]
    L.splrs_ref_reset_if_needed.argtypes = [P, C.c_int, C.c_int, C.c_int]
    L.splrs_ref_push.argtypes = [P, P, C.c_int, P, C.c_int, C.POINTER(C.c_int)]
    L.splrs_ref_mode.argtypes = [P]
    L.splrs_ref_state.argtypes = [P, C.c_int, C.c_int, C.c_int, P]

    def snapshot(h, which):
        st = np.zeros((3, 32), np.int32)
        for k, words in enumerate(STAGE_WORDS[L.splrs_ref_mode(h)]):
            assert L.splrs_ref_state(h, which, k, words, st[k].ctypes.data) == 0
        return st

    data, modes = {}, set()
    for i, spec in enumerate(RUNS):
        ch = spec.get("channels", 1)
        typ = SYNC_STEREO if ch == 2 else SYNC
        h = P(L.splrs_ref_create())
        assert L.splrs_ref_reset(h, spec["rates"][0], spec["rates"][1], typ) == 0
        sha = hashlib.sha256()
        outs = []
        for f, x in enumerate(inputs(spec)):
            ev = spec.get("events", {}).get(f)
            if ev:
                fn = L.splrs_ref_reset if ev[0] == "reset" else L.splrs_ref_reset_if_needed
                assert fn(h, ev[1], ev[2], typ) == 0
            modes.add(L.splrs_ref_mode(h))
            sha.update(x.tobytes())
            y = np.zeros(12 * x.size, np.int16)
            n = C.c_int(0)
            assert L.splrs_ref_push(h, x.ctypes.data, x.size, y.ctypes.data, y.size, C.byref(n)) == 0, (i, f)
            outs.append(y[:n.value].copy())
            if f in spec["snaps"]:
                for c in range(ch):
                    data["r%d_s%d_c%d" % (i, f, c)] = snapshot(h, 0 if ch == 1 else 1 + c)
        L.splrs_ref_free(h)
        data["r%d_sha" % i] = np.frombuffer(sha.digest(), np.uint8)
        data["r%d_out" % i] = np.concatenate(outs)
        print("run", i, "done:", data["r%d_out" % i].size, "samples")
    assert modes == set(range(21)), sorted(modes)
    for name, (reset, n, max_len) in RETURNS.items():
        h = P(L.splrs_ref_create())
        rc = [L.splrs_ref_reset(h, *reset)]
        x, y, k = np.zeros(n, np.int16), np.zeros(8000, np.int16), C.c_int(0)
        rc.append(L.splrs_ref_push(h, x.ctypes.data, n, y.ctypes.data, max_len, C.byref(k)))
        L.splrs_ref_free(h)
        data["ret_" + name] = np.array(rc, np.int32)
        print(name, rc)
    np.savez_compressed(os.path.join(HERE, "splrs_golden.npz"), **data)


if __name__ == "__main__":
    main()
