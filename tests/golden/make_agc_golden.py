"""Writes tests/golden/agc_golden.npz from the reference gain control compiled in place:

    R=<reference>/WebRtc_AMP_Port; A=$R/webrtc/common_audio/signal_processing
    M=$R/webrtc/modules/audio_processing/agc/legacy
    gcc -O2 -fwrapv -fPIC -shared -I$R -Iinclude $M/analog_agc.c $M/digital_agc.c $A/resample_by_2.c \
        $A/dot_product_with_scale.c $A/division_operations.c $A/spl_sqrt.c $A/copy_set_operations.c \
        tests/golden/agc_ref_shim.c -o libagc_ref.so
    sed -e 's|^static const int16_t kAvgDecayTime|int agc_limiter_hits, agc_limiter_wide_hits, agc_gate_wide_hits, agc_first_clip_hits;\n&|' \
        -e 's|// multiply by 253/256 ==> -0.1 dB|agc_limiter_hits++;|' \
        -e 's|gains\[k + 1\] = (gains\[k+1\] / 256) \* 253;|& agc_limiter_wide_hits++;|' \
        -e 's|tmp32 \*= 178 + gain_adj;|& agc_gate_wide_hits++;|' \
        -e 's|out\[i\]\[n\] = (int16_t)32767;|& agc_first_clip_hits++;|' \
        -e 's|out\[i\]\[n\] = (int16_t)-32768;|& agc_first_clip_hits++;|' $M/digital_agc.c > scratch/digital_agc_count.c
    (the same gcc line with scratch/digital_agc_count.c in place of $M/digital_agc.c) -o libagc_ref_counting.so
    python tests/golden/make_agc_golden.py libagc_ref.so libagc_ref_counting.so

The second library is the same build with four counters in a scratch copy of digital_agc.c (not committed): the paths
inside ProcessDigital cannot be told apart from outside.  It must give the first library's outputs, and it is what the
limiter conditions below are asserted on.

-fwrapv: the reference relies on 32-bit wrap-around (gain32 *= gain32 in the limiter, left shifts of negative
values, the AgcVad energy); the flag makes that defined, and csrc/agc_core.h does the same arithmetic on
uint32_t.  The shim zeroes the LegacyAgc before Init: WebRtcAgc_Init leaves Rxx16w32_array[1] and other fields
as malloc gave them, and a state of this project is zero after Create.

Each run of tests/agc_runs.py drives WebRtcAgc_* on inputs regenerated from synth.  The golden stores no audio
input, only a sha256 of it, and per run every output sample, every outMicLevel, every saturationWarning,
every return value, and the full state (AspAgcState field by field) at the run's snapshot frames; plus the
gain table for a grid of (compression, target, limiter, analogTarget).

Coverage, asserted on the reference alone (the runs that meet each, as last generated):
    outMicLevel rises                        runs 0, 1, 5, 7    outMicLevel falls               runs 0, 1
    saturationWarning == 1                   run 0              the zero-input control raises the level   runs 0, 5
    lowLevelSignal 0 and 1                   runs 1, 3, 6, 7    VirtualMic clips a sample       run 1
    AddMic's digital gain (gainTableIdx > 0) run 7              the gate is open (gatePrevious > 0)   runs 0, 1, 2, 5, 6, 7, 8
    first-sub-frame clip gives +-full scale  runs 1, 4, 8 (seen in the output, and counted)
    the limiter loop lowers a gain           runs 4, 8 (counted)
    the limiter's / 256 * 253 branch (a gain above 8388607)   run 8 (counted)
    the gate's >> 8 first branch (a gain more than 8388608 over gainTable[0])   run 8 (counted)
    a return value of -1 (ProcessAnalog: a level above maxAnalog after the re-Init)   run 7
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from audiosignalprocess_amd.agc import AspAgcState, WebRtcAgcConfig, state_dict  # noqa: E402
from tests.agc_runs import RUNS, inputs, replay  # noqa: E402

GRID = [(c, t, l, a) for c in (0, 3, 9, 15, 20, 30, 45, 90) for t in (0, 3, 6, 12, 31) for l in (0, 1)
        for a in (4, 8, 12, 20, 30)]
P, I16, I32, U8 = C.c_void_p, C.c_int16, C.c_int32, C.c_uint8


def load(path):
    L = C.CDLL(path)
    L.agc_ref_create.restype = P
    L.agc_ref_state.argtypes = [P, P]
    L.WebRtcAgc_Free.argtypes = [P]
    L.WebRtcAgc_Init.argtypes = [P, I32, I32, I16, C.c_uint32]
    L.WebRtcAgc_set_config.argtypes = [P, WebRtcAgcConfig]
    L.WebRtcAgc_AddFarend.argtypes = [P, P, I16]
    L.WebRtcAgc_AddMic.argtypes = [P, P, I16, I16]
    L.WebRtcAgc_VirtualMic.argtypes = [P, P, I16, I16, I32, C.POINTER(I32)]
    L.WebRtcAgc_Process.argtypes = [P, P, I16, I16, P, I32, C.POINTER(I32), I16, C.POINTER(U8)]
    L.WebRtcAgc_CalculateGainTable.argtypes = [P, I16, I16, U8, I16]
    return L


class Ref:
    """The adapter tests/agc_runs.replay drives; keeps what the coverage conditions need."""

    def __init__(self, L, spec, data, key):
        self.L, self.spec, self.data, self.key = L, spec, data, key
        self.h = P(L.agc_ref_create())
        self.seen = set()
        self.level_in = None

    def state(self):
        st = AspAgcState()
        self.L.agc_ref_state(self.h, C.addressof(st))
        return st

    def init(self, *a):
        return self.L.WebRtcAgc_Init(self.h, *a)

    def set_config(self, t, c, l):
        return self.L.WebRtcAgc_set_config(self.h, WebRtcAgcConfig(t, c, l))

    def far(self, x):
        return self.L.WebRtcAgc_AddFarend(self.h, x.ctypes.data, x.size)

    def _bands(self, y):
        return (P * y.shape[0])(*[y[b].ctypes.data for b in range(y.shape[0])])

    def add_mic(self, x):
        y = x.copy()
        rc = self.L.WebRtcAgc_AddMic(self.h, self._bands(y), y.shape[0], y.shape[1])
        if self.state().gainTableIdx > 0:
            self.seen.add("digital_gain")
        return rc, y

    def virtual_mic(self, x, level):
        y = x.copy()
        st = self.state()
        before = min(st.micVol, st.maxAnalog) if level == st.micRef else 127
        out = I32()
        rc = self.L.WebRtcAgc_VirtualMic(self.h, self._bands(y), y.shape[0], y.shape[1], level, C.byref(out))
        if out.value < before:
            self.seen.add("virtual_mic_clip")
        self.seen.add("low_level_%d" % self.state().lowLevelSignal)
        return rc, y, out.value

    def process(self, x, level, echo):
        y = np.zeros_like(x)
        out, sat = I32(), U8()
        before = self.state()
        rc = self.L.WebRtcAgc_Process(self.h, self._bands(x), x.shape[0], x.shape[1], self._bands(y), level, C.byref(out),
                                      echo, C.byref(sat))
        st = self.state()
        if out.value > level:
            self.seen.add("rise")
            if st.muteGuardMs == 8000 and before.msZero == 500:
                self.seen.add("zero_ctrl_rise")
        if out.value < level:
            self.seen.add("fall")
        if sat.value == 1:
            self.seen.add("saturation")
        if st.digitalAgc_gatePrevious > 0:
            self.seen.add("gate")
        L1 = x.shape[1] // 10
        first = y[0, :L1].astype(np.int32)
        if np.any(((first == 32767) | (first == -32768)) & (np.abs(x[0, :L1].astype(np.int32)) < 32767)):
            self.seen.add("first_clip")
        return rc, y, out.value, sat.value

    def snapshot(self, f):
        if f in self.spec["snaps"]:
            for n, v in state_dict(self.state()).items():
                self.data["%s_s%d_%s" % (self.key, f, n)] = v

    def close(self):
        self.L.WebRtcAgc_Free(self.h)


def main():
    L = load(sys.argv[1])
    data, seen = {}, {}
    for i, spec in enumerate(RUNS):
        sha = hashlib.sha256()
        for x, far in inputs(spec):
            sha.update(x.tobytes())
            if far is not None:
                sha.update(far.tobytes())
        r = Ref(L, spec, data, "r%d" % i)
        out, levels, sats, rcs = replay(spec, r)
        r.close()
        data["r%d_sha" % i] = np.frombuffer(sha.digest(), np.uint8)
        data["r%d_out" % i], data["r%d_level" % i], data["r%d_sat" % i], data["r%d_rc" % i] = out, levels, sats, rcs
        for k in r.seen:
            seen.setdefault(k, []).append(i)
        print("run", i, "done:", out.size, "samples; levels", levels.min(), "..", levels.max(), "rc", sorted(set(rcs.tolist())),
              sorted(r.seen))
    want = ["rise", "fall", "saturation", "zero_ctrl_rise", "low_level_0", "low_level_1", "virtual_mic_clip",
            "digital_gain", "gate", "first_clip"]
    for k in want:
        print("%-18s runs %s" % (k, seen.get(k)))
    missing = [k for k in want if k not in seen]
    assert not missing, "the runs do not reach: %r" % missing
    K = load(sys.argv[2])
    names = ["agc_limiter_hits", "agc_limiter_wide_hits", "agc_gate_wide_hits", "agc_first_clip_hits"]
    hits = {name: [] for name in names}
    for i, spec in enumerate(RUNS):
        for name in names:
            C.c_int.in_dll(K, name).value = 0
        r = Ref(K, spec, {}, "k")
        out = replay(spec, r)[0]
        r.close()
        assert np.array_equal(out, data["r%d_out" % i])
        for name in names:
            if C.c_int.in_dll(K, name).value > 0:
                hits[name].append(i)
    for name in names:
        print("%-22s runs %s" % (name, hits[name]))
    assert all(hits[name] for name in names), hits
    table = np.zeros((len(GRID), 33), np.int32)
    for k, (c, t, l, a) in enumerate(GRID):
        table[k, 0] = L.WebRtcAgc_CalculateGainTable(table[k, 1:].ctypes.data, c, t, l, a)
    data["gain_grid"] = np.array(GRID, np.int32)
    data["gain_tables"] = table
    np.savez_compressed(os.path.join(HERE, "agc_golden.npz"), **data)
    print(os.path.getsize(os.path.join(HERE, "agc_golden.npz")), "bytes")


if __name__ == "__main__":
    main()
