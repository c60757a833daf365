"""Writes tests/golden/agc_golden.npz and tests/golden/agc_edges_golden.npz from the reference gain control compiled in
place (oracle/Makefile: _ref/libagc_ref.so, which build() makes where the reference is present):

    python tests/golden/make_agc_golden.py [--edges] [--check] [libagc_ref.so [libagc_ref_counting.so]]

Without --edges: the golden runs (tests/agc_runs.RUNS) and the gain-table grid into agc_golden.npz.  With --edges:
EDGE_RUNS, the SEEDED case and EDGE_GRID into agc_edges_golden.npz; a run longer than 120 frames keeps its output
samples for the 20 frames from each snapshot on and a sha256 per block of 50 frames (tests/edge_pack.py).  --check
writes nothing: it regenerates every array from the reference build and compares it with the committed file (the
counting build below plays no part in that).  The first library's recipe, and the second's, which the writer follows
itself in a temporary directory when no second library is named:

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
from tests import agc_runs  # noqa: E402
from tests.edge_pack import pack_state  # noqa: E402
from tests.agc_runs import EDGE_GRID, EDGE_RUNS, RUNS, SEEDED, inputs, replay  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(HERE))
DEFAULT_LIB = os.path.join(ROOT, "oracle", "_ref", "libagc_ref.so")

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
        if f in self.spec["snaps"] and self.key.startswith("e"):   # an edge run: the state as one array
            self.data["%s_s%d" % (self.key, f)] = pack_state(AspAgcState, state_dict(self.state()))
        elif f in self.spec["snaps"]:
            for n, v in state_dict(self.state()).items():
                self.data["%s_s%d_%s" % (self.key, f, n)] = v

    def close(self):
        self.L.WebRtcAgc_Free(self.h)


def input_sha(spec):
    sha = hashlib.sha256()
    for x, far in inputs(spec):
        sha.update(x.tobytes())
        if far is not None:
            sha.update(far.tobytes())
    return np.frombuffer(sha.digest(), np.uint8)


def build_counting(tmp):
    """The docstring's second recipe: the same build with four counters in a scratch copy of digital_agc.c, in tmp."""
    import re
    import subprocess

    R = os.path.join(os.environ.get("REF", "/root/reference"), "WebRtc_AMP_Port")
    A = os.path.join(R, "webrtc", "common_audio", "signal_processing")
    M = os.path.join(R, "webrtc", "modules", "audio_processing", "agc", "legacy")
    with open(os.path.join(M, "digital_agc.c")) as f:
        src = f.read()
    for pat, rep in ((r"^static const int16_t kAvgDecayTime", "int agc_limiter_hits, agc_limiter_wide_hits, agc_gate_wide_hits, agc_first_clip_hits;\n\\g<0>"),
                     (r"// multiply by 253/256 ==> -0.1 dB", "agc_limiter_hits++;"),
                     (r"gains\[k \+ 1\] = \(gains\[k\+1\] / 256\) \* 253;", "\\g<0> agc_limiter_wide_hits++;"),
                     (r"tmp32 \*= 178 \+ gain_adj;", "\\g<0> agc_gate_wide_hits++;"),
                     (r"out\[i\]\[n\] = \(int16_t\)32767;", "\\g<0> agc_first_clip_hits++;"),
                     (r"out\[i\]\[n\] = \(int16_t\)-32768;", "\\g<0> agc_first_clip_hits++;")):
        src, k = re.subn(pat, rep, src, flags=re.M)
        assert k >= 1, pat
    with open(os.path.join(tmp, "digital_agc_count.c"), "w") as f:
        f.write(src)
    lib = os.path.join(tmp, "libagc_ref_counting.so")
    subprocess.run(["gcc", "-O2", "-fwrapv", "-fPIC", "-shared", "-w", "-I" + R, "-I" + M, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(M, "analog_agc.c"), os.path.join(tmp, "digital_agc_count.c")] +
                   [os.path.join(A, f) for f in ("resample_by_2.c", "dot_product_with_scale.c", "division_operations.c", "spl_sqrt.c",
                                                 "copy_set_operations.c")] + [os.path.join(HERE, "agc_ref_shim.c"), "-o", lib], check=True)
    return lib


def golden_arrays(L, counting, check):
    data, seen = {}, {}
    for i, spec in enumerate(RUNS):
        r = Ref(L, spec, data, "r%d" % i)
        out, levels, sats, rcs = replay(spec, r)
        r.close()
        data["r%d_sha" % i] = input_sha(spec)
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
    table = np.zeros((len(GRID), 33), np.int32)
    for k, (c, t, l, a) in enumerate(GRID):
        table[k, 0] = L.WebRtcAgc_CalculateGainTable(table[k, 1:].ctypes.data, c, t, l, a)
    data["gain_grid"] = np.array(GRID, np.int32)
    data["gain_tables"] = table
    if check:
        return data
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        counted(load(counting or build_counting(tmp)), data)
    return data


def counted(K, data):
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


def edge_arrays(L):
    data = {}
    for i, spec in enumerate(EDGE_RUNS):
        r = Ref(L, spec, data, "e%d" % i)
        out, levels, sats, rcs = replay(spec, r)
        r.close()
        data["e%d_sha" % i] = input_sha(spec)
        data["e%d_keep" % i], data["e%d_blocks" % i] = agc_runs.pack_outputs(spec, out)
        data["e%d_level" % i], data["e%d_sat" % i], data["e%d_rc" % i] = levels, sats, rcs
        d = np.diff(levels)
        print("edge run", i, "done: levels", levels.min(), "..", levels.max(), "steps up", int((d > 0).sum()), "down", int((d < 0).sum()),
              "rc", sorted(set(rcs.tolist())), sorted(r.seen))
    for k, case in enumerate(SEEDED):
        spec = dict(EDGE_RUNS[case["base"]], snaps=())
        r = Ref(L, spec, {}, "x")
        level = int(replay(spec, r, stop=case["at"])[1][-1])
        L.agc_ref_set.argtypes = [P, C.c_char_p, C.c_int]
        for name, v in case["plant"].items():
            assert L.agc_ref_set(r.h, name.encode(), v) == 0, name
        data["sd%d_in" % k] = pack_state(AspAgcState, state_dict(r.state()))
        data["sd%d_level_in" % k] = np.array([level], np.int32)
        out, levels, sats, rcs = agc_runs.replay_seeded(case, r, level)
        data["sd%d_out" % k], data["sd%d_level" % k], data["sd%d_sat" % k], data["sd%d_rc" % k] = out, levels, sats, rcs
        data["sd%d_s" % k] = pack_state(AspAgcState, state_dict(r.state()))
        r.close()
        print("seeded case", k, "done: levels", levels.tolist())
    table = np.zeros((len(EDGE_GRID), 33), np.int32)
    for k, (c, t, l, a) in enumerate(EDGE_GRID):
        table[k, 0] = L.WebRtcAgc_CalculateGainTable(table[k, 1:].ctypes.data, c, t, l, a)
    data["gain_grid"] = np.array(EDGE_GRID, np.int32)
    data["gain_tables"] = table
    return data


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    edges, check = "--edges" in sys.argv, "--check" in sys.argv
    L = load(args[0] if args else DEFAULT_LIB)
    data = edge_arrays(L) if edges else golden_arrays(L, args[1] if len(args) > 1 else None, check)
    path = os.path.join(HERE, "agc_edges_golden.npz" if edges else "agc_golden.npz")
    if check:
        have = np.load(path)
        bad = sorted(set(have.files) ^ set(data)) + [k for k in data if k in have.files and not (
            have[k].dtype == data[k].dtype and np.array_equal(have[k], data[k]))]
        print("%s: %d arrays regenerated, %d differ" % (os.path.basename(path), len(data), len(bad)))
        if bad:
            raise SystemExit("differing arrays: %r" % bad[:12])
        return
    np.savez_compressed(path, **data)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
