"""Writes tests/golden/hpf_golden.npz from the reference high-pass filter and RMS level compiled in place (DESIGN.md
section 2).  Build container only; the library goes outside the tree:

    R=<reference>/WebRtc_AMP_Port; W=$R/webrtc; A=$W/modules/audio_processing; CA=$W/common_audio
    F="-O2 -fPIC -DWEBRTC_POSIX -DWEBRTC_LINUX -msse2 -I$R"
    for c in copy_set_operations splitting_filter_c resample_by_2; do gcc $F -c $CA/signal_processing/$c.c -o hpf_$c.o; done
    g++ $F -shared tests/golden/hpf_ref_shim.cc $A/processing_component.cc $A/audio_buffer.cc $A/channel_buffer.cc \
        $A/splitting_filter.cc $A/rms_level.cc $CA/audio_util.cc $CA/resampler/push_sinc_resampler.cc \
        $CA/resampler/sinc_resampler.cc $CA/resampler/sinc_resampler_sse.cc $W/base/checks.cc \
        $W/system_wrappers/source/aligned_malloc.cc $W/system_wrappers/source/cpu_features.cc \
        hpf_copy_set_operations.o hpf_splitting_filter_c.o hpf_resample_by_2.o -o libhpf_ref.so
    python tests/golden/make_hpf_golden.py libhpf_ref.so

The runs are tests/hpf_runs.py's.  Per filter run the golden has the input, the output and the six state words
(y[0..3], x[0..1]) after the run's snapshot frames; a float-S16 run's input passes FloatS16ToS16 (audio_util.h) on
its way in and a plain conversion on its way out, as the int16 view of a float buffer does.  Per meter run it has the
input, sum_square_ as its 32 bits and sample_count_ after every frame, and every RMS() return.

Coverage, asserted here with hpf_runs.model's arithmetic, which is first held to the reference's outputs and state:
for each coefficient set the 2^27 clamp fires and the cast to y[0] wraps (the two places a port can go wrong), and no
intermediate leaves int32.  Every stored RMS() is either one of the two early returns or has rms + 0.5 at least 1e-3
from an integer, so that an ulp of log10f between two libm's cannot change it; 127 from silence, 127 from the clamp
and 0 from full scale all occur."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import hpf_runs as R  # noqa: E402

P, IP = C.c_void_p, C.c_int


def load(path):
    L = C.CDLL(path)
    L.hpf_ref_create.restype = P
    L.hpf_ref_create.argtypes = [IP]
    L.hpf_ref_free.argtypes = [P]
    L.hpf_ref_filter.argtypes = [P, P, IP]
    L.hpf_ref_state.argtypes = [P, P]
    L.hpf_ref_coeff_set.argtypes = [P]
    L.hpf_ref_float_s16_to_s16.argtypes = [P, IP, P]
    L.level_ref_create.restype = P
    for n in ("free", "reset", "rms"):
        getattr(L, "level_ref_" + n).argtypes = [P]
    L.level_ref_process.argtypes = [P, P, IP]
    L.level_ref_muted.argtypes = [P, IP]
    L.level_ref_state.argtypes = [P, P, P]
    return L


def float_s16_to_s16(L, x):
    """The reference's FloatS16ToS16 on a float32 array."""
    x = np.ascontiguousarray(x, np.float32)
    d = np.zeros(x.shape, np.int16)
    L.hpf_ref_float_s16_to_s16(x.ctypes.data, x.size, d.ctypes.data)
    return d


class RefFilter:
    def __init__(self, L, rate):
        self.L, self.h = L, C.c_void_p(L.hpf_ref_create(rate))
        assert L.hpf_ref_coeff_set(self.h) == R.coeff_set(rate)

    def process(self, frame):
        is_float = frame.dtype == np.float32
        d = float_s16_to_s16(self.L, frame) if is_float else frame.copy()
        assert self.L.hpf_ref_filter(self.h, d.ctypes.data, len(d)) == 0
        return d.astype(np.float32) if is_float else d

    def state(self):
        st = np.zeros(6, np.int16)
        self.L.hpf_ref_state(self.h, st.ctypes.data)
        return st


class RefMeter:
    def __init__(self, L):
        self.L, self.h = L, C.c_void_p(L.level_ref_create())
        self.margins = []   # (kind of return, distance of rms + 0.5 from an integer)

    def process(self, row):
        row = np.ascontiguousarray(row)
        self.L.level_ref_process(self.h, row.ctypes.data, len(row))

    def muted(self, length):
        self.L.level_ref_muted(self.h, length)

    def state(self):
        s, n = C.c_float(), C.c_int()
        self.L.level_ref_state(self.h, C.byref(s), C.byref(n))
        return np.float32(s.value).view(np.uint32), n.value

    def rms(self):
        bits, count = self.state()
        s = float(np.uint32(bits).view(np.float32))
        if count == 0 or s == 0:
            self.margins.append(("early", 1.0))
        else:
            v = -10 * np.log10(s / (count * 32768.0 * 32768.0))
            if v > 127 + 1e-3:
                self.margins.append(("clamp", 1.0))
            else:
                self.margins.append(("value", abs(v + 0.5 - round(v + 0.5))))
        return self.L.level_ref_rms(self.h)


def main(path):
    L = load(path)
    out = {}
    clamp, wrap = {0: 0, 1: 0}, {0: 0, 1: 0}
    for run in R.FILTER_RUNS:
        name, rate = run[0], run[1]
        x = R.filter_input(run)
        y, snaps = R.replay_filter(run, x, lambda r: RefFilter(L, r))
        xi = float_s16_to_s16(L, x) if x.dtype == np.float32 else x
        ym, sm, cl, wr, ov = R.model(R.coeff_set(rate), xi.reshape(-1))
        last = snaps[x.shape[0] - 1]
        assert np.array_equal(ym, y.reshape(-1).astype(np.int16)) and np.array_equal(sm, last), name
        assert ov == 0, (name, "an intermediate left int32")
        clamp[R.coeff_set(rate)] += cl
        wrap[R.coeff_set(rate)] += wr
        out["f_%s_in" % name] = x
        out["f_%s_out" % name] = y
        for f, st in snaps.items():
            out["f_%s_state%d" % (name, f)] = st
        print("filter", name, x.shape, x.dtype, "clamp", cl, "wrap", wr)
    for s in (0, 1):
        assert clamp[s] > 0 and wrap[s] > 0, (s, clamp, wrap)
    out["clamp_counts"] = np.array([clamp[0], clamp[1]], np.int32)
    out["wrap_counts"] = np.array([wrap[0], wrap[1]], np.int32)
    print("clamp counts", clamp, "wrap counts", wrap)
    kinds, values = set(), set()
    for run in R.METER_RUNS:
        name = run[0]
        x = R.meter_input(run)
        m = RefMeter(L)
        bits, counts, rms = R.replay_meter(run, x, m)
        assert len(rms) == len(m.margins) > 0
        for kind, margin in m.margins:
            assert margin >= 1e-3, (name, kind, margin)
            kinds.add(kind)
        values.update(int(v) for v in rms)
        out["m_%s_in" % name] = x
        out["m_%s_bits" % name] = bits
        out["m_%s_counts" % name] = counts
        out["m_%s_rms" % name] = rms
        print("meter", name, x.shape, "rms", rms.tolist(), "min margin %.4f" % min(mg for _, mg in m.margins),
              "sum past 2^24 in frame 0:", bool(np.uint32(bits[0]).view(np.float32) > 2 ** 24))
    assert kinds == {"early", "clamp", "value"} and {0, 127} <= values, (kinds, values)
    dst = os.path.join(HERE, "hpf_golden.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 1000000


if __name__ == "__main__":
    main(sys.argv[1])
