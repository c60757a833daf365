"""The runs of tests/golden/hpf_golden.npz: what the generator (tests/golden/make_hpf_golden.py) drives the compiled
reference with, and what the host and GPU tests replay.  The golden stores every input, so the tests read the
inputs from it; the functions here make them for the generator.

A filter run: (name, sample rate, frame length n, frames F, kind).  One channel, F frames of n samples through one
FilterState; the state is stored after the frames snapshots(F).  Kinds ending in _f32 go through the float-S16 entry.
A meter run: (name, channels C, samples n, frames F, kind, rms_every, muted_every).  Frame f is ProcessMuted(C * n)
where f % muted_every == muted_every - 1 and Process on channel 0 .. C - 1 otherwise; RMS() follows every
rms_every-th frame.  The accumulator is stored after every frame, before that RMS()."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpf_golden.npz")
NS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ns_golden.npz")

COEFFS = {0: (3798, -7596, 3798, 7807, -3733), 1: (4012, -8024, 4012, 8002, -3913)}

_KINDS = [("speech", 60), ("noise_lo", 20), ("dc", 10), ("square", 20), ("nyquist", 10), ("noise_fs", 20), ("worst", 0),
          ("halves_f32", 10)]
FILTER_RUNS = [("%s_%d" % (kind, rate), rate, n, F, kind) for rate, n in ((8000, 80), (16000, 160)) for kind, F in _KINDS]
FILTER_RUNS.append(("speech_48000", 48000, 160, 12, "speech"))   # band 0 of a 48 kHz stream: the 16 kHz coefficients

METER_RUNS = [
    ("noise_1x80", 1, 80, 24, "noise", 3, 0),
    ("noise_2x160", 2, 160, 24, "noise", 5, 4),
    ("speech_1x160", 1, 160, 40, "speech", 10, 0),
    ("noise_1x320", 1, 320, 12, "noise_lo", 4, 0),
    ("noise_2x480", 2, 480, 12, "noise", 2, 3),
    ("silence_2x160", 2, 160, 6, "silence", 2, 0),
    ("full_scale_1x480", 1, 480, 8, "full_scale", 2, 0),
    ("full_scale_2x480", 2, 480, 6, "square", 3, 5),
    ("lsb_2x480", 2, 480, 50, "lsb", 50, 0),
]


def coeff_set(rate):
    return 0 if rate == 8000 else 1


def snapshots(F):
    return sorted({0, F // 2, F - 1})


def i16(v):
    return ((v + 32768) & 0xffff) - 32768


def i32(v):
    return ((v + 2 ** 31) & 0xffffffff) - 2 ** 31


def model(set_, x):
    """Filter on Python integers with explicit two's-complement wrap: (out, state, samples where the 2^27 clamp
    fires, samples where the cast to y[0] wraps, samples where an intermediate leaves int32)."""
    ba = COEFFS[set_]
    y, xs, out = [0, 0, 0, 0], [0, 0], []
    clamp = wrap = ovf = 0
    for d in map(int, x):
        t = (y[1] * ba[3] + y[3] * ba[4]) >> 15
        t = (t + y[0] * ba[3] + y[2] * ba[4]) << 1
        t += d * ba[0] + xs[0] * ba[1] + xs[1] * ba[2]
        ovf += i32(t) != t
        t = i32(t)
        xs = [d, xs[0]]
        y[2], y[3] = y[0], y[1]
        wrap += i16(t >> 13) != (t >> 13)
        y[0] = i16(t >> 13)
        y[1] = i16(i32(i32(t - i32(y[0] << 13)) << 2))
        t += 2048
        clamp += t > 134217727 or t < -134217728
        out.append(min(134217727, max(-134217728, t)) >> 12)
    return np.array(out, np.int16), np.array(y + xs, np.int16), clamp, wrap, ovf


def worst_case(set_):
    """+-full scale following the sign of the time-reversed 400-tap impulse response, that block negated, the block
    again: drives the filter's output past twice full scale."""
    imp = np.zeros(400, np.int16)
    imp[0] = 16384
    h = model(set_, imp)[0].astype(np.int64)
    x = np.where(h[::-1] >= 0, 32767, -32768)
    return np.concatenate([x, np.clip(-x, -32768, 32767), x]).astype(np.int16)


def _speech(count, offset=16000):
    wav = np.load(NS_GOLDEN)["wav_in_i16"]
    return np.ascontiguousarray(wav[offset:offset + count])


def filter_input(run):
    """int16 [F][n], or float32 [F][n] for a float-S16 run."""
    name, rate, n, F, kind = run
    rng = np.random.default_rng(abs(hash_name(name)))
    if kind == "worst":
        x = worst_case(coeff_set(rate))
        x = np.concatenate([x, np.zeros(-len(x) % n, np.int16)])
        return x.reshape(-1, n)
    t = np.arange(F * n)
    if kind == "speech":
        x = _speech(F * n)
    elif kind == "noise_lo":
        x = rng.integers(-600, 600, F * n)
    elif kind == "dc":
        x = np.full(F * n, 12000)
    elif kind == "square":
        x = np.where((t // 800) % 2 == 0, 32767, -32768)
    elif kind == "nyquist":
        x = np.where(t % 2 == 0, 32767, -32768)
    elif kind == "noise_fs":
        x = rng.integers(-32768, 32768, F * n)
    elif kind == "halves_f32":
        # halves (ties of the rounding), values around the two saturation thresholds, out-of-range values
        x = rng.integers(-40000, 40000, F * n).astype(np.float32) + rng.choice(np.float32([0, 0.5, -0.5, 0.25, 0.49999]), F * n)
        x[:8] = np.float32([32766.5, 32766.49, 32767.0, 1e9, -32767.5, -32767.49, -32768.0, -1e9])
        x[8:12] = np.float32([0.5, -0.5, 0.0, -0.0])
        return x.astype(np.float32).reshape(F, n)
    else:
        raise ValueError(kind)
    return x.astype(np.int16).reshape(F, n)


def hash_name(name):
    import zlib

    return zlib.crc32(name.encode())


def meter_input(run):
    """int16 [F][C][n]"""
    name, C, n, F, kind, _, _ = run
    rng = np.random.default_rng(hash_name(name))
    N = F * C * n
    if kind == "noise":
        x = rng.integers(-9000, 9000, N)
    elif kind == "noise_lo":
        x = rng.integers(-40, 40, N)
    elif kind == "speech":
        x = _speech(N, 30000)
    elif kind == "silence":
        x = np.zeros(N)
    elif kind == "full_scale":
        x = np.full(N, -32768)
    elif kind == "square":
        x = np.where((np.arange(N) // 7) % 2 == 0, 32767, -32768)
    elif kind == "lsb":
        x = np.zeros(N)
        x[5] = 1
    else:
        raise ValueError(kind)
    return x.astype(np.int16).reshape(F, C, n)


def meter_is_muted(run, f):
    m = run[6]
    return bool(m) and f % m == m - 1


def meter_is_rms(run, f):
    return (f + 1) % run[5] == 0


def replay_filter(run, x, make):
    """Drives one filter (make(rate) -> object with process(frame) -> frame, state() -> int16 [6]) frame by frame:
    (out like x, {frame: state})."""
    name, rate, n, F, kind = run
    flt = make(rate)
    y, snaps = np.empty_like(x), {}
    for f in range(x.shape[0]):
        y[f] = flt.process(x[f])
        if f in snapshots(x.shape[0]):
            snaps[f] = flt.state()
    return y, snaps


def replay_meter(run, x, m):
    """Drives one meter (process(row), muted(length), rms() -> int, state() -> (bits, count)):
    (sum bits uint32 [F], counts int32 [F], RMS() returns int32 [F // rms_every])."""
    name, C, n, F = run[:4]
    bits, counts, rms = np.zeros(F, np.uint32), np.zeros(F, np.int32), []
    for f in range(F):
        if meter_is_muted(run, f):
            m.muted(C * n)
        else:
            for c in range(C):
                m.process(x[f, c])
        bits[f], counts[f] = m.state()
        if meter_is_rms(run, f):
            rms.append(m.rms())
    return bits, counts, np.array(rms, np.int32)
