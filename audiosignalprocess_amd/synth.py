"""Deterministic synthetic inputs; numpy only.

These are the generators the bench and the parity tests feed to every engine
(HIP path, CPU restatement, compiled reference) so all of them see identical
float32 frames.
"""
import numpy as np

_A = np.uint32(1664525)
_C = np.uint32(1013904223)


def _lcg_uniform(seeds, t0, count):
    """n[s, k] for absolute sample indices t0 .. t0+count-1 of each stream.

    u <- u*1664525 + 1013904223 (mod 2**32) once per sample, seeded per
    stream; n = ((u >> 16) - 32768) / 32768 in [-1, 1).
    """
    seeds = np.asarray(seeds, dtype=np.uint32)
    total = t0 + count
    with np.errstate(over="ignore"):
        a_pow = np.cumprod(np.full(total, _A, dtype=np.uint32), dtype=np.uint32)  # a^(t+1)
        geo = np.cumsum(np.concatenate(([np.uint32(1)], a_pow[:-1])), dtype=np.uint32)
        c_t = (_C * geo).astype(np.uint32)  # c * (a^t + ... + 1)
        u = seeds[:, None] * a_pow[None, t0:] + c_t[None, t0:]
    u = u.astype(np.uint32)
    return ((u >> np.uint32(16)).astype(np.float64) - 32768.0) / 32768.0


def ns_frames(num_streams, num_frames, stream0=0, frame0=0):
    """NS input, float-S16 units, shape [num_frames][num_streams][160] float32.

    x = 600 n + g(f) 3000 sin(2 pi (300 + 5 (s mod 64)) t / 16000) (0.5 + 0.5 sin(0.01 f)),
    g(f) = 1 when floor(f/100) is odd else 0; never all-zero.
    """
    s = np.arange(stream0, stream0 + num_streams, dtype=np.int64)
    seeds = (12345 + 7919 * s) & 0xFFFFFFFF
    n = _lcg_uniform(seeds, 160 * frame0, 160 * num_frames)  # [S][T]
    t = np.arange(160 * frame0, 160 * (frame0 + num_frames), dtype=np.float64)
    f = np.floor(t / 160.0)
    g = ((np.floor(f / 100.0).astype(np.int64) & 1) == 1).astype(np.float64)
    freq = 300.0 + 5.0 * (s % 64).astype(np.float64)
    tone = np.sin(2.0 * np.pi * freq[:, None] * t[None, :] / 16000.0)
    env = g * 3000.0 * (0.5 + 0.5 * np.sin(0.01 * f))
    x = 600.0 * n + tone * env[None, :]
    x = x.astype(np.float32).reshape(num_streams, num_frames, 160)
    return np.ascontiguousarray(x.transpose(1, 0, 2))


def bt_samples(num_streams, num_samples, stream0=0, t0=0):
    """BlockThresholding input, float in [-1, 1], shape [num_streams][num_samples] float32.

    0.2 sin(0.02 t (1 + 0.1 (s mod 16))) (1 if floor(t/20000) odd else 0.1) + 0.08 n
    (SURVEY.md section 8(d)); never an all-zero macroblock (the reference divides by the
    block energy, audioDenoiseBlockTreshold.c:397-398).
    """
    s = np.arange(stream0, stream0 + num_streams, dtype=np.int64)
    seeds = (12345 + 7919 * s) & 0xFFFFFFFF
    n = _lcg_uniform(seeds, t0, num_samples)
    t = np.arange(t0, t0 + num_samples, dtype=np.float64)
    gate = np.where((np.floor(t / 20000.0).astype(np.int64) & 1) == 1, 1.0, 0.1)
    w = 0.02 * (1.0 + 0.1 * (s % 16).astype(np.float64))
    x = 0.2 * np.sin(w[:, None] * t[None, :]) * gate[None, :] + 0.08 * n
    return np.ascontiguousarray(x.astype(np.float32))


def aec_frames(num_streams, num_frames, stream0=0):
    """AEC input (far, near), float-S16 units, each [num_frames][num_streams][160] float32.

    far = A(f) n_far, A = 4000 when floor(f/150) is odd else 40;
    near = 0.5 far[t-40-(s mod 16)] + 0.25 far[t-90] + 100 n_near
           (+ 1500 sin(0.05 t) when floor(f/200) mod 3 == 2)        (SURVEY.md section 8(d)).
    """
    s = np.arange(stream0, stream0 + num_streams, dtype=np.int64)
    T = 160 * num_frames
    n_far = _lcg_uniform((12345 + 7919 * s) & 0xFFFFFFFF, 0, T)
    n_near = _lcg_uniform((987654321 + 104729 * s) & 0xFFFFFFFF, 0, T)
    t = np.arange(T, dtype=np.float64)
    f = np.floor(t / 160.0).astype(np.int64)
    amp = np.where((f // 150) % 2 == 1, 4000.0, 40.0)
    far = n_far * amp[None, :]
    near = 100.0 * n_near
    for k in range(num_streams):
        d1 = 40 + int(s[k] % 16)
        near[k, d1:] += 0.5 * far[k, :-d1]
        near[k, 90:] += 0.25 * far[k, :-90]
    talk = ((f // 200) % 3 == 2)
    near += (1500.0 * np.sin(0.05 * t) * talk)[None, :]

    def shape(a):
        return np.ascontiguousarray(a.astype(np.float32).reshape(num_streams, num_frames, 160).transpose(1, 0, 2))

    return shape(far), shape(near)


def _lcg_u32(seeds, t0, count):
    """The raw uint32 LCG words of _lcg_uniform (same recurrence), integer only: [S][count] uint32."""
    seeds = np.asarray(seeds, dtype=np.uint32)
    total = t0 + count
    with np.errstate(over="ignore"):
        a_pow = np.cumprod(np.full(total, _A, dtype=np.uint32), dtype=np.uint32)
        geo = np.cumsum(np.concatenate(([np.uint32(1)], a_pow[:-1])), dtype=np.uint32)
        c_t = (_C * geo).astype(np.uint32)
        u = seeds[:, None] * a_pow[None, t0:] + c_t[None, t0:]
    return u.astype(np.uint32)


def vad_frames(num_streams, num_frames, fs, frame_ms, seed=0, stream0=0, frame0=0):
    """VAD input, int16 [num_frames][num_streams][fs * frame_ms / 1000]; integer arithmetic only, so the
    samples do not depend on the numpy version or on float rounding.

    Per stream s and 10 ms block b (absolute block index, frame0 counted in frames of frame_ms):
    a voiced burst (triangle of period fs / (110 + 13 (s mod 8)) plus noise, amplitude 1500..9000)
    while ((b + 17 s) mod (60 + 4 (s mod 5))) < 25, else a noise floor of +-(24 .. 87); every 97th
    block is all but silent (+-1), so the low-energy branch of the model is reached too.
    """
    L = fs * frame_ms // 1000
    s = np.arange(stream0, stream0 + num_streams, dtype=np.int64)
    seeds = ((12345 + 7919 * (s + 1000003 * seed)) & 0xFFFFFFFF).astype(np.uint32)
    T = L * num_frames
    t0 = L * frame0
    u = _lcg_u32(seeds, t0, T).astype(np.int64)
    n = (u >> 16) - 32768                                       # [-32768, 32767]
    t = np.arange(t0, t0 + T, dtype=np.int64)[None, :]
    b = t // (fs // 100)                                        # 10 ms block
    period = (fs // (110 + 13 * (s % 8)))[:, None]
    ph = t % period
    tri = (np.abs(2 * 65536 * ph // period - 65536) - 32768)   # [-32768, 32768]
    talk = ((b + 17 * s[:, None]) % (60 + 4 * (s[:, None] % 5))) < 25
    amp = 1500 + ((b * 37 + 11 * s[:, None]) % 16) * 500
    floor = 24 + (s[:, None] % 64)
    voiced = (tri * amp) // 32768 + (n * (amp // 4)) // 32768
    quiet = (n * floor) // 32768
    hush = (b % 97) == 5
    x = np.where(talk, voiced, quiet)
    x = np.where(hush, (n >> 15), x)
    x = np.clip(x, -32768, 32767).astype(np.int16)
    return np.ascontiguousarray(x.reshape(num_streams, num_frames, L).transpose(1, 0, 2))


def aecm_pair(num_streams, num_frames, n, delay=40, seed=0, stream0=0):
    """AECM input, three int16 arrays [num_frames][num_streams][n]: far, near, clean.  Integer only.

    Far: a talker (triangle of period 57 + 7 (s mod 5) samples plus noise, amplitude 2000..7000) while
    ((b + 13 s) mod 90) < 55 (b: absolute 80-sample block), else a noise floor.  Near: far delayed by
    `delay` + (s mod 7) samples through the echo path (x[t] / 2 - x[t - 3] / 8 + x[t - 9] / 16), plus
    near-end talk (a second triangle) while ((b + 29 s) mod 150) >= 120 -- the double-talk segments --
    plus noise.  Clean: near without its noise.
    """
    L = n * num_frames
    s = np.arange(stream0, stream0 + num_streams, dtype=np.int64)
    seeds = ((777 + 104729 * (s + 1000003 * seed)) & 0xFFFFFFFF).astype(np.uint32)
    pad = delay + 6 + 9
    u = _lcg_u32(seeds, 0, L + pad).astype(np.int64)
    nz = (u >> 16) - 32768
    t = np.arange(-pad, L, dtype=np.int64)[None, :]
    b = np.maximum(t, 0) // 80
    period = (57 + 7 * (s % 5))[:, None]
    tri = np.abs(2 * 65536 * (t % period) // period - 65536) - 32768
    amp = 2000 + ((b * 29 + 5 * s[:, None]) % 11) * 500
    talk = ((b + 13 * s[:, None]) % 90) < 55
    far = np.where(talk, (tri * amp) // 32768 + (nz * (amp // 8)) // 32768, (nz * 40) // 32768)
    far = np.where(t < 0, 0, far)
    d = delay + (s % 7)
    idx = np.arange(L)[None, :] + pad
    g = lambda k: np.take_along_axis(far, idx - d[:, None] - k, axis=1)
    echo = g(0) // 2 - g(3) // 8 + g(9) // 16
    tn = np.arange(L, dtype=np.int64)[None, :]
    bn = tn // 80
    period2 = (41 + 5 * (s % 3))[:, None]
    tri2 = np.abs(2 * 65536 * (tn % period2) // period2 - 65536) - 32768
    dt = ((bn + 29 * s[:, None]) % 150) >= 120
    clean = echo + np.where(dt, (tri2 * 3000) // 32768, 0)
    noise = (nz[:, pad:] * 60) // 32768
    near = clean + noise
    far = far[:, pad:]

    def shape(x):
        x = np.clip(x, -32768, 32767).astype(np.int16)
        return np.ascontiguousarray(x.reshape(num_streams, num_frames, n).transpose(1, 0, 2))

    return shape(far), shape(near), shape(clean)


def nsx_frames(num_streams, num_frames, n, num_bands=1, seed=0, stream0=0, level=800):
    """NSX input, int16 [num_frames][num_bands][num_streams][n].  Integer only, regenerable from its arguments.

    Band 0: noise of amplitude `level` (from the LCG) plus speech-like bursts: a triangle of period
    41 + 6 (s mod 5) samples, amplitude 3000..9000, on while ((f + 11 s) mod 70) < 30 (f: frame).
    Higher bands: noise of amplitude level / 2 with a fainter copy of the bursts.
    """
    L = n * num_frames
    s = np.arange(stream0, stream0 + num_streams, dtype=np.int64)
    out = np.zeros((num_frames, num_bands, num_streams, n), np.int16)
    t = np.arange(L, dtype=np.int64)[None, :]
    f = t // n
    period = (41 + 6 * (s % 5))[:, None]
    tri = np.abs(2 * 65536 * (t % period) // period - 65536) - 32768
    amp = 3000 + ((f * 17 + 3 * s[:, None]) % 13) * 500
    on = ((f + 11 * s[:, None]) % 70) < 30
    for b in range(num_bands):
        seeds = ((4242 + 104729 * (s + 1000003 * seed) + 7919 * b) & 0xFFFFFFFF).astype(np.uint32)
        nz = (_lcg_u32(seeds, 0, L).astype(np.int64) >> 16) - 32768
        lev = level if b == 0 else level // 2
        x = (nz * lev) // 32768 + np.where(on, (tri * amp) // 32768, 0) // (1 if b == 0 else 8 * b)
        out[:, b] = np.clip(x, -32768, 32767).astype(np.int16).reshape(num_streams, num_frames, n).transpose(1, 0, 2)
    return out


def agc_frames(num_streams, num_frames, n, num_bands=1, seed=0, stream0=0, level=8000, shift=0, gaps=True):
    """AGC input, int16 [num_frames][num_bands][num_streams][n].  Integer only, regenerable from its arguments.

    Speech-like and amplitude-modulated, since a steady noise does not move the analog loop.  Frame f of
    stream s is at position p = (f + shift + 37 s) mod 300 of a programme: p < 80 talk at `level`; p < 110 a
    noise floor of amplitude 30; p < 190 talk at level / 16; p < 250 all zero; else talk at 6 x level, which
    clips.  gaps=False: talk at `level` instead of the all-zero stretch (a long silence holds the analog loop's
    upward steps back for eight seconds).  Talk: a triangle of period 53 + 6 (s mod 5) samples whose amplitude follows a syllable pattern
    over the frames (0 .. 4 quarters of the level), plus noise at an eighth of it.  The far end of a run is
    band 0 of another seed.  Higher bands: an eighth of band 0's talk plus their own noise.
    """
    L = n * num_frames
    s = np.arange(stream0, stream0 + num_streams, dtype=np.int64)
    out = np.zeros((num_frames, num_bands, num_streams, n), np.int16)
    t = np.arange(L, dtype=np.int64)[None, :]
    f = t // n
    p = (f + shift + 37 * s[:, None]) % 300
    period = (53 + 6 * (s % 5))[:, None]
    tri = np.abs(2 * 65536 * (t % period) // period - 65536) - 32768
    syll = ((f * 7 + 3 * s[:, None]) // 3) % 5
    amp = np.where((p < 80) | ((p >= 190) & (p < 250) & (not gaps)), level, np.where((p >= 110) & (p < 190), level // 16, np.where(p >= 250, 6 * level, 0)))
    amp = amp * syll // 4
    for b in range(num_bands):
        seeds = ((9091 + 104729 * (s + 1000003 * seed) + 7919 * b) & 0xFFFFFFFF).astype(np.uint32)
        nz = (_lcg_u32(seeds, 0, L).astype(np.int64) >> 16) - 32768
        talk = (tri * amp) // 32768 // (1 if b == 0 else 8) + (nz * (amp // 8)) // 32768
        x = np.where((p >= 80) & (p < 110), (nz * 30) // 32768, talk)
        x = np.where((p >= 190) & (p < 250) & gaps, 0, x)
        out[:, b] = np.clip(x, -32768, 32767).astype(np.int16).reshape(num_streams, num_frames, n).transpose(1, 0, 2)
    return out


def ts_chunks(num_streams, num_chunks, rate, channels=1, seed=0, stream0=0, click_every=7, level=700):
    """Transient-suppressor input in float-S16 units: (data float32 [F][S][C][L], reference float32 [F][S][L]),
    L = rate / 100.  Integer-valued samples, LCG noise and rational arithmetic only (no libm).

    Channel c of stream s: level * n + 4 * level * e(f) * (m(t) + m(t-1) + m(t-2) + m(t-3)) / 4 with n, m two
    LCG noises and e(f) a syllable envelope (0, 1/2, 1, 1/2 over four chunks, off every other 16 chunks), plus
    a click every click_every chunks: amplitude 2000 * (1 + (k mod 6)) for the k-th click, alternating sign,
    halving over six samples, a quarter of the way into the chunk.  The reference channel holds the clicks
    alone (all zero in a chunk without one)."""
    L = rate // 100
    T = L * num_chunks
    s = np.arange(stream0, stream0 + num_streams, dtype=np.int64)
    f = np.arange(T) // L
    env = np.array([0.0, 0.5, 1.0, 0.5])[f % 4] * ((f // 16) % 2 == 0)
    click = np.zeros(T)
    for k, c in enumerate(range(click_every // 2, num_chunks, click_every)):
        a = 2000.0 * (1 + k % 6) * (1 if k % 2 == 0 else -1)
        for j in range(6):
            click[c * L + L // 4 + j] = a / (1 << j) * (1 if j % 2 == 0 else -1)
    data = np.empty((num_streams, channels, T))
    for c in range(channels):
        n = _lcg_uniform((777 + 31 * seed + 7919 * s + 104729 * c) & 0xFFFFFFFF, 0, T)
        m = _lcg_uniform((4242 + 17 * seed + 6007 * s + 15485863 * c) & 0xFFFFFFFF, 0, T + 3)
        lp = (m[:, 3:] + m[:, 2:-1] + m[:, 1:-2] + m[:, :-3]) / 4.0
        data[:, c] = np.rint(level * n + 4.0 * level * env[None, :] * lp + click[None, :])
    data = data.astype(np.float32).reshape(num_streams, channels, num_chunks, L)
    ref = np.broadcast_to(click.astype(np.float32).reshape(1, num_chunks, L), (num_streams, num_chunks, L))
    return np.ascontiguousarray(data.transpose(2, 0, 1, 3)), np.ascontiguousarray(ref.transpose(1, 0, 2))


def bf_chunks(num_streams, num_chunks, num_mics, seed=0, stream0=0, delay=2, level=3000, diffuse=60,
              broadside=((0, 20), (70, 80)), offaxis=((24, 70),), silent=((20, 24),)):
    """Microphone-array input for the beamformer in float-S16 units at the 16 kHz band rate: (input float32
    [F][S][M][160], high band float32 [F][S][M][160]).  Integer-valued samples, LCG noise only (no libm).

    Microphone c of stream s: a broadside source (the same low-passed noise on every microphone) during the chunk
    ranges `broadside`, an off-axis source (another low-passed noise, delayed by c * delay samples) during
    `offaxis`, and diffuse noise (independent per microphone, amplitude `diffuse`) everywhere except the ranges
    `silent`, where every microphone is exactly zero.  The high band is the sources' sum at a quarter of the level
    with its own per-microphone noise, silent in the same ranges."""
    L = 160
    T = L * num_chunks
    s = np.arange(stream0, stream0 + num_streams, dtype=np.int64)
    f = np.arange(T) // L

    def gate(ranges):
        g = np.zeros(T)
        for a, b in ranges:
            g[(f >= a) & (f < b)] = 1.0
        return g

    def lowpassed(salt, extra):
        m = _lcg_uniform((salt + 97 * seed + 7919 * s) & 0xFFFFFFFF, 0, T + 3 + extra)
        return (m[:, 3:] + m[:, 2:-1] + m[:, 1:-2] + m[:, :-3]) / 4.0

    pad = delay * (num_mics - 1)
    b = lowpassed(1357, 0) * gate(broadside)[None]
    o = lowpassed(8642, pad)   # o[:, pad + t - c * delay] is the source at microphone c
    live = 1.0 - gate(silent)
    x = np.empty((num_streams, num_mics, T))
    hi = np.empty((num_streams, num_mics, T))
    for c in range(num_mics):
        oc = o[:, pad - c * delay:pad - c * delay + T] * gate(offaxis)[None]
        n = _lcg_uniform((2468 + 13 * seed + 6007 * s + 15485863 * c) & 0xFFFFFFFF, 0, T)
        h = _lcg_uniform((9753 + 29 * seed + 104729 * s + 32452843 * c) & 0xFFFFFFFF, 0, T)
        x[:, c] = np.rint((level * (b + oc) + diffuse * n) * live[None])
        hi[:, c] = np.rint((0.25 * level * (b + oc) + diffuse * h) * live[None])
    shape = (num_streams, num_mics, num_chunks, L)
    return (np.ascontiguousarray(x.astype(np.float32).reshape(shape).transpose(2, 0, 1, 3)),
            np.ascontiguousarray(hi.astype(np.float32).reshape(shape).transpose(2, 0, 1, 3)))
