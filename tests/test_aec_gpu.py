"""GPU parity tests of the batched echo canceller (through the C-ABI, include/asp_aec.h).

Chain of evidence: reference build == oracle/aec_oracle.c bit for bit (tests/test_aec_oracle.py);
here the HIP path is compared with that oracle on the same inputs and with the committed
reference outputs tests/golden/aec_golden.npz.  The FFT, the adaptive filter, the PSD / coherence
state and the control plane are bit-exact; the NLP output goes through powf / cosf / sinf, which
the device evaluates in fp64 and rounds (glibc's float versions are not correctly rounded in rare
last-place cases), so output and NLP-dependent comparisons carry the tolerance stated in each
test."""
import ctypes as C
import os

import numpy as np
import pytest

from audiosignalprocess_amd._abi import aec_state_arrays
from audiosignalprocess_amd.synth import aec_frames
from tests import oracle_lib
from tests.oracle_lib import OracleAec

from tests.conftest import parity_note

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def aec():
    from audiosignalprocess_amd import aec as mod
    from audiosignalprocess_amd import ns

    assert ns.device_count() >= 1, "GPU tests need a HIP device"
    return mod


@pytest.fixture(scope="module")
def aec_golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "aec_golden.npz")))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30)


def test_rdft128_bit_exact(aec):
    rng = np.random.default_rng(5)
    x = np.concatenate([np.sin(np.arange(128, dtype=np.float32))[None], np.eye(1, 128, 0, dtype=np.float32),
                        np.ones((1, 128), np.float32), np.zeros((1, 128), np.float32),
                        (rng.standard_normal((61, 128)) * 4000).astype(np.float32)])
    for isgn in (1, -1):
        got = aec.rdft128(x, isgn)
        want = oracle_lib.aec_oracle_rdft128(x, isgn)
        assert np.array_equal(_bits(got), _bits(want)), isgn


def _state_report(sa, sb):
    """max |diff| per field relative to the field's scale, plus exact equality flags."""
    da, db = aec_state_arrays(sa), aec_state_arrays(sb)
    rep = {}
    for k in da:
        if isinstance(da[k], np.ndarray):
            scale = max(np.abs(db[k]).max(), 1e-30)
            rep[k] = (bool(np.array_equal(_bits(da[k]), _bits(db[k]))), float(np.abs(da[k] - db[k]).max() / scale))
        else:
            rep[k] = (da[k] == db[k], float(abs(float(da[k]) - float(db[k]))))
    return rep


# fields that never see the NLP's transcendental functions: must be bit-exact
LINEAR_FIELDS = ["dBuf", "eBuf", "xPow", "dPow", "dMinPow", "dInitMinPow", "xfBuf", "wfBuf", "sde", "sxd",
                 "xfwBuf", "sx", "sd", "se", "hNlFbMin", "hNlFbLocalMin", "hNlXdAvgMin",
                 "hNlNewMin", "hNlMinCtr", "delayIdx", "stNearState", "echoState", "divergeState",
                 "xfBufBlockPos", "noiseEstCtr", "delayEstCtr", "seed"]


@pytest.mark.parametrize("fs,n,nlp", [(16000, 160, 1), (16000, 80, 2), (8000, 80, 0)])
def test_free_running_vs_oracle(aec, fs, n, nlp):
    """8 streams x 600 frames, delay changes included: control plane equal, linear state bit-exact,
    outputs within 1e-5 per-stream rel-L2 of the oracle (measured ~1e-8: only powf/cosf/sinf last
    places differ)."""
    S, F = 8, 600
    far, near = aec_frames(S, F if n == 160 else F // 2)
    far = far.reshape(-1, S, 160 // n, n).transpose(0, 2, 1, 3).reshape(-1, S, n)[:F]
    near = near.reshape(-1, S, 160 // n, n).transpose(0, 2, 1, 3).reshape(-1, S, n)[:F]
    g = aec.AecBatch(S, fs, nlp_mode=nlp)
    oras = [OracleAec(fs, nlp_mode=nlp) for _ in range(S)]
    out_g = np.empty((F, S, n), np.float32)
    out_o = np.empty((F, S, n), np.float32)
    for f in range(F):
        d = 0
        if f in (200, 201):
            d = 700
        if f == 250:
            d = -5
        if 300 <= f < 380:
            d = 60
        out_g[f], rc_g = g.frame(far[f], near[f], d)
        for s in range(S):
            out_o[f, s], rc_o = oras[s].frame(far[f, s], near[f, s], d)
        assert rc_g == rc_o, f
        if f % 100 == 99:
            cg = g.control()
            _, co = oras[0].export()
            for name, _t in cg._fields_:
                assert getattr(cg, name) == getattr(co, name), (f, name)
    for s in range(S):
        st_o, _ = oras[s].export()
        rep = _state_report(g.export_state(s), st_o)
        bad = [k for k in LINEAR_FIELDS if not rep[k][0]]
        assert bad == [], (s, {k: rep[k] for k in bad})
        assert rep["outBuf"][1] <= 1e-5 and rep["overDrive"][1] <= 1e-6 and rep["overDriveSm"][1] <= 1e-6
        assert _rel_l2(out_g[:, s], out_o[:, s]) <= 1e-5, s
    frac_exact = (_bits(out_g) == _bits(out_o)).mean()
    parity_note("AEC fs=%d n=%d: %.4f of output samples bit-equal to the oracle, worst rel-L2 %.2e"
          % (fs, n, frac_exact, max(_rel_l2(out_g[:, s], out_o[:, s]) for s in range(S))))
    assert frac_exact > 0.9


@pytest.mark.parametrize("fs,n,nlp", [(16000, 160, 1), (16000, 80, 2), (8000, 80, 0)])
def test_extended_filter_vs_oracle(aec, fs, n, nlp):
    """AspAecBatch_enable_delay_correction(b, 1): the extended filter (32 partitions, kExtendedMu, the extended
    smoothing coefficients and overdrive floors, no divergence reset) and the ProcessExtended /
    EstBufDelayExtended control plane (aec_core.c:172-174, 337-338, 383, 872-873, 1876-1881;
    echo_cancellation.c:744-814, 869-922) against the oracle (== reference build, tests/test_aec_oracle.py):
    return codes and control plane equal, linear state over all 32 partitions bit-exact, outputs within 1e-5
    per-stream rel-L2; then switched off again mid-stream (back to 12 partitions, state carried over)."""
    S, F = 6, 460
    far, near = aec_frames(S, F if n == 160 else F // 2)
    far = far.reshape(-1, S, 160 // n, n).transpose(0, 2, 1, 3).reshape(-1, S, n)[:F]
    near = near.reshape(-1, S, 160 // n, n).transpose(0, 2, 1, 3).reshape(-1, S, n)[:F]
    g = aec.AecBatch(S, fs, nlp_mode=nlp)
    assert g.delay_correction_enabled() == 0
    g.enable_delay_correction(1)
    assert g.delay_correction_enabled() == 1
    oras = [OracleAec(fs, nlp_mode=nlp) for _ in range(S)]
    for o in oras:
        o.enable_delay_correction(1)
    out_g = np.empty((F, S, n), np.float32)
    out_o = np.empty((F, S, n), np.float32)

    def delay(f):
        if f in (150, 151):
            return 700       # >= kMaxTrustedDelayMs: replaced by kFixedDelayMs (ec:766-768)
        if f == 200:
            return -5
        if 250 <= f < 330:
            return 180       # a sustained change: EstBufDelayExtended moves knownDelay
        return 5 if f >= 400 else 30   # 5: below kMinTrustedDelayMs

    def compare(f):
        cg = g.control()
        _, co = oras[0].export()
        for name, _t in cg._fields_:
            assert getattr(cg, name) == getattr(co, name), (f, name)
        for s in range(S):
            st_o, _ = oras[s].export()
            rep = _state_report(g.export_state(s), st_o)
            bad = [k for k in LINEAR_FIELDS if not rep[k][0]]
            assert bad == [], (f, s, {k: rep[k] for k in bad})
            assert rep["outBuf"][1] <= 1e-5 and rep["overDrive"][1] <= 1e-6 and rep["overDriveSm"][1] <= 1e-6

    for f in range(F):
        out_g[f], rc_g = g.frame(far[f], near[f], delay(f))
        for s in range(S):
            out_o[f, s], rc_o = oras[s].frame(far[f, s], near[f, s], delay(f))
        assert rc_g == rc_o, f
        if f % 115 == 114:
            compare(f)
    compare(F)
    worst = max(_rel_l2(out_g[:, s], out_o[:, s]) for s in range(S))
    frac_exact = (_bits(out_g) == _bits(out_o)).mean()
    parity_note("AEC extended fs=%d n=%d: %.4f of output samples bit-equal to the oracle, worst rel-L2 %.2e" % (fs, n, frac_exact, worst))
    assert worst <= 1e-5 and frac_exact > 0.9
    assert np.abs(aec_state_arrays(g.export_state(0))["wfBuf"].reshape(2, 32 * 65)[:, 12 * 65:]).max() > 0   # the long filter is live
    # off again, mid-stream (legal where xfBufBlockPos lies inside the short filter, as in the reference): the
    # 12-partition path then reads the 32-deep far-spectrum history the extended run left, delayIdx included
    k = 0
    while g.export_state(0).xfBufBlockPos >= 12:
        _, rc_g = g.frame(far[k], near[k], 30)
        for s in range(S):
            _, rc_o = oras[s].frame(far[k, s], near[k, s], 30)
        k += 1
    g.enable_delay_correction(0)
    for o in oras:
        o.enable_delay_correction(0)
    for f in range(k, k + 60):
        og, rc_g = g.frame(far[f], near[f], 30)
        for s in range(S):
            oo, rc_o = oras[s].frame(far[f, s], near[f, s], 30)
            assert rc_g == rc_o and _rel_l2(og[s], oo) <= 1e-5, (f, s)
    for s in range(S):   # partitions 12..31 of xfBuf / wfBuf stay (stale) in the reference; the device drops them
        st_o, _ = oras[s].export()
        da, db = aec_state_arrays(g.export_state(s)), aec_state_arrays(st_o)
        for name in ("xfBuf", "wfBuf"):
            assert np.array_equal(_bits(da[name].reshape(2, 32 * 65)[:, :12 * 65]), _bits(db[name].reshape(2, 32 * 65)[:, :12 * 65])), (s, name)
        for name in ("xfwBuf", "sd", "se", "sx", "sde", "sxd", "xPow", "dPow", "delayIdx", "xfBufBlockPos", "seed"):
            assert np.array_equal(_bits(np.asarray(da[name], np.float32)) if isinstance(da[name], np.ndarray) else da[name],
                                  _bits(np.asarray(db[name], np.float32)) if isinstance(db[name], np.ndarray) else db[name]), (s, name)


def test_extended_filter_golden_and_layer1(aec):
    """The reference's own extended-filter outputs (tests/golden/aec_ext_golden.npz, written by the reference
    build): batch path and the per-stream WebRtcAec_enable_delay_correction(WebRtcAec_aec_core(h), 1) path,
    <= 1e-5 per-stream rel-L2 (bar 1e-4); Init switches the mode off again (aec_core.c:1522-1523)."""
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "aec_ext_golden.npz")))
    far, near = gold["far_i16"].astype(np.float32), gold["near_i16"].astype(np.float32)
    F, S = far.shape[:2]
    d = int(gold["delay_ms"])
    g = aec.AecBatch(S, 16000)
    g.enable_delay_correction(1)
    out = g.run(far, near, d)
    for s in range(S):
        assert _rel_l2(out[:, s], gold["out_f32"][:, s]) <= 1e-5, s
    lib = g.lib
    f32p = C.POINTER(C.c_float)
    lib.WebRtcAec_Create.argtypes = [C.POINTER(C.c_void_p)]
    lib.WebRtcAec_Init.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.WebRtcAec_BufferFarend.argtypes = [C.c_void_p, f32p, C.c_int16]
    lib.WebRtcAec_Process.argtypes = [C.c_void_p, C.POINTER(f32p), C.c_int, C.POINTER(f32p), C.c_int16,
                                      C.c_int16, C.c_int32]
    lib.WebRtcAec_Free.argtypes = [C.c_void_p]
    lib.WebRtcAec_aec_core.restype = C.c_void_p
    lib.WebRtcAec_aec_core.argtypes = [C.c_void_p]
    lib.WebRtcAec_enable_delay_correction.restype = None
    lib.WebRtcAec_enable_delay_correction.argtypes = [C.c_void_p, C.c_int]
    lib.WebRtcAec_delay_correction_enabled.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert lib.WebRtcAec_Create(C.byref(h)) == 0 and lib.WebRtcAec_Init(h, 16000, 48000) == 0
    core = lib.WebRtcAec_aec_core(h)
    assert lib.WebRtcAec_delay_correction_enabled(core) == 0
    lib.WebRtcAec_enable_delay_correction(core, 1)
    assert lib.WebRtcAec_delay_correction_enabled(core) == 1
    F1 = 200
    got = np.empty((F1, 160), np.float32)
    for f in range(F1):
        fr = np.ascontiguousarray(far[f, 2])
        nr = np.ascontiguousarray(near[f, 2])
        assert lib.WebRtcAec_BufferFarend(h, fr.ctypes.data_as(C.POINTER(C.c_float)), 160) == 0
        o = np.empty(160, np.float32)
        pin = (C.POINTER(C.c_float) * 1)(nr.ctypes.data_as(C.POINTER(C.c_float)))
        pout = (C.POINTER(C.c_float) * 1)(o.ctypes.data_as(C.POINTER(C.c_float)))
        assert lib.WebRtcAec_Process(h, pin, 1, pout, 160, d, 0) == 0
        got[f] = o
    assert _rel_l2(got, gold["out_f32"][:F1, 2]) <= 1e-5
    assert lib.WebRtcAec_Init(h, 16000, 48000) == 0 and lib.WebRtcAec_delay_correction_enabled(core) == 0
    assert lib.WebRtcAec_Free(h) == 0


def _lagged_frames(S, F, lags):
    """far / near [F][S][160] of the generator with stream s's near end (echo included) lags[s] x 10 ms late"""
    L = max(lags)
    far, near = aec_frames(S, F + L)
    far_o, near_o = np.empty((F, S, 160), np.float32), np.empty((F, S, 160), np.float32)
    for s in range(S):
        far_o[:, s] = far[lags[s]:lags[s] + F, s]
        near_o[:, s] = near[:F, s]
    return far_o, near_o


@pytest.mark.parametrize("fs,ext", [(16000, 0), (8000, 0), (16000, 1)])
def test_delay_logging_vs_oracle(aec, fs, ext):
    """set_config(delay_logging = kAecTrue): the block-wise binary-spectrum delay estimator (aec_delay_kernel) against
    the oracle (== reference build, tests/test_aec_oracle.py): the estimator's whole state bit for bit -- thresholds,
    binary histories, smoothed bit counts, validation histogram, scalars -- the logging histogram and
    WebRtcAec_GetDelayMetrics of every stream; the audio path is not touched by it."""
    S, F = 6, 420
    n = 160 if fs == 16000 else 80
    far, near = _lagged_frames(S, F, [6, 0, 9, 3, 6, 12])
    far, near = far[:, :, :n], near[:, :, :n]
    g = aec.AecBatch(S, fs)
    rc, _, _ = g.delay_metrics()
    assert rc == -1 and g.error_code() == 12001          # logging disabled
    assert g.set_config(1, delay_logging=1) == 0
    oras = [OracleAec(fs) for _ in range(S)]
    for o in oras:
        assert o.set_nlp(1, delay_logging=1) == 0
    if ext:
        g.enable_delay_correction(1)
        for o in oras:
            o.enable_delay_correction(1)
    seen = []
    for f in range(F):
        og, rc_g = g.frame(far[f], near[f], 20)
        for s in range(S):
            oo, rc_o = oras[s].frame(far[f, s], near[f, s], 20)
            assert rc_g == rc_o and _rel_l2(og[s], oo) <= 1e-5, (f, s)
        if f % 60 == 59 or f == F - 1:
            for s in range(S):
                assert g.delay_state(s).diff(oras[s].delay_state()) == [], (f, s)
        if f % 140 == 139:
            rc, med, std = g.delay_metrics()
            assert rc == 0
            for s in range(S):
                assert (0, int(med[s]), int(std[s])) == oras[s].delay_metrics(), (f, s)
            seen.append(med.copy())
    assert any((m >= 0).any() for m in seen), seen


@pytest.mark.parametrize("fs,n,ext", [(16000, 160, 0), (8000, 80, 0), (16000, 160, 1)])
def test_delay_agnostic_mode_vs_oracle(aec, fs, n, ext):
    """AspAecBatch_enable_reported_delay(b, 0) + delay logging: every stream's far-end read pointer follows its OWN
    delay estimate (SignalBasedDelayCorrection, aec_core.c:797-850, 1719-1751), so the streams of one batch move apart
    -- different echo-path delays per stream here.  Against one oracle per stream (== reference build): outputs
    <= 1e-5 rel-L2, linear state bit-exact, and the per-stream estimator / far-buffer / system-delay state bit for
    bit, through corrections in both directions and an under-run guard."""
    S, F = 6, 520
    lags = [9, 0, 14, 5, 9, 2]
    far, near = _lagged_frames(S, F, lags)
    far, near = far[:, :, :n], near[:, :, :n]
    g = aec.AecBatch(S, fs)
    assert g.set_config(1, delay_logging=1) == 0
    g.enable_reported_delay(0)
    oras = [OracleAec(fs) for _ in range(S)]
    for o in oras:
        assert o.set_nlp(1, delay_logging=1) == 0
        o.enable_reported_delay(0)
    if ext:
        g.enable_delay_correction(1)
        for o in oras:
            o.enable_delay_correction(1)
    out_g = np.empty((F, S, n), np.float32)
    out_o = np.empty((F, S, n), np.float32)
    for f in range(F):
        d = 700 if f in (300, 301) else 40
        out_g[f], rc_g = g.frame(far[f], near[f], d)
        for s in range(S):
            out_o[f, s], rc_o = oras[s].frame(far[f, s], near[f, s], d)
            assert rc_g == rc_o, (f, s)
        if f % 65 == 64 or f == F - 1:
            for s in range(S):
                assert g.delay_state(s).diff(oras[s].delay_state(), skip=()) == [], (f, s)
                st_o, _ = oras[s].export()
                rep = _state_report(g.export_state(s), st_o)
                bad = [k for k in LINEAR_FIELDS if not rep[k][0]]
                assert bad == [], (f, s, {k: rep[k] for k in bad})
    corr = [g.delay_state(s).delay_correction_count for s in range(S)]
    reads = {g.delay_state(s).far_read for s in range(S)}
    parity_note("delay-agnostic fs=%d n=%d ext=%d: corrections per stream %s, %d distinct far read positions, worst rel-L2 %.2e"
          % (fs, n, ext, corr, len(reads), max(_rel_l2(out_g[:, s], out_o[:, s]) for s in range(S))))
    for s in range(S):
        assert _rel_l2(out_g[:, s], out_o[:, s]) <= 1e-5, s
    assert max(corr) >= 1 and len(reads) > 1          # the streams did move apart
    rc, med, std = g.delay_metrics()
    assert rc == 0
    for s in range(S):
        assert (0, int(med[s]), int(std[s])) == oras[s].delay_metrics(), s


def test_delay_agnostic_bursty_far_end_vs_oracle(aec):
    """Delay-agnostic mode under an irregular call pattern: far-end frames arrive in bursts (several
    WebRtcAec_BufferFarend calls between two WebRtcAec_Process calls -- more than one launch descriptor holds, so the
    replay is flushed early -- and once 215 in a row, which overflows the 250-partition far buffer: every stream then
    drops ITS oldest partitions, aec_core.c:1622-1625) and near-end frames catch up in bursts; both call sizes.  One
    oracle per stream replays the same calls: return codes, outputs (<= 1e-5 rel-L2), linear state and the
    per-stream estimator / far-buffer / system-delay state bit for bit."""
    S = 5
    lags = [9, 0, 14, 5, 2]
    F = 620
    far, near = _lagged_frames(S, F, lags)
    g = aec.AecBatch(S, 16000)
    assert g.set_config(1, delay_logging=1) == 0
    g.enable_reported_delay(0)
    oras = [OracleAec(16000) for _ in range(S)]
    for o in oras:
        assert o.set_nlp(1, delay_logging=1) == 0
        o.enable_reported_delay(0)
    # the schedule: ("F", frame) = BufferFarend, ("N", frame) = Process; far frames never run behind the near frames
    sched, fi, ni = [], 0, 0
    rng = np.random.default_rng(17)
    flooded = False
    while ni < 330:
        burst = int(rng.choice([1, 1, 1, 2, 3, 11]))
        if ni >= 260 and not flooded:
            burst, flooded = 215, True
        burst = min(burst, F - fi)
        for _ in range(burst):
            sched.append(("F", fi))
            fi += 1
        for _ in range(min(max(burst, 1), 12) if burst != 215 else 1):
            if ni < fi and ni < 330:
                sched.append(("N", ni))
                ni += 1
    outs_g, outs_o = [], [[] for _ in range(S)]
    for k, (kind, f) in enumerate(sched):
        half = (k % 7) == 3      # some calls as two 80-sample halves
        parts = [(0, 80), (80, 160)] if half else [(0, 160)]
        for lo, hi in parts:
            if kind == "F":
                rc_g = g.buffer_farend(far[f][:, lo:hi])
                for s in range(S):
                    rc_o = oras[s].lib.asp_aec_oracle_buffer_farend(oras[s].h, np.ascontiguousarray(far[f, s, lo:hi]), hi - lo)
                    assert rc_g == rc_o, (k, s)
            else:
                og, rc_g = g.process(near[f][:, lo:hi], 40)
                outs_g.append(og)
                for s in range(S):
                    nn = np.ascontiguousarray(near[f, s, lo:hi])
                    oo = np.empty_like(nn)
                    rc_o = oras[s].lib.asp_aec_oracle_process(oras[s].h, nn, oo, hi - lo, 40, 0)
                    assert rc_g == rc_o, (k, s)
                    outs_o[s].append(oo)
        if k % 150 == 149 or k == len(sched) - 1:
            for s in range(S):
                assert g.delay_state(s).diff(oras[s].delay_state(), skip=()) == [], (k, s)
                st_o, _ = oras[s].export()
                rep = _state_report(g.export_state(s), st_o)
                bad = [x for x in LINEAR_FIELDS if not rep[x][0]]
                assert bad == [], (k, s, {x: rep[x] for x in bad})
    for s in range(S):
        a = np.concatenate([o[s] for o in outs_g])
        b = np.concatenate(outs_o[s])
        assert _rel_l2(a, b) <= 1e-5, s
    assert len({g.delay_state(s).system_delay for s in range(S)}) > 1      # the overflow hit the streams differently


def test_delay_agnostic_golden_and_layer1(aec):
    """tests/golden/aec_modes_golden.npz (written by the reference build): the delay-agnostic mode through the batch
    and through the per-stream WebRtcAec_enable_reported_delay / WebRtcAec_GetDelayMetrics symbols: outputs <= 1e-5
    rel-L2 (bar 1e-4), the reference's own delay metrics reproduced."""
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "aec_modes_golden.npz")))
    far, near = gold["agn_far_i16"].astype(np.float32), gold["agn_near_i16"].astype(np.float32)
    F, S = far.shape[:2]
    at = list(gold["agn_metrics_at"])
    g = aec.AecBatch(S, 16000)
    assert g.set_config(1, delay_logging=1) == 0
    g.enable_reported_delay(0)
    out = np.empty_like(near)
    for f in range(F):
        out[f], rc = g.frame(far[f], near[f], 40)
        assert rc == 0
        if f in at:
            rc, med, std = g.delay_metrics()
            for s in range(S):
                assert tuple(gold["agn_metrics"][at.index(f), s]) == (rc, int(med[s]), int(std[s])), (f, s)
    for s in range(S):
        assert _rel_l2(out[:, s], gold["agn_out_f32"][:, s]) <= 1e-5, s
    lib = g.lib
    f32p = C.POINTER(C.c_float)
    lib.WebRtcAec_Create.argtypes = [C.POINTER(C.c_void_p)]
    lib.WebRtcAec_Init.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.WebRtcAec_BufferFarend.argtypes = [C.c_void_p, f32p, C.c_int16]
    lib.WebRtcAec_Process.argtypes = [C.c_void_p, C.POINTER(f32p), C.c_int, C.POINTER(f32p), C.c_int16, C.c_int16, C.c_int32]
    lib.WebRtcAec_Free.argtypes = [C.c_void_p]
    lib.WebRtcAec_aec_core.restype = C.c_void_p
    lib.WebRtcAec_aec_core.argtypes = [C.c_void_p]
    lib.WebRtcAec_enable_reported_delay.restype = None
    lib.WebRtcAec_enable_reported_delay.argtypes = [C.c_void_p, C.c_int]
    lib.WebRtcAec_reported_delay_enabled.argtypes = [C.c_void_p]
    lib.WebRtcAec_GetDelayMetrics.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.WebRtcAec_set_config.argtypes = [C.c_void_p, aec.AecConfig]
    lib.WebRtcAec_get_error_code.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert lib.WebRtcAec_Create(C.byref(h)) == 0 and lib.WebRtcAec_Init(h, 16000, 48000) == 0
    med, std = C.c_int(), C.c_int()
    assert lib.WebRtcAec_GetDelayMetrics(h, C.byref(med), C.byref(std)) == -1 and lib.WebRtcAec_get_error_code(h) == 12001
    assert lib.WebRtcAec_set_config(h, aec.AecConfig(1, 0, 0, 1)) == 0
    core = lib.WebRtcAec_aec_core(h)
    assert lib.WebRtcAec_reported_delay_enabled(core) == 1
    lib.WebRtcAec_enable_reported_delay(core, 0)
    assert lib.WebRtcAec_reported_delay_enabled(core) == 0
    F1 = at[0] + 1
    got = np.empty((F1, 160), np.float32)
    for f in range(F1):
        fr, nr = np.ascontiguousarray(far[f, 1]), np.ascontiguousarray(near[f, 1])
        assert lib.WebRtcAec_BufferFarend(h, fr.ctypes.data_as(f32p), 160) == 0
        o = np.empty(160, np.float32)
        pin = (f32p * 1)(nr.ctypes.data_as(f32p))
        pout = (f32p * 1)(o.ctypes.data_as(f32p))
        assert lib.WebRtcAec_Process(h, pin, 1, pout, 160, 40, 0) == 0
        got[f] = o
    assert _rel_l2(got, gold["agn_out_f32"][:F1, 1]) <= 1e-5
    assert lib.WebRtcAec_GetDelayMetrics(h, C.byref(med), C.byref(std)) == 0
    assert (0, med.value, std.value) == tuple(gold["agn_metrics"][0, 1])
    assert lib.WebRtcAec_Free(h) == 0


@pytest.mark.parametrize("fs,n,sc_skew", [(16000, 160, 12), (8000, 80, -9)])
def test_skew_mode_vs_oracle(aec, fs, n, sc_skew):
    """set_config(skewMode = kAecTrue): the skew estimate from the calls' skew arguments (host, once per batch) and
    the linear resampling of every stream's far end on the device (aec_resample_kernel; aec_resampler.c:74-123,
    echo_cancellation.c:304-313, 614-645, 831-833) against the oracle (== reference build): control plane equal,
    linear state bit-exact, outputs <= 1e-5 rel-L2, across the estimate (call 425) and 130 resampled frames."""
    S, F = 5, 560
    far, near = aec_frames(S, F)
    far, near = far[:, :, :n], near[:, :, :n]
    g = aec.AecBatch(S, fs)
    assert g.set_config(1, skew=1) == 0
    oras = [OracleAec(fs) for _ in range(S)]
    for o in oras:
        assert o.set_nlp(1, skew=1) == 0
    rng = np.random.default_rng(3)
    out_g = np.empty((F, S, n), np.float32)
    out_o = np.empty((F, S, n), np.float32)
    resampled = 0
    for f in range(F):
        sk = 5000 if f % 97 == 0 else int(sc_skew + rng.integers(-2, 3))
        out_g[f], rc_g = g.frame(far[f], near[f], 30, sk)
        for s in range(S):
            out_o[f, s], rc_o = oras[s].frame_skew(far[f, s], near[f, s], 30, sk)
            assert rc_g == rc_o, (f, s)
        resampled += oras[0].skew_state()[1]
        if f % 70 == 69 or f == F - 1:
            cg = g.control()
            _, co = oras[0].export()
            for name, _t in cg._fields_:
                assert getattr(cg, name) == getattr(co, name), (f, name)
            for s in range(S):
                st_o, _ = oras[s].export()
                rep = _state_report(g.export_state(s), st_o)
                bad = [k for k in LINEAR_FIELDS if not rep[k][0]]
                assert bad == [], (f, s, {k: rep[k] for k in bad})
    assert resampled > 100
    worst = max(_rel_l2(out_g[:, s], out_o[:, s]) for s in range(S))
    parity_note("AEC skew fs=%d: %d resampled frames, %.4f of output samples bit-equal to the oracle, worst rel-L2 %.2e"
          % (fs, resampled, (_bits(out_g) == _bits(out_o)).mean(), worst))
    assert worst <= 1e-5


def test_skew_mode_golden(aec):
    """The reference's own skew-mode outputs (tests/golden/aec_modes_golden.npz): <= 1e-5 per-stream rel-L2."""
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "aec_modes_golden.npz")))
    far, near = gold["skew_far_i16"].astype(np.float32), gold["skew_near_i16"].astype(np.float32)
    F, S = far.shape[:2]
    g = aec.AecBatch(S, 16000)
    assert g.set_config(1, skew=1) == 0
    out = np.empty_like(near)
    for f in range(F):
        out[f], _ = g.frame(far[f], near[f], 30, int(gold["skew_arg"][f]))
    for s in range(S):
        assert _rel_l2(out[:, s], gold["skew_out_f32"][:, s]) <= 1e-5, s


def test_golden_reference_outputs(aec, aec_golden):
    """The reference's own outputs (committed fixture): <= 1e-5 per-stream rel-L2 (bar 1e-4),
    start-up frames passed through untouched, echo cancelled by > 15 dB."""
    far, near = aec_golden["far_i16"].astype(np.float32), aec_golden["near_i16"].astype(np.float32)
    g = aec.AecBatch(far.shape[1])
    out = g.run(far, near)
    want = aec_golden["out_f32"]
    assert np.array_equal(out[0], near[0])
    for s in range(far.shape[1]):
        assert _rel_l2(out[:, s], want[:, s]) <= 1e-5, s
    seg = slice(170, 290)
    erle = 10 * np.log10((near[seg].astype(np.float64) ** 2).mean() / (out[seg].astype(np.float64) ** 2).mean())
    assert erle > 15, erle


def test_run_equals_frame_by_frame_and_device_pointers(aec):
    """AspAecBatch_Run (one call, host or device buffers, in place) == BufferFarend + Process per
    frame, bit for bit; odd stream count exercises the partial workgroup."""
    from audiosignalprocess_amd.ns import DeviceBuffer

    S, F = 5, 130
    far, near = aec_frames(S, F)
    a = aec.AecBatch(S)
    want = np.stack([a.frame(far[f], near[f])[0] for f in range(F)])
    b = aec.AecBatch(S)
    assert np.array_equal(_bits(b.run(far, near)), _bits(want))
    c = aec.AecBatch(S)
    df, dn = DeviceBuffer(far.nbytes), DeviceBuffer(near.nbytes)
    df.upload(far)
    dn.upload(near)
    c.run_device(df.ptr, dn.ptr, dn.ptr, 160, F)   # in place
    c.synchronize()
    assert np.array_equal(_bits(dn.download(near.shape)), _bits(want))


def test_state_export_import_roundtrip(aec):
    """A stream's state exported from one batch and imported into another (same call history, so
    the same control plane) continues bit-identically; all-zero input stays finite."""
    S, F = 3, 160
    far, near = aec_frames(S, F + 40)
    a, b = aec.AecBatch(S), aec.AecBatch(S)
    far2 = far.copy()
    far2[:, 1] = 0      # silent far end on one stream
    near2 = near.copy()
    near2[:, 2] = 0     # silent near end on another
    for f in range(F):
        a.frame(far2[f], near2[f])
        b.frame(far2[f] * 0, near2[f] * 0)     # same calls, different data
    for s in range(S):
        st = a.export_state(s)
        b.import_state(s, st)
        rep = _state_report(b.export_state(s), st)
        assert all(v[0] for v in rep.values()), {k: v for k, v in rep.items() if not v[0]}
    # the rings are not part of the state: feed both the same frames and compare after the ring
    # contents have been flushed through (far ring keeps history only for delay jumps)
    oa = np.stack([a.frame(far2[F + k], near2[F + k])[0] for k in range(40)])
    assert np.isfinite(oa).all()


def test_layer1_reference_api(aec, aec_golden):
    """WebRtcAec_* exactly as test_aec_module.cpp:60-88 calls them; error codes of
    echo_cancellation.c:196-215,278-300,341-375."""
    lib = aec._lib()
    f32p = C.POINTER(C.c_float)
    lib.WebRtcAec_Create.argtypes = [C.POINTER(C.c_void_p)]
    lib.WebRtcAec_Init.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.WebRtcAec_BufferFarend.argtypes = [C.c_void_p, f32p, C.c_int16]
    lib.WebRtcAec_Process.argtypes = [C.c_void_p, C.POINTER(f32p), C.c_int, C.POINTER(f32p), C.c_int16,
                                      C.c_int16, C.c_int32]
    lib.WebRtcAec_Free.argtypes = [C.c_void_p]
    lib.WebRtcAec_get_error_code.argtypes = [C.c_void_p]
    lib.WebRtcAec_get_echo_status.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    h = C.c_void_p()
    assert lib.WebRtcAec_Create(C.byref(h)) == 0
    z = (C.c_float * 160)()
    assert lib.WebRtcAec_BufferFarend(h, z, 160) == -1 and lib.WebRtcAec_get_error_code(h) == 12002
    assert lib.WebRtcAec_Init(h, 44100, 48000) == -1 and lib.WebRtcAec_get_error_code(h) == 12004
    assert lib.WebRtcAec_Init(h, 16000, 48000) == 0
    assert lib.WebRtcAec_BufferFarend(h, z, 100) == -1 and lib.WebRtcAec_get_error_code(h) == 12004
    far, near = aec_golden["far_i16"][:, 0].astype(np.float32), aec_golden["near_i16"][:, 0].astype(np.float32)
    F = 260
    out = np.empty((F, 160), np.float32)
    for f in range(F):
        fb = np.ascontiguousarray(far[f])
        nb = np.ascontiguousarray(near[f])      # processed in place, like the driver
        assert lib.WebRtcAec_BufferFarend(h, fb.ctypes.data_as(f32p), 160) == 0
        p = (f32p * 1)(nb.ctypes.data_as(f32p))
        assert lib.WebRtcAec_Process(h, p, 1, p, 160, 0, 0) == 0
        out[f] = nb
    st = C.c_int(-1)
    assert lib.WebRtcAec_get_echo_status(h, C.byref(st)) == 0 and st.value in (0, 1)
    assert lib.WebRtcAec_Free(h) == 0
    assert _rel_l2(out, aec_golden["out_f32"][:F, 0]) <= 1e-5


def test_layer1_handles_as_echo_cancellation_unittest(aec):
    """The reference's EchoCancellationTest (aec/echo_cancellation_unittest.cc:26-50), restated on the exported symbols:
    Create / Free reject NULL, the core handle is NULL for NULL, a system delay set through the core handle reads back."""
    lib = aec._lib()
    lib.WebRtcAec_Create.argtypes = [C.POINTER(C.c_void_p)]
    lib.WebRtcAec_Free.argtypes = [C.c_void_p]
    lib.WebRtcAec_aec_core.restype = C.c_void_p
    lib.WebRtcAec_aec_core.argtypes = [C.c_void_p]
    lib.WebRtcAec_SetSystemDelay.restype = None
    lib.WebRtcAec_SetSystemDelay.argtypes = [C.c_void_p, C.c_int]
    lib.WebRtcAec_system_delay.argtypes = [C.c_void_p]
    assert lib.WebRtcAec_Create(None) == -1
    h = C.c_void_p()
    assert lib.WebRtcAec_Create(C.byref(h)) == 0 and h.value
    assert lib.WebRtcAec_Free(None) == -1
    assert lib.WebRtcAec_aec_core(None) is None
    core = lib.WebRtcAec_aec_core(h)
    assert core
    lib.WebRtcAec_SetSystemDelay(core, 111)
    assert lib.WebRtcAec_system_delay(core) == 111
    assert lib.WebRtcAec_Free(h) == 0


def test_scale_4096_streams_identical_inputs(aec):
    """BASELINE config-4 scale: 4096 streams; streams fed the same data give the same output
    whatever their position in the grid, and all outputs are finite."""
    S, F = 4096, 60
    far1, near1 = aec_frames(4, F)
    idx = np.arange(S) % 4
    g = aec.AecBatch(S)
    out = g.run(far1[:, idx], near1[:, idx])
    assert np.isfinite(out).all()
    for k in range(4):
        ref = out[:, k]
        assert np.array_equal(_bits(out[:, k::4]), _bits(np.broadcast_to(ref[:, None], out[:, k::4].shape)))
    assert not np.array_equal(out[F - 1, 0], near1[F - 1, 0])


def test_scale_4096_streams_optional_modes(aec):
    """BASELINE config-4 scale with every optional mode on at once -- extended filter, echo metrics, delay logging,
    the delay-agnostic mode (per-stream far-buffer control on the device) and skew compensation: 4096 streams of 4
    distinct signals with 4 different echo-path delays; equal inputs give bit-equal outputs and equal per-stream
    control state wherever the stream sits in the grid, streams with different delays end at different far-buffer
    positions, and stream k equals an oracle fed the same calls (<= 1e-5 rel-L2, estimator state bit for bit)."""
    S, F = 4096, 460      # past call 425: the skew estimate exists and the far end is resampled
    far4, near4 = _lagged_frames(4, F, [9, 0, 14, 5])
    idx = np.arange(S) % 4
    g = aec.AecBatch(S)
    assert g.set_config(1, skew=1, metrics=1, delay_logging=1) == 0
    g.enable_reported_delay(0)
    g.enable_delay_correction(1)
    oras = [OracleAec(16000) for _ in range(4)]
    for o in oras:
        assert o.set_nlp(1, skew=1, metrics=1, delay_logging=1) == 0
        o.enable_reported_delay(0)
        o.enable_delay_correction(1)
    out = np.empty((F, S, 160), np.float32)
    out_o = np.empty((F, 4, 160), np.float32)
    for f in range(F):
        out[f], rc = g.frame(far4[f][idx], near4[f][idx], 40, 15 + f % 3)
        for k in range(4):
            out_o[f, k], rc_o = oras[k].frame_skew(far4[f, k], near4[f, k], 40, 15 + f % 3)
            assert rc == rc_o, (f, k)
    assert np.isfinite(out).all()
    for k in range(4):
        assert np.array_equal(_bits(out[:, k::4]), _bits(np.broadcast_to(out[:, k][:, None], out[:, k::4].shape))), k
        assert _rel_l2(out[:, k], out_o[:, k]) <= 1e-5, k
        for s in (k, 2048 + k, 4092 + k):
            assert g.delay_state(s).diff(oras[k].delay_state(), skip=()) == [], s
    assert len({g.delay_state(k).far_read for k in range(4)}) > 1
    rc, med, std = g.delay_metrics()
    assert rc == 0
    for k in range(4):
        assert (med[k::4] == med[k]).all() and (0, int(med[k]), int(std[k])) == oras[k].delay_metrics(), k


def test_timed_steps_two_chains_equal_one_chain(aec, monkeypatch):
    """The K-step path (AspAecBatch_TimedSteps) runs large batches as two launch chains over the two halves
    of the batch: outputs and the filter state must equal the single-chain run bit for bit, and an odd half
    boundary (S / 2 not a multiple of four) must not lose streams."""
    from audiosignalprocess_amd.ns import DeviceBuffer

    S, F = 2050, 150
    far4, near4 = aec_frames(4, F)
    idx = np.arange(S) % 4
    far = np.ascontiguousarray(far4[:, idx])
    near = np.ascontiguousarray(near4[:, idx])
    per = S * 160 * 4  # bytes per frame of all streams
    df, dn = DeviceBuffer(far.nbytes), DeviceBuffer(near.nbytes)
    df.upload(far)
    dn.upload(near)
    outs, states = [], []
    for chains, flow in (("1", 0), ("2", 0), ("1", 1)):   # one chain, two chains, the hand-off build
        monkeypatch.setenv("ASP_AEC_CHAINS", chains)
        g = aec.AecBatch(S)
        g.set_flow(flow)
        do = DeviceBuffer(near.nbytes)
        g.timed_steps(df.ptr, dn.ptr, do.ptr, 160, F, 100)   # through the start-up phase: one chain
        g.timed_steps(df.ptr + 100 * per, dn.ptr + 100 * per, do.ptr + 100 * per, 160, F - 100, F - 100)
        g.synchronize()
        outs.append(do.download(near.shape))
        states.append([np.ctypeslib.as_array(g.export_state(s).wfBuf).copy() for s in (0, 1023, 1027, 2049)])
        g.close()
    for k in (1, 2):
        assert np.array_equal(outs[0].view(np.uint32), outs[k].view(np.uint32)), k
        for a, b in zip(states[0], states[k]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    # and both equal the four distinct streams they replicate
    assert np.array_equal(outs[1][:, 4:8].view(np.uint32), outs[1][:, 2044:2048].view(np.uint32))


def test_timed_steps_equal_run_and_oracle(aec, monkeypatch):
    """AspAecBatch_TimedSteps (the entry point bench.py times: K steps over device rings, one or two
    launch chains) against AecBatch.run() on the same frames -- bit for bit, outputs and filter state --
    and against the oracle with the bars of test_free_running_vs_oracle."""
    from audiosignalprocess_amd.ns import DeviceBuffer

    S, F, D = 2056, 220, 4
    far4, near4 = aec_frames(D, F)
    idx = np.arange(S) % D
    far = np.ascontiguousarray(far4[:, idx])
    near = np.ascontiguousarray(near4[:, idx])
    per = S * 160 * 4
    df, dn = DeviceBuffer(far.nbytes), DeviceBuffer(near.nbytes)
    df.upload(far)
    dn.upload(near)
    gr = aec.AecBatch(S)
    gr.set_flow(0)                      # the reference run: one launch per call
    out_run = gr.run(far, near)
    oras = [OracleAec() for _ in range(D)]
    out_o = np.stack([oras[s].run(far4[:, s], near4[:, s]) for s in range(D)], axis=1)
    for chains, flow in (("1", 0), ("2", 0), ("1h", 1)):   # one chain, two chains, the hand-off build
        monkeypatch.setenv("ASP_AEC_CHAINS", chains[0])
        g = aec.AecBatch(S)
        g.set_flow(flow)
        do = DeviceBuffer(near.nbytes)
        g.timed_steps(df.ptr, dn.ptr, do.ptr, 160, F, 100)
        g.timed_steps(df.ptr + 100 * per, dn.ptr + 100 * per, do.ptr + 100 * per, 160, F - 100, F - 100)
        g.synchronize()
        out_t = do.download(near.shape)
        assert np.array_equal(_bits(out_t), _bits(out_run)), chains
        for s in (0, 1, 1027, 1028, S - 1):
            rep = _state_report(g.export_state(s), gr.export_state(s))
            assert all(v[0] for v in rep.values()), (chains, s, {k: v for k, v in rep.items() if not v[0]})
            st_o, _ = oras[int(idx[s])].export()
            rep = _state_report(g.export_state(s), st_o)
            bad = [k for k in LINEAR_FIELDS if not rep[k][0]]
            assert bad == [], (chains, s, {k: rep[k] for k in bad})
            assert _rel_l2(out_t[:, s], out_o[:, idx[s]]) <= 1e-5, (chains, s)
        g.close()
    gr.close()


@pytest.mark.parametrize("ext", [0, 1])
def test_per_stream_delays_and_reinit_vs_one_oracle_per_stream(aec, ext):
    """The reference takes the reported delay and Init per handle (echo_cancellation.c:341-347, 196-276).
    AspAecBatch_ProcessV / _InitStream: twelve streams with different reported delays -- so their start-up phases end
    at different frames and their far buffers, ring positions and partition positions move apart -- a delay jump, an
    out-of-range delay (returns -1, still processes) and a negative one on three of them, one stream re-initialised
    in the middle of the run, and the uniform-argument calls used on top of it: every stream against its OWN oracle
    driven the same way, with the bars of test_free_running_vs_oracle (control plane equal, linear state bit-exact,
    outputs within 1e-5)."""
    S, F = 12, 460
    far, near = aec_frames(S, F)
    g = aec.AecBatch(S, 16000)
    oras = [OracleAec(16000) for _ in range(S)]
    if ext:
        g.enable_delay_correction(1)
        for o in oras:
            o.enable_delay_correction(1)
    base = [0, 0, 20, 40, 60, 100, 5, 0, 250, 30, 80, 10]

    def delay(s, f):
        d = base[s]
        if s == 1 and f >= 130:
            d = 90
        if s == 4 and 200 <= f < 210:
            d = 700
        if s == 7 and f == 250:
            d = -5
        return d

    out_g = np.empty((F, S, 160), np.float32)
    out_o = np.empty((F, S, 160), np.float32)
    born = [0] * S
    for f in range(F):
        if f == 170:
            g.init_stream(5)
            oras[5] = OracleAec(16000)
            if ext:
                oras[5].enable_delay_correction(1)
            born[5] = f
        uniform = 300 <= f < 320          # the uniform-argument entry points on top of the per-stream control
        assert g.buffer_farend(far[f]) == 0
        if uniform:
            out_g[f], rc_g = g.process(near[f], 35)
        else:
            out_g[f], status = g.process_v(near[f], [delay(s, f) for s in range(S)])
        for s in range(S):
            out_o[f, s], rc_o = oras[s].frame(far[f, s], near[f, s], 35 if uniform else delay(s, f))
            if not uniform:
                assert status[s] == rc_o, (f, s)
        if f % 50 == 49:
            for s in range(S):
                cg = g.control_stream(s)
                _, co = oras[s].export()
                for name, _t in cg._fields_:
                    assert getattr(cg, name) == getattr(co, name), (f, s, name)
    assert len({g.control_stream(s).far_read for s in range(S)}) > 3      # the streams did move apart
    assert len({g.control_stream(s).blocks_processed for s in range(S)}) > 1
    for s in range(S):
        st_o, _ = oras[s].export()
        rep = _state_report(g.export_state(s), st_o)
        bad = [k for k in LINEAR_FIELDS if not rep[k][0]]
        assert bad == [], (s, {k: rep[k] for k in bad})
        assert _rel_l2(out_g[born[s]:, s], out_o[born[s]:, s]) <= 1e-5, s
    parity_note("AEC per-stream control ext=%d: %d streams, %d distinct far read positions, worst rel-L2 %.2e"
                % (ext, S, len({g.control_stream(s).far_read for s in range(S)}),
                   max(_rel_l2(out_g[born[s]:, s], out_o[born[s]:, s]) for s in range(S))))
    g.close()


@pytest.mark.parametrize("S,ext", [(5, 0), (4100, 0), (9000, 0), (1030, 1)])
def test_handoff_build_equals_plain_launches(aec, S, ext):
    """The hand-off build (AspAecBatch_SetFlow; the default of Run / TimedSteps in the plain configuration) against
    one launch per call: outputs and the whole state bit for bit over 300 frames (start-up, delay jumps are in
    test_free_running_vs_oracle; here: many streams, ragged last workgroup, more streams than the chip holds
    waves, the extended filter).  Two hand-off batches and the plain one run at the same time, so the waits
    happen under uneven load."""
    from audiosignalprocess_amd.ns import DeviceBuffer

    F, D = 300, 8
    far8, near8 = aec_frames(D, F)
    idx = (np.arange(S) * 3) % D
    far = np.ascontiguousarray(far8[:, idx])
    near = np.ascontiguousarray(near8[:, idx])
    df, dn = DeviceBuffer(far.nbytes), DeviceBuffer(near.nbytes)
    df.upload(far)
    dn.upload(near)
    outs, batches = [], []
    for flow in (0, 1, 1):
        g = aec.AecBatch(S)
        if ext:
            g.enable_delay_correction(1)
        g.set_flow(flow)
        do = DeviceBuffer(near.nbytes)
        g.run_device(df.ptr, dn.ptr, do.ptr, 160, F)   # asynchronous: the batches overlap on the chip
        outs.append(do)
        batches.append(g)
    for g in batches:
        g.synchronize()
    y = [o.download(near.shape) for o in outs]
    assert np.isfinite(y[0][-50:]).all() and np.abs(y[0]).max() > 0
    for k in (1, 2):
        assert np.array_equal(_bits(y[0]), _bits(y[k])), k
    for s_ in sorted(set([0, 1, 3, 4, S // 2, S - 2, S - 1] + list(range(0, S, max(1, S // 23))))):
        want = batches[0].export_state(s_)
        for k in (1, 2):
            rep = _state_report(batches[k].export_state(s_), want)
            assert all(v[0] for v in rep.values()), (s_, k, {f: v for f, v in rep.items() if not v[0]})
    for g in batches:
        g.close()

@pytest.mark.parametrize("S,ext", [(37, 0), (1030, 0), (37, 1)])
def test_handoff_build_delay_logging(aec, S, ext):
    """Delay logging in the hand-off build: the process kernel forms each block's binary far / near spectra (bands
    12..43 against the mean spectra, delay_estimator_wrapper.c:96-124) and the rest of the estimator runs once per
    launch over all its blocks (aec_delay_bits_kernel) -- against one process + one estimator launch per call:
    outputs, the estimator's whole state, the logging histogram's metrics, bit for bit; and for the first streams
    against the oracle."""
    from audiosignalprocess_amd.ns import DeviceBuffer

    F, D = 330, 6
    far8, near8 = _lagged_frames(D, F, [6, 0, 9, 3, 6, 12])
    idx = (np.arange(S) * 5) % D
    far = np.ascontiguousarray(far8[:, idx])
    near = np.ascontiguousarray(near8[:, idx])
    df, dn = DeviceBuffer(far.nbytes), DeviceBuffer(near.nbytes)
    df.upload(far)
    dn.upload(near)
    outs, batches = [], []
    for flow in (0, 1):
        g = aec.AecBatch(S)
        assert g.set_config(1, delay_logging=1) == 0
        if ext:
            g.enable_delay_correction(1)
        g.set_flow(flow)
        do = DeviceBuffer(near.nbytes)
        for f0 in (0, 150, 151):   # three calls: 150 frames (64 + 64 + 22 per launch), one frame (no hand-off), the rest
            f1 = {0: 150, 150: 151, 151: F}[f0]
            off = f0 * S * 160 * 4
            g.run_device(df.ptr + off, dn.ptr + off, do.ptr + off, 160, f1 - f0, 20)
        outs.append(do)
        batches.append(g)
    for g in batches:
        g.synchronize()
    y = [o.download(near.shape) for o in outs]
    assert np.array_equal(_bits(y[0]), _bits(y[1]))
    for s_ in sorted(set([0, 1, 2, 3, 4, 5, S // 2, S - 1])):
        assert batches[1].delay_state(s_).diff(batches[0].delay_state(s_)) == [], s_
    oras = [OracleAec(16000) for _ in range(3)]
    for k, o in enumerate(oras):
        assert o.set_nlp(1, delay_logging=1) == 0
        if ext:
            o.enable_delay_correction(1)
        for f in range(F):
            o.frame(far[f, k], near[f, k], 20)
        assert batches[1].delay_state(k).diff(o.delay_state()) == [], k
    m = [g.delay_metrics() for g in batches]   # (clears the logging histogram, aec_core.c:1780-1836)
    assert m[0][0] == 0 and m[1][0] == 0
    assert np.array_equal(m[0][1], m[1][1]) and np.array_equal(m[0][2], m[1][2])
    assert (m[0][1] >= 0).any()
    for k, o in enumerate(oras):
        assert (0, int(m[1][1][k]), int(m[1][2][k])) == o.delay_metrics(), k
    for g in batches:
        g.close()

@pytest.mark.parametrize("S,ext", [(37, 0), (1030, 0), (37, 1)])
def test_handoff_build_delay_agnostic(aec, S, ext):
    """The delay-agnostic mode in the hand-off build: each stream's wave runs its own far-buffer control step per
    sub-frame (SignalBasedDelayCorrection, read-pointer moves, soft reset) and the estimator's share of its blocks,
    inside a launch of up to 64 frame steps -- against one launch per call (the same fused wave, aec_process_agn_kernel):
    outputs, the whole state, the estimator and the far-buffer positions bit for bit; the first streams against the
    oracle; the streams' read positions must have moved apart."""
    from audiosignalprocess_amd.ns import DeviceBuffer

    F, D = 330, 6
    far8, near8 = _lagged_frames(D, F, [6, 0, 9, 3, 6, 12])
    idx = (np.arange(S) * 5) % D
    far = np.ascontiguousarray(far8[:, idx])
    near = np.ascontiguousarray(near8[:, idx])
    df, dn = DeviceBuffer(far.nbytes), DeviceBuffer(near.nbytes)
    df.upload(far)
    dn.upload(near)
    outs, batches = [], []
    for flow in (0, 1):
        g = aec.AecBatch(S)
        assert g.set_config(1, delay_logging=1) == 0
        if ext:
            g.enable_delay_correction(1)
        g.enable_reported_delay(0)
        g.set_flow(flow)
        do = DeviceBuffer(near.nbytes)
        for f0, f1 in ((0, 150), (150, 151), (151, F)):
            off = f0 * S * 160 * 4
            g.run_device(df.ptr + off, dn.ptr + off, do.ptr + off, 160, f1 - f0, 20)
        outs.append(do)
        batches.append(g)
    for g in batches:
        g.synchronize()
    y = [o.download(near.shape) for o in outs]
    assert np.array_equal(_bits(y[0]), _bits(y[1]))
    reads = set()
    for s_ in sorted(set([0, 1, 2, 3, 4, 5, S // 2, S - 1])):
        d0, d1 = batches[0].delay_state(s_), batches[1].delay_state(s_)
        assert d1.diff(d0) == [], s_
        reads.add(d1.far_available())
        rep = _state_report(batches[1].export_state(s_), batches[0].export_state(s_))
        assert all(v[0] for v in rep.values()), (s_, {f: v for f, v in rep.items() if not v[0]})
    assert len(reads) >= 3, reads
    for k in range(3):
        o = OracleAec(16000)
        assert o.set_nlp(1, delay_logging=1) == 0
        if ext:
            o.enable_delay_correction(1)
        o.enable_reported_delay(0)
        for f in range(F):
            oo, _ = o.frame(far[f, k], near[f, k], 20)
            assert _rel_l2(y[1][f, k], oo) <= 1e-5, (f, k)
        assert batches[1].delay_state(k).diff(o.delay_state()) == [], k
    for g in batches:
        g.close()


def test_wav_driver_end_to_end(aec, aec_golden, tmp_path):
    """drivers/test_aec_module (the reference's test_aec_module.cpp loop in C over WebRtcAec_*):
    mic.wav + speaker.wav -> result.wav equals the reference's float output rounded by
    FloatS16ToS16, within 1 LSB on < 0.1 % of samples (powf/cosf/sinf last places)."""
    import struct
    import subprocess

    from audiosignalprocess_amd.build import build_drivers

    exe = [e for e in build_drivers() if e.endswith("test_aec_module")][0]
    F = 400
    far, near = aec_golden["far_i16"][:F, 0].reshape(-1), aec_golden["near_i16"][:F, 0].reshape(-1)

    def wav(samples):
        return b"RIFF" + struct.pack("<i", 36 + samples.nbytes) + b"WAVE" + \
            struct.pack("<4sihhiihh", b"fmt ", 16, 1, 1, 16000, 32000, 2, 16) + \
            b"data" + struct.pack("<i", samples.nbytes) + samples.tobytes()

    (tmp_path / "mic.wav").write_bytes(wav(near))
    (tmp_path / "spk.wav").write_bytes(wav(far))
    subprocess.run([exe, str(tmp_path / "mic.wav"), str(tmp_path / "spk.wav"), str(tmp_path / "out.wav"), "-q"],
                   check=True, stdout=subprocess.DEVNULL)
    out = np.frombuffer((tmp_path / "out.wav").read_bytes()[44:], dtype=np.int16)
    assert out.size == (F + 1) * 160          # the feof loop emits one extra (stale) frame
    want = aec_golden["out_f32"][:F, 0].reshape(-1)
    want_i16 = np.where(want > 0, np.floor(want + np.float32(0.5)), np.ceil(want - np.float32(0.5)))
    want_i16 = np.clip(want_i16, -32768, 32767).astype(np.int32)
    d = np.abs(out[:F * 160].astype(np.int32) - want_i16)
    assert d.max() <= 1 and (d == 0).mean() >= 0.999


def test_device_pow_sincos_lean_equal_plain_forms(aec):
    """The NLP's lean fp64 pow / cos / sin (ns_device.h) return what the plain
    (float)f((double)x) forms return: pow for EVERY float base (all 2^32 bit patterns: negative,
    zero, denormal, > 1, inf, NaN included) at several exponents in the overdrive range, cos / sin
    for every float in [0, 8] and a stretch beyond (fallback range)."""
    from audiosignalprocess_amd import ns
    from tests.test_ns_gpu import _sweep_all_floats

    lib = ns.load_library()
    step = 1 << 28
    for y in (1.0, 1.1767766, 2.0, 3.3137085, 7.25, 15.0, 40.0):
        total, examples = 0, []
        for start in range(0, 1 << 32, step):
            from tests.test_ns_gpu import _debug_compare
            n, ex = _debug_compare(lib, 14, 13, start, step, param=y)
            total += n
            examples += ex
        assert total == 0, (y, total, [hex(b) for b in examples[:8]])
    for fa, fb, name in [(16, 15, "cos"), (18, 17, "sin")]:
        bad, ex = _sweep_all_floats(lib, fa, fb, 0x00000000, 0x42000000)   # [0, 32)
        assert bad == 0, (name, bad, [hex(b) for b in ex[:8]])
        bad, ex = _sweep_all_floats(lib, fa, fb, 0x80000000, 0xc1000000)   # negatives: fallback
        assert bad == 0, (name, bad, [hex(b) for b in ex[:8]])


def test_two_bands_32khz_vs_oracle(aec):
    """32 kHz: low band as at 16 kHz; the high band (delay line x average NLP gain + H-band comfort
    noise) against the oracle: the device evaluates this branch's (float)cos / (float)sin exactly as
    the reference does, so the high band inherits only the low band's powf last places.  Linear
    state bit-exact, both outputs within 1e-5 per-stream rel-L2, layer-1 entry point included."""
    from tests.test_aec_oracle import _aec_band_frames

    S, F = 5, 420
    far1, nl1, nh1 = _aec_band_frames(F)
    rng = np.random.default_rng(9)
    scale = (0.5 + rng.random(S)).astype(np.float32)
    far = far1[:, None, :] * scale[None, :, None]
    nl = nl1[:, None, :] * scale[None, :, None]
    nh = nh1[:, None, :] * scale[None, :, None]
    g = aec.AecBatch(S, 32000)
    oras = [OracleAec(32000) for _ in range(S)]
    gl, gh = np.empty_like(nl), np.empty_like(nh)
    ol, oh = np.empty_like(nl), np.empty_like(nh)
    for f in range(F):
        d = 40 if 250 <= f < 330 else 0
        gl[f], gh[f], rc_g = g.frame_bands(far[f], nl[f], nh[f], d)
        for s in range(S):
            ol[f, s], oh[f, s], rc_o = oras[s].frame_bands(far[f, s], nl[f, s], nh[f, s], d)
        assert rc_g == rc_o, f
    for s in range(S):
        st_o, _ = oras[s].export()
        rep = _state_report(g.export_state(s), st_o)
        bad = [k for k in LINEAR_FIELDS + ["dBufH"] if not rep[k][0]]
        assert bad == [], (s, {k: rep[k] for k in bad})
        assert _rel_l2(gl[:, s], ol[:, s]) <= 1e-5 and _rel_l2(gh[:, s], oh[:, s]) <= 1e-5, s
    parity_note("AEC 32 kHz: low %.4f / high %.4f of output samples bit-equal to the oracle"
          % ((_bits(gl) == _bits(ol)).mean(), (_bits(gh) == _bits(oh)).mean()))
    assert np.abs(gh[170:240]).mean() < 0.9 * np.abs(nh[170:240]).mean()
    # a 32 kHz batch refuses the one-band entry point, 48 kHz is refused at Init
    out, rc = g.process(nl[0])
    assert rc == -1 and g.error_code() == 12004
    assert aec.AecBatch(2, 48000).init_rc == -1


def test_two_bands_32khz_optional_modes_vs_oracle(aec):
    """32 kHz with the extended filter, delay logging and the delay-agnostic mode together (each 160-sample call is two
    per-sub-frame launches with both bands' buffers offset by 80 samples): both bands within 1e-5 rel-L2 of one
    oracle per stream, linear state and the per-stream estimator / far-buffer state bit for bit."""
    from tests.test_aec_oracle import _aec_band_frames

    S, F = 4, 460
    lags = [7, 0, 11, 4]
    far1, nl1, nh1 = _aec_band_frames(F + max(lags))
    far = np.stack([far1[l:l + F] for l in lags], axis=1)
    nl = np.repeat(nl1[:F, None, :], S, axis=1)
    nh = np.repeat(nh1[:F, None, :], S, axis=1)
    g = aec.AecBatch(S, 32000)
    assert g.set_config(1, delay_logging=1) == 0
    g.enable_reported_delay(0)
    g.enable_delay_correction(1)
    oras = [OracleAec(32000) for _ in range(S)]
    for o in oras:
        assert o.set_nlp(1, delay_logging=1) == 0
        o.enable_reported_delay(0)
        o.enable_delay_correction(1)
    gl, gh = np.empty_like(nl), np.empty_like(nh)
    ol, oh = np.empty_like(nl), np.empty_like(nh)
    for f in range(F):
        gl[f], gh[f], rc_g = g.frame_bands(far[f], nl[f], nh[f], 30)
        for s in range(S):
            ol[f, s], oh[f, s], rc_o = oras[s].frame_bands(far[f, s], nl[f, s], nh[f, s], 30)
            assert rc_g == rc_o, (f, s)
    for s in range(S):
        st_o, _ = oras[s].export()
        rep = _state_report(g.export_state(s), st_o)
        bad = [k for k in LINEAR_FIELDS + ["dBufH"] if not rep[k][0]]
        assert bad == [], (s, {k: rep[k] for k in bad})
        assert g.delay_state(s).diff(oras[s].delay_state(), skip=()) == [], s
        assert _rel_l2(gl[:, s], ol[:, s]) <= 1e-5 and _rel_l2(gh[:, s], oh[:, s]) <= 1e-5, s
    assert max(g.delay_state(s).delay_correction_count for s in range(S)) >= 1


def _metrics_compare(ma, mb):
    """ma: HIP image, mb: oracle image (uint32[65], include/asp_aec.h: AspAecMetricsState).
    far / near / linear-out levels come from bit-exact spectra summed in the reference's order:
    identical words.  The NLP-out level sits behind powf / cosf / sinf (<= 1e-5 relative) and the
    statistics behind log10 of ratios of those levels (<= 1e-3 dB); counters are identical."""
    assert np.array_equal(ma[:21], mb[:21])
    fa, fb = ma.view(np.float32), mb.view(np.float32)
    for k in (21, 23, 24, 26, 27):        # nlpoutlevel floats: sfrsum framelevel frsum minlevel averagelevel
        assert abs(fa[k] - fb[k]) <= 1e-5 * abs(fb[k]) + 1e-12, k
    assert ma[22] == mb[22] and ma[25] == mb[25]
    for j in range(4):
        o = 28 + 9 * j
        assert np.allclose(fa[o:o + 7], fb[o:o + 7], rtol=0, atol=1e-3), (j, fa[o:o + 7], fb[o:o + 7])
        assert np.array_equal(ma[o + 7:o + 9], mb[o + 7:o + 9])
    assert ma[64] == mb[64]


def test_metrics_mode_vs_oracle_and_golden(aec, aec_golden):
    """metricsMode = kAecTrue (aec_core.c:585-770, echo_cancellation.c:456-548): ERL / ERLE / A_NLP of
    every stream against the oracle and against the reference's values in the fixture."""
    far, near = aec_golden["far_i16"].astype(np.float32), aec_golden["near_i16"].astype(np.float32)
    F, S = far.shape[:2]
    g = aec.AecBatch(S)
    assert g.set_config(1, metrics=2) == -1 and g.error_code() == 12004
    assert g.set_config(1, metrics=1) == 0
    assert (g.get_metrics()[:, [0, 4, 8, 12]] == -100).all()          # nothing measured yet
    outs = []
    for f in range(F):
        out, rc = g.frame(far[f], near[f])
        assert rc == 0
        outs.append(out)
        if f + 1 in (F // 2, F):
            k = 0 if f + 1 == F // 2 else 1
            for s in range(S):
                _metrics_compare(g.metrics_state(s).to_array(), aec_golden["met_state_u32"][k, s])
            lv = g.get_metrics()
            assert np.abs(lv - aec_golden["met_levels_i32"][k]).max() <= 1   # (int) of a float within 1e-3 dB
            assert (lv == aec_golden["met_levels_i32"][k]).mean() >= 0.9
    assert _rel_l2(np.stack(outs), aec_golden["out_f32"]) <= 1e-5          # metrics leave the audio alone
    # set_config restarts the statistics (aec_core.c:1858-1861); Init leaves the mode off
    assert g.set_config(1, metrics=1) == 0
    m = g.metrics_state(0)
    assert m.erle.counter == 0 and m.farlevel.minlevel == np.float32(1e17) and m.erle.min == 100
    # layer 1 (one stream): WebRtcAec_GetMetrics goes the same way
    lib = aec._lib()
    from audiosignalprocess_amd._abi import AecMetrics
    lib.WebRtcAec_GetMetrics.argtypes = [C.c_void_p, C.c_void_p]
    h1 = aec.AecBatch(1)
    m1 = AecMetrics()
    assert lib.WebRtcAec_GetMetrics(h1.h, C.byref(m1)) == 0 and m1.to_tuple()[:4] == (-100,) * 4
    assert lib.WebRtcAec_GetMetrics(h1.h, None) == -1 and h1.error_code() == 12003


def test_metrics_bursty_far_end_vs_oracle(aec):
    """A bursty far end through a synthetic echo path, 3 streams with different seeds, 80-sample
    frames with a reported delay; also the case where the reference's NLP emits NaN (hNl < 0 into
    powf, aec_core.c:289): the device must do the same, and the poisoned NLP-out level must
    recover the same way."""
    F, S = 700, 3
    far = np.empty((F, S, 160), np.float32)
    near = np.empty((F, S, 160), np.float32)
    for s in range(S):
        rng = np.random.default_rng(5 + s)
        x = (rng.standard_normal((F, 160)) * 3000).astype(np.float32)
        x *= np.repeat((rng.random(F // 20) > 0.3).astype(np.float32), 20)[:, None] * 0.98 + 0.02
        h = (rng.standard_normal(200) * np.exp(-np.arange(200) / 40)).astype(np.float32) * 0.3
        y = np.convolve(x.reshape(-1), h)[:F * 160].astype(np.float32)
        far[:, s] = x
        near[:, s] = (y + rng.standard_normal(F * 160).astype(np.float32) * 30).reshape(F, 160)
    g = aec.AecBatch(S)
    assert g.set_config(2, metrics=1) == 0
    orc = [OracleAec(16000) for _ in range(S)]
    for o in orc:
        assert o.set_nlp(2, metrics=1) == 0
    nan_frames = 0
    for f in range(F):
        out, rc = g.frame(far[f], near[f], 40)
        assert rc == 0
        for s in range(S):
            ref, _ = orc[s].frame(far[f, s], near[f, s], 40)
            assert np.array_equal(np.isnan(out[s]), np.isnan(ref)), (f, s)
            ok = ~np.isnan(ref)
            nan_frames += int((~ok).any())
            assert np.abs(out[s][ok] - ref[ok]).max() <= 0.05 + 1e-4 * np.abs(ref[ok]).max(), (f, s)
    for s in range(S):
        ma, mb = g.metrics_state(s).to_array(), orc[s].metrics_state().to_array()
        assert np.array_equal(ma[:21], mb[:21])
        fa, fb = ma.view(np.float32), mb.view(np.float32)
        assert np.array_equal(ma[[22, 25, 35, 36, 44, 45, 53, 54, 64]], mb[[22, 25, 35, 36, 44, 45, 53, 54, 64]])
        assert np.allclose(fa[28:35], fb[28:35], atol=1e-3, equal_nan=True)          # ERL: no NLP in it
        assert np.allclose(fa[46:53], fb[46:53], atol=1e-3, equal_nan=True)          # A_NLP: linear output only
        assert np.allclose(fa[37:44], fb[37:44], atol=1e-2, equal_nan=True)          # ERLE: behind the NLP (NaN included)
    assert np.array_equal(g.get_metrics()[:, 4:8], np.array([o.get_metrics().to_tuple()[4:8] for o in orc]))
    assert nan_frames > 0, "this input is meant to reach the reference's NaN case"


def test_same_input_through_every_issuer(aec):
    """One input through every way a control step's work reaches the device (aec_api.hip, DeviceIssuer: launch, hand-off
    record, stream record; the fourth, none, issues nothing): (a) plain launches, BufferFarend + Process per frame;
    (b) Run with the hand-off build; (c) Run without it (plain launches with the far-end work deferred into each
    Process launch); (d) per-stream control, BufferFarend + ProcessV with the same delay on every
    stream.  5 streams (a ragged workgroup), 200 frames, reported delay 40 ms jumping to 90 ms at frame 130: start-up
    end, a far-pointer move, steady state.  Outputs and the whole state of (a), (b), (c) are equal bit for bit, and
    so are those of (d): its kernels run the same block code on the same descriptors, read from device memory
    (measured equal before the control plane was split; test_handoff_build_equals_plain_launches holds the same bar
    between (b) and (c)).  (d)'s control plane of every stream equals (a)'s."""
    from audiosignalprocess_amd.ns import DeviceBuffer

    S, F, J = 5, 200, 130
    far, near = aec_frames(S, F)
    delay = lambda f: 40 if f < J else 90
    outs, batches = {}, {}
    g = batches["a"] = aec.AecBatch(S)
    outs["a"] = np.stack([g.frame(far[f], near[f], delay(f))[0] for f in range(F)])
    # Run on device buffers: there a hand-off build that cannot get its resources is an error, not a quiet fall-back
    per = S * 160 * 4
    df, dn = DeviceBuffer(far.nbytes), DeviceBuffer(near.nbytes)
    df.upload(far)
    dn.upload(near)
    for key, flow in (("b", 1), ("c", 0)):
        g = batches[key] = aec.AecBatch(S)
        g.set_flow(flow)
        do = DeviceBuffer(near.nbytes)
        g.run_device(df.ptr, dn.ptr, do.ptr, 160, J, delay(0))
        g.run_device(df.ptr + J * per, dn.ptr + J * per, do.ptr + J * per, 160, F - J, delay(J))
        g.synchronize()
        outs[key] = do.download(near.shape)
    g = batches["d"] = aec.AecBatch(S)
    out_d = np.empty_like(near)
    for f in range(F):
        assert g.buffer_farend(far[f]) == 0
        out_d[f], status = g.process_v(near[f], [delay(f)] * S)
        assert not status.any(), f
    outs["d"] = out_d
    assert np.isfinite(outs["a"]).all() and np.abs(outs["a"][-50:]).max() > 0
    ca = batches["a"].control()
    assert ca.startup_phase == 0 and ca.knownDelay > 0            # past start-up, the delay jump has been followed
    for key in "bcd":
        assert np.array_equal(_bits(outs[key]), _bits(outs["a"])), key
        for s in range(S):
            rep = _state_report(batches[key].export_state(s), batches["a"].export_state(s))
            assert all(v[0] for v in rep.values()), (key, s, {k: v for k, v in rep.items() if not v[0]})
    for s in range(S):
        cd = batches["d"].control_stream(s)
        for name, _t in ca._fields_:
            assert getattr(cd, name) == getattr(ca, name), (s, name)
    for g in batches.values():
        g.close()
