"""The legacy gain control on the GPU: every golden run bit-exact through the batch API (stream 1 of 3,
outputs, levels, warnings, return values, exported state at the snapshots) and through layer 1 from one
compiled C client; 3 / 65 / 130 streams with mixed modes and rates and 4100 streams against the CPU build
stream by stream; the fused ProcessFrames against single-frame calls and against the four single operations;
level chaining, state export / import, per-stream Init and set_config, host against device buffers, in place
against out of place, and the mixed 80 / 160 refusal.  Equality everywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from audiosignalprocess_amd import agc
from audiosignalprocess_amd.agc import OP_BY_MODE, OP_FAR, OP_PROCESS, AgcBatch, Restate, state_dict
from audiosignalprocess_amd.build import LIBDIR
from audiosignalprocess_amd.synth import agc_frames
from tests.agc_runs import RUNS, inputs, replay

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "agc_golden.npz"))
MODES = [(0, 255, 1), (0, 255, 2), (0, 255, 0), (0, 255, 3), (10, 800, 1)]   # (min, max, mode) by stream


def check_run(i, out, levels, sats, rcs):
    want = GOLDEN["r%d_out" % i]
    assert out.shape == want.shape
    diff = np.nonzero(out != want)[0]
    assert diff.size == 0, "first differing output sample %d of %d" % (diff[0], out.size)
    assert np.array_equal(levels, GOLDEN["r%d_level" % i]) and np.array_equal(sats, GOLDEN["r%d_sat" % i])
    assert np.array_equal(rcs, GOLDEN["r%d_rc" % i])


class BatchRun:
    """tests/agc_runs.replay's adapter: the run on stream 1 of a batch of 3 whose streams get the same calls."""

    def __init__(self, i):
        self.b, self.i = AgcBatch(3), i

    def three(self, x):
        return np.ascontiguousarray(np.repeat(x[:, None, :], 3, axis=1))

    def same(self, a):
        assert np.array_equal(a[..., 0, :], a[..., 1, :]) and np.array_equal(a[..., 2, :], a[..., 1, :])

    def init(self, *a):
        return self.b.init(*a)

    def set_config(self, t, c, l):
        return self.b.set_config(t, c, l)

    def far(self, x):
        self.b.add_farend(np.repeat(x[None], 3, axis=0))
        return int(self.b.returns(3)[1])

    def add_mic(self, x):
        y = self.b.add_mic(self.three(x))
        self.same(y)
        return int(self.b.returns(3)[1]), y[:, 1]

    def virtual_mic(self, x, level):
        y, lo = self.b.virtual_mic(self.three(x), np.full(3, level, np.int32))
        self.same(y)
        assert lo[0] == lo[1] == lo[2]
        return int(self.b.returns(3)[1]), y[:, 1], int(lo[1])

    def process(self, x, level, echo):
        y, lo, sat = self.b.process(self.three(x), np.full(3, level, np.int32), np.full(3, echo, np.int16))
        self.same(y)
        assert lo[0] == lo[1] == lo[2] and sat[0] == sat[1] == sat[2]
        return int(self.b.returns(3)[1]), y[:, 1], int(lo[1]), int(sat[1])

    def snapshot(self, f):
        if f in RUNS[self.i]["snaps"]:
            bad = [n for n, v in state_dict(self.b.export_state(1)).items()
                   if not np.array_equal(v, GOLDEN["r%d_s%d_%s" % (self.i, f, n)])]
            assert bad == [], "run %d frame %d: state fields differ: %r" % (self.i, f, bad)
            assert bytes(self.b.export_state(0)) == bytes(self.b.export_state(1)) == bytes(self.b.export_state(2))


@pytest.mark.parametrize("i", range(len(RUNS)))
def test_batch_equals_golden_with_state(i):
    run = BatchRun(i)
    check_run(i, *replay(RUNS[i], run))
    run.b.close()


class Script:
    """Records the run as tests/agc_client.c's script; the levels that steer the run are the golden's."""

    def __init__(self, i, script, samples, want):
        self.i, self.script, self.samples, self.want, self.f = i, script, samples, want, 0
        self.rc = iter(GOLDEN["r%d_rc" % i].tolist())
        self.cur = None

    def init(self, *a):
        self.script.append("I %d %d %d %d" % a)
        self.want.append("I %d" % next(self.rc))
        return 0

    def set_config(self, t, c, l):
        self.script.append("C %d %d %d" % (t, c, l))
        self.want.append("C %d" % next(self.rc))
        return 0

    def far(self, x):
        self.script.append("F %d" % x.size)
        self.samples.append(x)
        self.want.append("F %d" % next(self.rc))
        return 0

    def add_mic(self, x):
        self.script.append("M %d %d" % x.shape)
        self.samples.append(x.reshape(-1))
        self.want.append("M %d" % next(self.rc))
        self.cur = True
        return 0, x

    def virtual_mic(self, x, level):
        self.script.append("V %d %d %d" % (x.shape + (level,)))
        self.samples.append(x.reshape(-1))
        self.want.append(("V %d " % next(self.rc), self.f))
        self.cur = True
        return 0, x, level

    def process(self, x, level, echo):
        if not self.cur:
            self.script.append("L %d %d" % x.shape)
            self.samples.append(x.reshape(-1))
        self.cur = None
        lo, sat = int(GOLDEN["r%d_level" % self.i][self.f]), int(GOLDEN["r%d_sat" % self.i][self.f])
        self.script.append(("P %d %d " % x.shape, self.f, echo))
        self.want.append("P %d %d %d" % (next(self.rc), lo, sat))
        self.f += 1
        return 0, np.zeros(0, np.int16), lo, sat

    def snapshot(self, f):
        pass


def test_layer1_equals_golden_from_a_c_client(tmp_path):
    """Every golden run through WebRtcAgc_* in one compiled client.  The level Process gets in an adaptive-digital
    run is what VirtualMic returned: the client's log has it, and the script is completed from a first pass of
    the CPU build (equal to the golden by tests/test_agc_host.py)."""
    exe = str(tmp_path / "agc_client")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "agc_client.c"), "-L" + LIBDIR, "-lasp_amd", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    from tests.test_agc_host import RestateRun

    script, samples, want, outs = [], [], [], []
    for i, spec in enumerate(RUNS):
        # the levels each Process call was given, from the CPU build's replay
        given = []

        class Spy(RestateRun):
            def process(self, x, level, echo):
                given.append(level)
                return RestateRun.process(self, x, level, echo)

            def virtual_mic(self, x, level):
                r = RestateRun.virtual_mic(self, x, level)
                vm.append(r[2])
                return r

        vm = []
        replay(spec, Spy(GOLDEN, i))
        script.append("N")
        s = Script(i, script, samples, want)
        replay(spec, s)
        vm = iter(vm)
        for k, line in enumerate(script):
            if isinstance(line, tuple):
                script[k] = line[0] + "%d %d" % (given[line[1]], line[2])
        for k, line in enumerate(want):
            if isinstance(line, tuple):
                want[k] = line[0] + "%d" % next(vm)
        outs.append(GOLDEN["r%d_out" % i])
    (tmp_path / "script").write_text("\n".join(script) + "\n")
    np.concatenate(samples).astype(np.int16).tofile(str(tmp_path / "in.i16"))
    r = subprocess.run([exe, str(tmp_path / "script"), str(tmp_path / "in.i16"), str(tmp_path / "out.i16"),
                        str(tmp_path / "log")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    log = (tmp_path / "log").read_text().split("\n")[:-1]
    assert len(log) == len(want)
    bad = [(k, g, w) for k, (g, w) in enumerate(zip(log, want)) if g != w]
    assert bad == [], bad[:5]
    out, ref = np.fromfile(str(tmp_path / "out.i16"), np.int16), np.concatenate(outs)
    assert out.size == ref.size
    diff = np.nonzero(out != ref)[0]
    assert diff.size == 0, "first differing output sample %d of %d" % (diff[0], out.size)


def mixed_batch(S, fs_of):
    """A batch whose stream s has MODES[s % 5], rate fs_of(s), its own config for every third stream."""
    b = AgcBatch(S)
    for s in range(S):
        lo, hi, mode = MODES[s % 5]
        assert b.init(lo, hi, mode, fs_of(s), s) == 0
        if s % 3 == 1:
            assert b.set_config(2 + s % 7, 6 + s % 20, s % 2, s) == 0
        assert b.set_mic_level(127 if mode == 2 else lo + 20 + (s * 13) % (hi - lo - 20), s) == 0
    return b


def restate_stream(s, fs, x, far, echo, F0=0, r=None, level=None):
    """Stream s of mixed_batch on the CPU build through frames x [F][bands][n]: (out, levels, sats, rcs, r, level)."""
    lo, hi, mode = MODES[s % 5]
    if r is None:
        r = Restate()
        assert r.init(lo, hi, mode, fs) == 0
        if s % 3 == 1:
            assert r.set_config(2 + s % 7, 6 + s % 20, s % 2) == 0
        level = 127 if mode == 2 else lo + 20 + (s * 13) % (hi - lo - 20)
    outs, lv, sa, rc = [], [], [], []
    for f in range(x.shape[0]):
        ops = OP_BY_MODE | OP_PROCESS | (OP_FAR if far is not None else 0)
        ret, y, _, out, sat = r.frame(ops, x[f], far=None if far is None else far[f], level_in=level, echo=int(echo[f]))
        outs.append(y)
        lv.append(out)
        sa.append(sat)
        rc.append(ret)
        if mode != 2:
            level = out
    return np.array(outs), np.array(lv, np.int32), np.array(sa, np.uint8), np.array(rc, np.int32), r, level


def audio(S, F, nb, seed, n=160):
    x = agc_frames(S, F, n, nb, seed=seed, level=7000)
    x[:, :, 1::4] //= 12          # every fourth stream is quiet: the loop raises its level
    far = np.ascontiguousarray(agc_frames(S, F, n, 1, seed=seed + 50, level=4000, shift=30)[:, 0])
    echo = ((np.arange(F)[:, None] + np.arange(S)[None, :]) % 11 == 0).astype(np.int16)
    return x, far, echo


@pytest.mark.parametrize("S", [3, 65, 130])
def test_mixed_streams_against_the_restatement(S):
    """Modes, configs and rates (16 / 32 / 48 kHz handed two bands) differ inside every wave; chained levels."""
    F, nb = 70, 2
    fs_of = lambda s: (16000, 32000, 48000)[s % 3]
    x, far, echo = audio(S, F, nb, seed=31)
    b = mixed_batch(S, fs_of)
    y, lv, sat = b.process_frames(x, far=far, echo=echo)
    rc = b.returns(F * S).reshape(F, S)
    for s in range(S):
        o, l, a, r, inst, level = restate_stream(s, fs_of(s), x[:, :, s], far[:, s], echo[:, s])
        assert np.array_equal(o, y[:, :, s]), s
        assert np.array_equal(l, lv[:, s]) and np.array_equal(a, sat[:, s]) and np.array_equal(r, rc[:, s]), s
        assert bytes(b.export_state(s)) == bytes(inst.state), s
        assert b.get_mic_level(s) == level, s
    assert len(set(lv[-1].tolist())) >= 3   # the streams ended at different levels
    b.close()


def test_many_streams_against_the_restatement():
    S, F = 4100, 4
    x, far, echo = audio(S, F, 1, seed=32)
    b = mixed_batch(S, lambda s: 16000)
    y, lv, sat = b.process_frames(x, far=far, echo=echo)
    for s in sorted(set([0, 1, 2, 3, 4, 63, 64, 65, 1234, 2047, 4095, 4096, 4099])):
        o, l, a, r, inst, _ = restate_stream(s, 16000, x[:, :, s], far[:, s], echo[:, s])
        assert np.array_equal(o, y[:, :, s]) and np.array_equal(l, lv[:, s]) and np.array_equal(a, sat[:, s]), s
        assert bytes(b.export_state(s)) == bytes(inst.state), s
    b.close()


@pytest.mark.parametrize("fs,nb", [(8000, 1), (48000, 3)])
def test_process_frames_equals_single_calls_and_single_operations(fs, nb):
    S, n = 5, 80 if fs == 8000 else 160
    x, far, echo = audio(S, 60, nb, seed=33, n=n)
    ref = mixed_batch(S, lambda s: fs)
    want = ref.process_frames(x, far=far, echo=echo)
    for chunks in ([1] * 60, [2] * 30, [7] * 8 + [4], [50, 10]):
        b = mixed_batch(S, lambda s: fs)
        got, f = [], 0
        for k in chunks:
            got.append(b.process_frames(np.ascontiguousarray(x[f:f + k]), far=far[f:f + k], echo=echo[f:f + k]))
            f += k
        for j in range(3):
            assert np.array_equal(np.concatenate([g[j] for g in got]), want[j]), (chunks[0], j)
        for s in range(S):
            assert bytes(b.export_state(s)) == bytes(ref.export_state(s))
        b.close()
    # the four single operations in the reference's order; a batch-wide AddMic / VirtualMic serves only the
    # streams of that mode, so the modes run in batches of their own
    for mode_s in (0, 1, 2):
        lo, hi, mode = MODES[mode_s]
        b, c = AgcBatch(S), AgcBatch(S)
        for q in (b, c):
            assert q.init(lo, hi, mode, fs) == 0 and q.set_mic_level(127 if mode == 2 else 60) == 0
        yc, lc, sc = c.process_frames(x, far=far, echo=echo)
        level = np.full(S, 127 if mode == 2 else 60, np.int32)
        for f in range(60):
            b.add_farend(far[f])
            xi, lv = x[f], level
            if mode == 1:
                xi = b.add_mic(xi)
            if mode == 2:
                xi, lv = b.virtual_mic(xi, level)
            y, lo_, sat = b.process(xi, lv, echo[f])
            assert np.array_equal(y, yc[f]) and np.array_equal(lo_, lc[f]) and np.array_equal(sat, sc[f]), (mode, f)
            if mode != 2:
                level = lo_
        for s in range(S):
            assert bytes(b.export_state(s)) == bytes(c.export_state(s))
        b.close()
        c.close()
    ref.close()


def test_level_chaining_equals_feeding_the_levels_back_by_hand():
    S, F = 6, 80
    x, far, echo = audio(S, F, 1, seed=34)
    a, b = mixed_batch(S, lambda s: 16000), mixed_batch(S, lambda s: 16000)
    ya, la, sa = a.process_frames(x, far=far, echo=echo)
    level = np.array([a_ for a_ in [127 if MODES[s % 5][2] == 2 else MODES[s % 5][0] + 20 + (s * 13) % (MODES[s % 5][1] - MODES[s % 5][0] - 20) for s in range(S)]], np.int32)
    digital = np.array([MODES[s % 5][2] == 2 for s in range(S)])
    for f in range(F):
        y, lo, sat = b.process_frames(np.ascontiguousarray(x[f:f + 1]), far=far[f:f + 1], echo=echo[f:f + 1], level_in=level[None])
        assert np.array_equal(y[0], ya[f]) and np.array_equal(lo[0], la[f]) and np.array_equal(sat[0], sa[f]), f
        level = np.where(digital, level, lo[0]).astype(np.int32)
    assert np.any(la[-1] != la[0])
    a.close()
    b.close()


def test_export_import_and_per_stream_control_leave_neighbours_alone():
    S, F = 4, 90
    x, far, echo = audio(S, F, 1, seed=35)
    a, b = mixed_batch(S, lambda s: 16000), mixed_batch(S, lambda s: 16000)
    a.process_frames(np.ascontiguousarray(x[:40]), far=far[:40], echo=echo[:40])
    # stream s of a continues as stream (s + 1) % S of b
    for s in range(S):
        assert b.import_state((s + 1) % S, a.export_state(s)) == 0
        assert b.set_mic_level(a.get_mic_level(s), (s + 1) % S) == 0
    roll = lambda v, ax: np.ascontiguousarray(np.roll(v, 1, axis=ax))
    ya = a.process_frames(np.ascontiguousarray(x[40:]), far=far[40:], echo=echo[40:])
    yb = b.process_frames(roll(x[40:], 2), far=roll(far[40:], 1), echo=roll(echo[40:], 1))
    assert np.array_equal(roll(ya[0], 2), yb[0]) and np.array_equal(roll(ya[1], 1), yb[1]) and np.array_equal(roll(ya[2], 1), yb[2])
    # InitStream and set_config_stream on stream 2 only
    before = [bytes(a.export_state(s)) for s in range(S)]
    assert a.init(0, 255, 3, 16000, 2) == 0 and a.set_config(7, 25, 0, 2) == 0
    assert a.get_config(2) == (0, (7, 25, 0)) and a.get_config(1)[1] != (7, 25, 0)
    after = [bytes(a.export_state(s)) for s in range(S)]
    assert [after[s] == before[s] for s in range(S)] == [True, True, False, True]
    assert a.set_config(40, 9, 1, 2) == -1 and a.last_error(2) == 18004 and a.last_error(1) == 0
    bad = a.export_state(0)
    bad.Rxx16pos = 10
    assert a.import_state(0, bad) != 0 and bytes(a.export_state(0)) == before[0]
    a.close()
    b.close()


_DEVICE_BUFFERS = """
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
torch.zeros(1).cuda()
from audiosignalprocess_amd.agc import MEM_DEVICE, AgcBatch, split
from audiosignalprocess_amd.synth import agc_frames
S, F, n = 6, 30, 160
x = agc_frames(S, F, n, 3, seed=36, level=7000)
far = np.ascontiguousarray(agc_frames(S, F, n, 1, seed=37, level=4000)[:, 0])
a, b, c = AgcBatch(S), AgcBatch(S), AgcBatch(S)
for q in (a, b, c):
    assert q.init(0, 255, 1, 48000) == 0 and q.init(0, 255, 2, 48000, 3) == 0 and q.set_mic_level(127) == 0
ya, la, sa = a.process_frames(x, far=far)
yc, lc, sc = c.process_frames(x.copy(), far=far, in_place=True)
assert np.array_equal(ya, yc) and np.array_equal(la, lc) and np.array_equal(sa, sc)
low, high = split(x)
t = lambda v: torch.from_numpy(v).cuda()
low, high, fa = t(low), t(high), t(far)
lo, ho = torch.zeros_like(low), torch.zeros_like(high)
lv = torch.zeros((F, S), dtype=torch.int32, device="cuda")
sat = torch.zeros((F, S), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
rc = b.lib.AspAgcBatch_ProcessFrames(b.h, F, fa.data_ptr(), low.data_ptr(), high.data_ptr(), lo.data_ptr(), ho.data_ptr(), 3, n,
                                     None, None, lv.data_ptr(), sat.data_ptr(), MEM_DEVICE)
assert rc == 0
torch.cuda.synchronize()
assert np.array_equal(lo.cpu().numpy(), ya[:, 0]) and np.array_equal(ho.cpu().numpy(), ya[:, 1:])
assert np.array_equal(lv.cpu().numpy(), la) and np.array_equal(sat.cpu().numpy(), sa)
print("DEVICE_BUFFERS_OK")
"""


def test_host_and_device_buffers_agree_and_in_place_equals_out_of_place():
    """torch tensors as ASP_MEM_DEVICE buffers give what host buffers give.  A child process: torch's HIP runtime
    is initialised before the library is loaded, as in bench.py."""
    r = subprocess.run([sys.executable, "-c", _DEVICE_BUFFERS % ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_BUFFERS_OK" in r.stdout, r.stdout + r.stderr


def test_a_call_that_mixes_frame_lengths_is_refused():
    b = AgcBatch(4)
    x = agc_frames(4, 1, 160, 1, seed=38)
    with pytest.raises(agc.AspError):
        b.process_frames(x)  # not initialised
    assert b.init(0, 255, 1, 16000) == 0 and b.init(0, 255, 1, 8000, 2) == 0
    before = [bytes(b.export_state(s)) for s in range(4)]
    with pytest.raises(agc.AspError) as exc:
        b.process_frames(x)
    assert "frame length" in str(exc.value)
    with pytest.raises(agc.AspError):
        b.process_frames(agc_frames(4, 1, 80, 1, seed=38))
    assert [bytes(b.export_state(s)) for s in range(4)] == before
    assert b.init(0, 255, 1, 44100) == -1 and b.init(0, 255, 4, 16000) == -1
    assert [bytes(b.export_state(s)) for s in range(4)] == before
    b.close()
    # layer 1: a call before Init, and num_bands outside 1..3, return -1 and touch nothing
    lib = agc.load_library()
    h = C.c_void_p()
    assert lib.WebRtcAgc_Create(C.byref(h)) == 0
    y = np.full(160, 7, np.int16)
    bands = (C.c_void_p * 4)(*[y.ctypes.data] * 4)
    lv, sat = C.c_int32(5), C.c_uint8(5)
    assert lib.WebRtcAgc_Process(h, bands, 1, 160, bands, 100, C.byref(lv), 0, C.byref(sat)) == -1
    assert lib.WebRtcAgc_AddMic(h, bands, 1, 160) == -1 and lib.WebRtcAgc_AddFarend(h, y.ctypes.data, 160) == -1
    cfg = agc.WebRtcAgcConfig()
    assert lib.WebRtcAgc_get_config(h, C.byref(cfg)) == -1 and lib.WebRtcAgc_Init(h, 0, 255, 1, 44100) == -1
    assert lib.WebRtcAgc_Init(h, 0, 255, 1, 16000) == 0
    assert lib.WebRtcAgc_Process(h, bands, 4, 160, bands, 100, C.byref(lv), 0, C.byref(sat)) == -1
    assert lib.WebRtcAgc_Process(h, bands, 0, 160, bands, 100, C.byref(lv), 0, C.byref(sat)) == -1
    assert lib.WebRtcAgc_Process(h, bands, 1, 80, bands, 100, C.byref(lv), 0, C.byref(sat)) == -1
    assert lib.WebRtcAgc_Process(h, None, 1, 160, bands, 100, C.byref(lv), 0, C.byref(sat)) == -1
    assert np.all(y == 7) and lv.value == 5 and sat.value == 5
    lib.WebRtcAgc_Free(h)
