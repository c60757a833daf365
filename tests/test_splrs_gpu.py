"""The fixed-point resampler on the GPU: every golden run bit-exact through AspResamplerBatch_* and through
the webrtc::Resampler class (outputs, exported state, return values), every mode at 3 / 65 / 130 streams and
16 -> 48 kHz at 4100 streams against the CPU build stream by stream, PushFrames against single Pushes, state
export / import, ResetStream, host against device buffers, and the overlap refusal.  Equality everywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from audiosignalprocess_amd import splrs
from audiosignalprocess_amd.build import LIBDIR
from audiosignalprocess_amd.splrs import MODES, ResamplerBatch, Restate
from audiosignalprocess_amd.synth import nsx_frames
from tests.splrs_runs import PAIRS, RETURNS, RUNS, SYNC, SYNC_STEREO, inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "splrs_golden.npz"))


def frames(S, F, n, seed):
    """int16 [F][S][n], every stream from its own seed."""
    return np.ascontiguousarray(nsx_frames(S, F, n, 1, seed=seed, level=3000)[:, 0])


def restate_streams(rates, x):
    """x [F][S][n] through one CPU instance per stream: (out [F][S][m], the instances)."""
    F, S, _ = x.shape
    rs = [Restate(*rates) for _ in range(S)]
    out = [[r.push(x[f, s])[1] for s, r in enumerate(rs)] for f in range(F)]
    return np.array(out, np.int16), rs


@pytest.mark.parametrize("i", range(len(RUNS)))
def test_batch_equals_golden_with_state(i):
    """Stream 1 of a batch of 3 follows the run; the exported state at the snapshots equals the reference's."""
    spec = RUNS[i]
    ch = spec.get("channels", 1)
    b = ResamplerBatch(3)
    assert b.reset(spec["rates"][0], spec["rates"][1], ch) == 0
    outs = []
    for f, x in enumerate(inputs(spec)):
        ev = spec.get("events", {}).get(f)
        if ev:
            assert (b.reset if ev[0] == "reset" else b.reset_if_needed)(ev[1], ev[2], ch) == 0
        rc, y = b.push(np.ascontiguousarray(np.repeat(x[None], 3, axis=0)))
        assert rc == 0 and np.array_equal(y[0], y[1]) and np.array_equal(y[2], y[1])
        outs.append(y[1])
        if f in spec["snaps"]:
            for c in range(ch):
                st = b.export_state(1, c)
                assert np.array_equal(st.stages(), GOLDEN["r%d_s%d_c%d" % (i, f, c)]), (i, f, c)
    b.close()
    out, want = np.concatenate(outs), GOLDEN["r%d_out" % i]
    assert out.size == want.size
    diff = np.nonzero(out != want)[0]
    assert diff.size == 0, "first differing output sample %d of %d" % (diff[0], out.size)


def test_class_equals_golden(tmp_path):
    """Every golden run and every recorded return value through webrtc::Resampler (include/webrtc_resampler.h)
    in one compiled client."""
    exe = str(tmp_path / "splrs_client")
    subprocess.run(["g++", "-O1", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "splrs_client.cpp"), "-L" + LIBDIR, "-lasp_amd", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    script, samples, want_log, want_out = [], [], [], []
    for i, spec in enumerate(RUNS):
        typ = SYNC_STEREO if spec.get("channels", 1) == 2 else SYNC
        script.append("R %d %d %d" % (spec["rates"][0], spec["rates"][1], typ))
        want_log.append("R 0")
        for f, x in enumerate(inputs(spec)):
            ev = spec.get("events", {}).get(f)
            if ev:
                script.append("%s %d %d %d" % ("R" if ev[0] == "reset" else "N", ev[1], ev[2], typ))
                want_log.append("%s 0" % ("R" if ev[0] == "reset" else "N"))
            script.append("P %d %d" % (x.size, 12 * x.size))
            samples.append(x)
            n = GOLDEN["r%d_out" % i].size // spec["frames"] if not spec.get("events") else None
            want_log.append(n)
        want_out.append(GOLDEN["r%d_out" % i])
    for name, (reset, n, max_len) in RETURNS.items():
        rc = GOLDEN["ret_" + name]
        script += ["R %d %d %d" % reset, "P %d %d" % (n, max_len)]
        samples.append(np.zeros(n, np.int16))
        want_log += ["R %d" % rc[0], "P %d -7" % rc[1]]
        assert rc[1] == -1
    (tmp_path / "script").write_text("\n".join(script) + "\n")
    np.concatenate(samples).tofile(str(tmp_path / "in.i16"))
    r = subprocess.run([exe, str(tmp_path / "script"), str(tmp_path / "in.i16"), str(tmp_path / "out.i16"),
                        str(tmp_path / "log")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    log = (tmp_path / "log").read_text().split("\n")[:-1]
    assert len(log) == len(want_log)
    for got, want in zip(log, want_log):
        if want is None:
            assert got.startswith("P 0 ")
        elif isinstance(want, str):
            assert got == want
        else:
            assert got == "P 0 %d" % want
    out, want = np.fromfile(str(tmp_path / "out.i16"), np.int16), np.concatenate(want_out)
    assert out.size == want.size
    diff = np.nonzero(out != want)[0]
    assert diff.size == 0, "first differing output sample %d of %d" % (diff[0], out.size)


@pytest.mark.parametrize("S", [3, 65, 130])
@pytest.mark.parametrize("mode", range(len(MODES)))
def test_every_stream_equals_the_cpu_build(S, mode):
    rates = (PAIRS[mode][0] * 1000, PAIRS[mode][1] * 1000)
    x = frames(S, 12, rates[0] // 100, seed=50 + mode)
    b = ResamplerBatch(S)
    assert b.reset(*rates) == 0
    assert b.export_state(0).mode == mode
    y = np.concatenate([b.push_frames(x[:5]), b.push_frames(x[5:])])
    want, rs = restate_streams(rates, x)
    bad = [s for s in range(S) if not np.array_equal(y[:, s], want[:, s])]
    assert bad == [], "streams that differ from the CPU build: %r" % bad[:10]
    for s in range(S):
        assert np.array_equal(b.export_state(s).stages(), rs[s].state.stages()), s
    b.close()


def test_many_streams():
    S, rates = 4100, (16000, 48000)
    x = frames(S, 5, 160, seed=80)
    b = ResamplerBatch(S)
    assert b.reset(*rates) == 0
    y = b.push_frames(x)
    b.close()
    want, _ = restate_streams(rates, x)
    bad = [s for s in range(S) if not np.array_equal(y[:, s], want[:, s])]
    assert bad == [], "streams that differ from the CPU build: %r" % bad[:10]


@pytest.mark.parametrize("rates,ch,ms", [((48000, 8000), 1, 10), ((8000, 44000), 1, 40), ((16000, 48000), 2, 10),
                                         ((32000, 8000), 1, 10)])
def test_push_frames_equals_single_pushes(rates, ch, ms):
    S, F = 5, 7
    x = frames(S, F, rates[0] // 1000 * ms * ch, seed=81)
    a, b = ResamplerBatch(S), ResamplerBatch(S)
    for q in (a, b):
        assert q.reset(rates[0], rates[1], ch) == 0
    ya = np.stack([a.push(x[f])[1] for f in range(F)])
    yb = b.push_frames(x)
    assert np.array_equal(ya, yb)
    for s in range(S):
        for c in range(ch):
            assert bytes(a.export_state(s, c)) == bytes(b.export_state(s, c))
    if ch == 2:   # each channel is a mono stream of its own
        want, _ = restate_streams(rates, np.ascontiguousarray(x[:, :, 1::2]))
        assert np.array_equal(yb[:, :, 1::2], want)
    a.close()
    b.close()


def test_export_import_continues_bit_for_bit():
    S, F, rates = 3, 12, (44000, 16000)
    x = frames(S, F, 440, seed=82)
    a, b = ResamplerBatch(S), ResamplerBatch(S)
    assert a.reset(*rates) == 0 and b.reset(*rates) == 0
    a.push_frames(x[:6])
    for s in range(S):
        assert b.import_state(s, a.export_state(s)) == 0
    assert np.array_equal(a.push_frames(x[6:]), b.push_frames(x[6:]))
    st = a.export_state(0)
    st.mode = 3
    assert b.import_state(0, st) != 0   # another mode's state
    a.close()
    b.close()


def test_reset_stream_inside_a_running_batch():
    S, F, rates, k = 6, 10, (48000, 16000), 4
    x = frames(S, F, 480, seed=83)
    b = ResamplerBatch(S)
    assert b.reset(*rates) == 0
    y0 = b.push_frames(x[:5])
    b.reset_stream(k)
    y1 = b.push_frames(x[5:])
    b.close()
    want, _ = restate_streams(rates, x)
    fresh, _ = restate_streams(rates, x[5:, k:k + 1])
    assert np.array_equal(y0, want[:5])
    assert np.array_equal(y1[:, k], fresh[:, 0]) and not np.array_equal(y1[:, k], want[5:, k])
    others = [s for s in range(S) if s != k]
    assert np.array_equal(y1[:, others], want[5:, others])


def test_return_values_and_the_overlap_refusal():
    b = ResamplerBatch(2)
    lib = b.lib
    x = np.zeros((2, 160), np.int16)
    assert b.push(x, 480)[0] == -1                       # before any Reset
    for name, (reset, n, max_len) in RETURNS.items():
        if reset[2] & 0x0f:
            continue   # an asynchronous type exists in the class only (test_class_equals_golden)
        got = [b.reset(reset[0], reset[1], 2 if reset[2] == SYNC_STEREO else 1),
               b.push(np.zeros((2, n), np.int16), max_len)[0]]
        assert got == list(GOLDEN["ret_" + name]), name
    assert b.reset(16000, 48000) == 0 and b.out_length(160) == 480 and b.out_length(80) == -1
    buf = np.zeros(4096, np.int16)
    k = C.c_int(-5)
    before = bytes(b.export_state(1))
    # out begins inside in: refused, with text, nothing written
    rc = lib.AspResamplerBatch_Push(b.h, buf.ctypes.data, 160, buf.ctypes.data + 2 * 300, 480, C.byref(k), splrs.MEM_HOST)
    assert rc != 0 and "overlap" in lib.AspNs_last_error().decode() and k.value == -5
    assert bytes(b.export_state(1)) == before
    assert b.reset(16000, 48000, 3) == -1 and b.push(x, 480)[0] == -1
    b.close()


_DEVICE_BUFFERS = """
import sys
sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import torch
torch.zeros(1).cuda()
from audiosignalprocess_amd.splrs import MEM_DEVICE, ResamplerBatch
from audiosignalprocess_amd.synth import nsx_frames
S, F, n = 6, 4, 480
x = np.ascontiguousarray(nsx_frames(S, F, n, 1, seed=84)[:, 0])
a, b = ResamplerBatch(S), ResamplerBatch(S)
for q in (a, b):
    assert q.reset(48000, 32000) == 0
ya = a.push_frames(x)
xd = torch.from_numpy(x).cuda()
yd = torch.zeros((F, S, 320), dtype=torch.int16, device="cuda")
torch.cuda.synchronize()
assert b.lib.AspResamplerBatch_PushFrames(b.h, xd.data_ptr(), n, F, yd.data_ptr(), MEM_DEVICE) == 0
torch.cuda.synchronize()
assert np.array_equal(yd.cpu().numpy(), ya)
k = C.c_int(0)
rc = b.lib.AspResamplerBatch_Push(b.h, xd.data_ptr(), n, xd.data_ptr() + 2 * n * S - 2, 320, C.byref(k), MEM_DEVICE)
assert rc != 0 and "overlap" in b.lib.AspNs_last_error().decode()
print("DEVICE_BUFFERS_OK")
"""


def test_host_and_device_buffers_agree():
    """torch int16 tensors as ASP_MEM_DEVICE buffers give what host buffers give, and an overlap of device
    buffers is refused.  A child process: torch's HIP runtime is initialised before the library is loaded."""
    r = subprocess.run([sys.executable, "-c", _DEVICE_BUFFERS % ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_BUFFERS_OK" in r.stdout, r.stdout + r.stderr
