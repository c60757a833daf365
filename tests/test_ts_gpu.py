"""GPU suite of the batched transient suppressor (include/asp_ts.h): the kernel against the golden of the
reference and against the CPU build of the same core (lib/libts_restate.so), bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from audiosignalprocess_amd import ts
from audiosignalprocess_amd.build import LIBDIR
from audiosignalprocess_amd.synth import ts_chunks
from tests.test_ts_host import GOLDEN, SNAP_FIELDS, bits, snapshot
from tests.ts_runs import RUNS, inputs, state_scalars

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return np.array_equal(bits(np.asarray(a)).reshape(-1), bits(np.asarray(b)).reshape(-1))


@pytest.mark.parametrize("r", range(len(RUNS)))
def test_batch_equals_the_golden_and_the_cpu_state(r):
    """A batch of two streams runs the golden run on both: outputs and per-chunk scalars equal the golden's, and
    the full state at the snapshot chunks equals the golden's (which the CPU build equals, test_ts_host.py)."""
    spec = RUNS[r]
    x, det, ref, voice, keys = inputs(spec)
    F, dims = spec["chunks"], (spec["rate"], spec["det_rate"], spec["channels"])
    b = ts.TsBatch(2)
    assert b.initialize(*dims) == 0
    two = lambda a: None if a is None else np.ascontiguousarray(np.stack([a, a], axis=1))  # noqa: E731
    want, want_sc = GOLDEN["r%d_out" % r], GOLDEN["r%d_scalars" % r]
    cuts = sorted(set(f + 1 for f in spec["snaps"]) | {F})   # one launch up to each snapshot chunk
    f0 = 0
    for f1 in cuts:
        sl = slice(f0, f1)
        rc, y, res = b.suppress_frames(two(x)[sl], two(voice)[sl], two(keys)[sl], None if det is None else two(det)[sl],
                                       None if ref is None else two(ref)[sl])
        assert rc == 0 and not res.any()
        for s in range(2):
            bad = np.nonzero((bits(y[:, s]) != bits(want[sl])).reshape(f1 - f0, -1).any(axis=1))[0]
            assert bad.size == 0, "stream %d: outputs differ first at chunk %d" % (s, f0 + bad[0])
        st, buf = b.get_state(1)
        assert np.array_equal(state_scalars(st), want_sc[f1 - 1]), "scalars after chunk %d" % (f1 - 1)
        if f1 - 1 in spec["snaps"]:
            snap = snapshot(st, buf, dims)
            for k in SNAP_FIELDS:
                assert same(snap[k], GOLDEN["r%d_s%d_%s" % (r, f1 - 1, k)]), "state %s at chunk %d" % (k, f1 - 1)
        f0 = f1
    b.close()


def drifting(S, F, rate, seed):
    """Inputs of S streams that drift apart: keys, voice probabilities, one stream with a reference channel."""
    x, ref = ts_chunks(S, F, rate, 1, seed=seed)
    s = np.arange(S)
    f = np.arange(F)[:, None]
    keys = ((f == 1 + s % 3) | (f == 3 + s % 5) | ((f % 17 == 0) & (s % 2 == 0))).astype(np.uint8)
    if S > 1:
        keys[:, S - 1] = 0                                # the last stream never enables detection
    voice = np.where((f + s) % 11 < 3, 0.01, 0.2 + 0.7 * ((s % 7) / 7.0)).astype(np.float32)
    voice[:, s % 4 == 1] = 0.0                            # these go for hard restoration
    present = np.zeros((F, S), np.uint8)
    present[:, S // 2] = 1
    return x, ref, keys, voice, present


@pytest.mark.parametrize("S", (1, 3, 65, 130))
def test_streams_drift_apart_each_against_its_own_cpu_instance(S):
    F, rate = 100, 8000
    x, ref, keys, voice, present = drifting(S, F, rate, seed=20 + S)
    reinit, bad_stream, bad_chunk = S // 3, 0, 40           # stream 0 has suppression enabled at chunk 40
    voice[bad_chunk, bad_stream] = 1.5
    b = ts.TsBatch(S)
    assert b.initialize(rate, rate, 1) == 0
    rc1, y1, res1 = b.suppress_frames(x[:60], voice[:60], keys[:60], reference=ref[:60], present=present[:60])
    assert b.initialize(rate, rate, 1, stream=reinit) == 0
    rc2, y2, res2 = b.suppress_frames(x[60:], voice[60:], keys[60:], reference=ref[60:], present=present[60:])
    assert rc1 == -1 and rc2 == 0
    y, res = np.concatenate([y1, y2]), np.concatenate([res1, res2])
    want_res = np.zeros((F, S), np.int32)
    want_res[bad_chunk, bad_stream] = -1
    assert np.array_equal(res, want_res)
    enabled = []
    for s in range(S):
        cpu = ts.Restate()
        cpu.initialize(rate, rate, 1)
        for f in range(F):
            if f == 60 and s == reinit:
                cpu.initialize(rate, rate, 1)
            if f == bad_chunk and s == bad_stream:
                assert cpu.state.suppression_enabled and cpu.state.detector_smoothed > 0
            rc, w = cpu.suppress(x[f, s], voice[f, s], keys[f, s], reference=ref[f, s] if present[f, s] else None)
            assert rc == res[f, s]
            assert same(w, y[f, s]), "stream %d chunk %d" % (s, f)
        st, buf = b.get_state(s)
        assert bytes(st) == bytes(cpu.state) and same(buf, cpu.buffers), "state of stream %d" % s
        enabled.append(int(st.detection_enabled))
    if S > 1:   # the streams did drift apart: the last one never saw a key, some other is still detecting
        assert any(enabled[:-1]) and enabled[-1] == 0
    b.close()


def test_suppress_frames_equals_single_chunks_and_state_moves_between_batches():
    """SuppressFrames(F = 7) against seven Suppress calls, at 32 kHz stereo; then a stream moves to another batch
    mid-run through GetState / SetState without a differing bit."""
    S, F, rate = 3, 21, 32000
    x, ref = ts_chunks(S, F, rate, 2, seed=31)
    keys = np.zeros((F, S), np.uint8)
    keys[1:4] = 1
    voice = np.full((F, S), 0.4, np.float32)
    a, b, c = ts.TsBatch(S), ts.TsBatch(S), ts.TsBatch(2)
    for q in (a, b, c):
        assert q.initialize(rate, rate, 2) == 0
    ya = np.concatenate([a.suppress_frames(x[f:f + 7], voice[f:f + 7], keys[f:f + 7], reference=ref[f:f + 7])[1]
                         for f in range(0, F, 7)])
    yb = np.concatenate([b.suppress_frames(x[f:f + 1], voice[f:f + 1], keys[f:f + 1], reference=ref[f:f + 1],
                                           single=True)[1] for f in range(F)])
    assert same(ya, yb)
    for s in range(S):
        sa, sb = a.get_state(s), b.get_state(s)
        assert bytes(sa[0]) == bytes(sb[0]) and same(sa[1], sb[1])
    # the move: stream 2 of a fresh run of `a`'s inputs continues as stream 0 of c after chunk 9
    assert a.initialize(rate, rate, 2) == 0
    a.suppress_frames(x[:10], voice[:10], keys[:10], reference=ref[:10])
    st, buf = a.get_state(2)
    assert c.set_state(0, st, buf) == 0
    pick = lambda v: np.ascontiguousarray(np.stack([v[10:, 2], v[10:, 0]], axis=1))  # noqa: E731
    yc = c.suppress_frames(pick(x), pick(voice), pick(keys), reference=pick(ref))[1]
    assert same(yc[:, 0], ya[10:, 2])
    bad = ts.AspTsState.from_buffer_copy(bytes(st))
    bad.num_channels = 1
    assert c.set_state(0, bad, buf) < 0
    for q in (a, b, c):
        q.close()


def test_argument_errors_return_minus_one_and_touch_nothing():
    b = ts.TsBatch(2)
    x = np.zeros((1, 2, 1, 160), np.float32)
    v, k = np.full((1, 2), 0.5, np.float32), np.ones((1, 2), np.uint8)
    assert b.suppress_frames(x, v, k)[0] == -1             # before Initialize
    assert b.initialize(44100, 16000, 1) == -1 and b.initialize(16000, 16000, 0) == -1
    assert b.initialize(16000, 32000, 1) == 0
    assert b.suppress_frames(x, v, k)[0] == -1             # no detection data and a longer detection chunk
    assert b.initialize(16000, 16000, 1) == 0
    assert b.suppress_frames(x, v, k)[0] == 0
    before = [(bytes(s), u.tobytes()) for s, u in (b.get_state(i) for i in range(2))]
    lib, p = b.lib, lambda a: a.ctypes.data  # noqa: E731
    r = np.zeros((1, 2), np.int32)
    for args in ((159, 1, 160), (160, 2, 160), (160, 1, 80)):
        assert lib.AspTsBatch_Suppress(b.h, p(x), args[0], args[1], None, args[2], None, 0, None, p(v), p(k), p(r),
                                       ts.MEM_HOST) == -1
    assert lib.AspTsBatch_Suppress(b.h, None, 160, 1, None, 160, None, 0, None, p(v), p(k), p(r), ts.MEM_HOST) == -1
    assert [(bytes(s), u.tobytes()) for s, u in (b.get_state(i) for i in range(2))] == before
    b.close()


def test_cpp_class_from_a_compiled_client(tmp_path):
    """webrtc::TransientSuppressor (include/webrtc_transient_suppressor.h) driven by tests/ts_client.cpp at 16 kHz
    mono for 520 chunks: enable, hard onset and disable all occur; against the CPU build."""
    exe = str(tmp_path / "ts_client")
    subprocess.run(["g++", "-O1", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "ts_client.cpp"), "-L" + LIBDIR, "-lasp_amd", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    F, rate = 520, 16000
    x, ref = ts_chunks(1, F, rate, 1, seed=77)
    x, ref = x[:, 0], ref[:, 0]
    keys = np.zeros(F, np.uint8)
    keys[[4, 6, 90]] = 1
    voice = np.where((np.arange(F) >= 120) & (np.arange(F) < 260), 0.0, 0.8).astype(np.float32)
    has_ref = (np.arange(F) % 2 == 0).astype(np.uint8)
    with open(tmp_path / "script", "w") as fh:
        fh.write("%d %d 1 %d %d\n" % (rate, rate, F, ref.shape[-1]))
        for f in range(F):
            fh.write("%.9g %d %d\n" % (voice[f], keys[f], has_ref[f]))
    x.tofile(tmp_path / "in.f32")
    ref.tofile(tmp_path / "ref.f32")
    r = subprocess.run([exe, str(tmp_path / "script"), str(tmp_path / "in.f32"), str(tmp_path / "ref.f32"),
                        str(tmp_path / "out.f32"), str(tmp_path / "log")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    log = [int(v) for v in (tmp_path / "log").read_text().split()]
    assert log == [-1, 0] + [0] * F + [-1]
    y = np.fromfile(tmp_path / "out.f32", np.float32).reshape(F, 1, 160)
    cpu, seen = ts.Restate(), set()
    cpu.initialize(rate, rate, 1)
    for f in range(F):
        _, w = cpu.suppress(x[f], voice[f], keys[f], reference=ref[f] if has_ref[f] else None)
        assert same(w, y[f]), "chunk %d" % f
        seen.add((cpu.state.suppression_enabled, cpu.state.use_hard_restoration))
    assert seen == {(0, 0), (1, 0), (1, 1)} and cpu.state.suppression_enabled == 0 and cpu.state.seed != 182


_DEVICE_BUFFERS = """
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
torch.zeros(1).cuda()
from audiosignalprocess_amd.ts import MEM_DEVICE, TsBatch
from audiosignalprocess_amd.synth import ts_chunks
S, F, rate = 5, 12, 48000
x, ref = ts_chunks(S, F, rate, 1, seed=84)
keys = np.zeros((F, S), np.uint8); keys[1:3] = 1
voice = np.full((F, S), 0.3, np.float32); voice[7, 2] = -0.5
a, b = TsBatch(S), TsBatch(S)
for q in (a, b):
    assert q.initialize(rate, rate, 1) == 0
rc, ya, res = a.suppress_frames(x, voice, keys, reference=ref)
assert rc == -1 and res[7, 2] == -1 and res.sum() == -1
xd, rd = torch.from_numpy(x).cuda(), torch.from_numpy(ref).cuda()
kd, vd = torch.from_numpy(keys).cuda(), torch.from_numpy(voice).cuda()
resd = torch.zeros((F, S), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
rc = b.lib.AspTsBatch_SuppressFrames(b.h, F, xd.data_ptr(), 480, 1, None, 480, rd.data_ptr(), 480, None, vd.data_ptr(),
                                     kd.data_ptr(), resd.data_ptr(), MEM_DEVICE)
torch.cuda.synchronize()
assert rc == -1
assert np.array_equal(xd.cpu().numpy().view(np.uint32), ya.view(np.uint32)) and np.array_equal(resd.cpu().numpy(), res)
print("DEVICE_BUFFERS_OK")
"""


def test_host_and_device_buffers_agree():
    """torch tensors as ASP_MEM_DEVICE buffers give what host buffers give (48 kHz, one stream with a voice
    probability out of range on one chunk).  A child process: torch's HIP runtime is initialised before the library
    is loaded."""
    r = subprocess.run([sys.executable, "-c", _DEVICE_BUFFERS % ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_BUFFERS_OK" in r.stdout, r.stdout + r.stderr


def test_second_device_gives_the_same_bytes():
    if ts.device_count() < 2:
        pytest.skip("one HIP device")
    x, ref = ts_chunks(4, 10, 16000, 1, seed=90)
    keys = np.zeros((10, 4), np.uint8)
    keys[0:2] = 1
    voice = np.full((10, 4), 0.5, np.float32)
    a, b = ts.TsBatch(4, device=0), ts.TsBatch(4, device=1)
    hip = C.CDLL("libamdhip64.so")
    cur = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(cur)) == 0
    before = cur.value
    for q in (a, b):
        assert q.initialize(16000, 16000, 1) == 0
    ya, yb = a.suppress_frames(x, voice, keys, reference=ref)[1], b.suppress_frames(x, voice, keys, reference=ref)[1]
    assert same(ya, yb) and bytes(a.get_state(3)[0]) == bytes(b.get_state(3)[0])
    assert hip.hipGetDevice(C.byref(cur)) == 0 and cur.value == before
    a.close()
    b.close()
