#!/usr/bin/env python3
"""What a list call of the AEC batch costs next to the per-stream-control calls it replaces (needs an MI355X; run it as
ONE command under its own `timeout`).

4096 streams at 16 kHz, 160 samples, the normal filter, device buffers, every stream primed past start-up.  Each cell
is timed with device events on the batch's stream around a window of calls enqueued back to back, after a warm-up of
the same calls, `--windows` times; a window holds as many calls as fill `--window-ms` of device time (sized from a
pilot of the cell, at least `--calls`).  The median window is reported per call, with the slowest and fastest window
and the host's wall clock around the same window beside it.  What a call costs the HOST -- the control plane of every
listed stream and frame, and the descriptor copy's enqueue -- is measured apart, because inside a window the ring of 4
descriptor slots throttles the enqueue loop to the device's pace: bursts of 3 calls (the ring never wraps) after a
synchronise, host clock around the 3 calls alone, median of 30 bursts, as `host_us_per_api_call`.  A cell whose device
time per call is no larger than that figure is bound by the host.  Cells, all in one run:

  v        20 x (BufferFarend + ProcessV): today's per-stream-control path, forty launches and forty descriptor copies
  run      lock-step Run of 20 frames on a second batch (the hand-off build): context only
  a        the identity list of all streams x 20 frames: the work of `v` in three launches
  b1, b4   1024 random streams of the 4096, 1 and 4 frames each
  c        all streams, counts drawn from {0, 1, 1, 1, 2, 3} (max_frames 3): one jitter-buffer tick

One JSON line per cell goes to --out (default profiles/aec_list_perf.jsonl) and to stdout.  No threshold is set here."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window, at least")
    ap.add_argument("--window-ms", type=float, default=250.0, help="device time a timed window is sized to")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aec_list_perf.jsonl"))
    args = ap.parse_args()

    import torch

    from audiosignalprocess_amd._abi import MEM_DEVICE
    from audiosignalprocess_amd.aec import AecBatch
    from audiosignalprocess_amd.ns import device_count
    from audiosignalprocess_amd.synth import aec_frames

    if device_count() < 1 or not torch.cuda.is_available():
        sys.exit("aec_list_perf: no HIP device (nothing is measured without one)")
    S, F, n = args.streams, 20, 160
    far, near = aec_frames(S, F)
    d_far, d_near = torch.from_numpy(far).cuda(), torch.from_numpy(near).cuda()
    d_out = torch.empty_like(d_near)
    pf, pn, po = d_far.data_ptr(), d_near.data_ptr(), d_out.data_ptr()
    frame_bytes = S * n * 4
    aec, lock = AecBatch(S), AecBatch(S)
    aec.lib.AspAecBatch_GetStream.restype = C.c_void_p
    aec.lib.AspAecBatch_GetStream.argtypes = [C.c_void_p]
    zeros = np.zeros(S, np.int16)
    ident = np.arange(S, dtype=np.int32)
    full = np.full(S, F, np.int32)

    def v_call():
        for f in range(F):
            off = f * frame_bytes
            rc = aec.lib.AspAecBatch_BufferFarend(aec.h, C.c_void_p(pf + off), n, MEM_DEVICE)
            rc |= aec.lib.AspAecBatch_ProcessV(aec.h, C.c_void_p(pn + off), C.c_void_p(po + off), n, zeros.ctypes.data, None,
                                               None, MEM_DEVICE)
            if rc != 0:
                sys.exit("aec_list_perf: BufferFarend / ProcessV failed (%d)" % rc)

    def list_call(streams, counts, max_frames):
        d = zeros[:len(streams)]
        return lambda: aec.run_list_device(streams, counts, pf, pn, po, n, max_frames, d)

    for _ in range(3):  # 60 frames: every stream past start-up, on both batches
        aec.run_list_device(ident, full, pf, pn, po, n, F, zeros)
        lock.run_device(pf, pn, po, n, F)
    aec.synchronize()
    lock.synchronize()
    if any(aec.control_stream(s).startup_phase for s in (0, S // 2, S - 1)) or lock.control().startup_phase:
        sys.exit("aec_list_perf: a stream is still in its start-up phase")

    rng = np.random.RandomState(1)
    quarter = np.sort(rng.choice(S, S // 4, replace=False)).astype(np.int32)
    ragged = rng.choice(np.array([0, 1, 1, 1, 2, 3], np.int32), S).astype(np.int32)
    cells = [
        ("v", aec, F, S * F, 2 * F, v_call),
        ("run", lock, F, S * F, 1, lambda: lock.run_device(pf, pn, po, n, F)),
        ("a", aec, F, S * F, 1, list_call(ident, full, F)),
        ("b1", aec, 1, len(quarter), 1, list_call(quarter, np.full(len(quarter), 1, np.int32), 1)),
        ("b4", aec, 4, 4 * len(quarter), 1, list_call(quarter, np.full(len(quarter), 4, np.int32), 4)),
        ("c", aec, 3, int(ragged.sum()), 1, list_call(ident, ragged, 3)),
    ]
    lines = []
    for name, batch, longest, stream_frames, api_calls, call in cells:
        stream = torch.cuda.ExternalStream(batch.lib.AspAecBatch_GetStream(batch.h))
        for _ in range(max(3, args.calls // 4)):
            call()
        batch.synchronize()
        t0 = time.perf_counter()  # pilot: the window's length
        for _ in range(args.calls):
            call()
        batch.synchronize()
        pilot_us = (time.perf_counter() - t0) * 1e6 / args.calls
        calls = int(min(20000, max(args.calls, args.window_ms * 1e3 / pilot_us)))
        host_us = []  # the host's cost of one call, descriptor ring not wrapped
        for _ in range(30):
            batch.synchronize()
            t0 = time.perf_counter()
            for _ in range(3 if api_calls == 1 else 1):
                call()
            host_us.append((time.perf_counter() - t0) * 1e6 / (3 if api_calls == 1 else 1))
        batch.synchronize()
        ev_us, wall_us = [], []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            for _ in range(calls):
                call()
            e1.record(stream)
            e1.synchronize()
            wall_us.append((time.perf_counter() - t0) * 1e6 / calls)
            ev_us.append(e0.elapsed_time(e1) * 1e3 / calls)
        batch.synchronize()
        us = float(np.median(ev_us))
        lines.append({"tool": "aec_list_perf", "cell": name, "streams": S, "longest_entry_frames": longest,
                      "stream_frames_per_call": stream_frames, "api_calls_per_call": api_calls, "calls_per_window": calls,
                      "windows": args.windows, "us_per_call": round(us, 3), "us_per_call_min": round(float(np.min(ev_us)), 3),
                      "us_per_call_max": round(float(np.max(ev_us)), 3),
                      "us_per_stream_frame": round(us / stream_frames, 5),
                      "host_wall_us_per_call": round(float(np.median(wall_us)), 3),
                      "host_us_per_api_call": round(float(np.median(host_us)) / api_calls, 3)})
    if not torch.isfinite(d_out).all():
        sys.exit("aec_list_perf: non-finite output")
    by = {ln["cell"]: ln for ln in lines}
    for ln in lines:
        ln["v_us_per_call"] = by["v"]["us_per_call"]
        ln["run_us_per_call"] = by["run"]["us_per_call"]
    by["a"]["a_over_v"] = round(by["a"]["us_per_call"] / by["v"]["us_per_call"], 4)
    by["a"]["a_median_within_v_slowest_window"] = bool(by["a"]["us_per_call"] <= by["v"]["us_per_call_max"])
    aec.close()
    lock.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
