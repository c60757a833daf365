#!/usr/bin/env python3
"""What a list call of the NS batch costs next to the lock-step call (needs an MI355X; run it as ONE command under its
own `timeout`).

4096 streams at 16 kHz, device buffers, every stream primed past start-up.  Each cell is timed with device events on
the batch's stream around a window of calls enqueued back to back, after a warm-up of the same calls, `--windows`
times; a window holds as many calls as fill `--window-ms` of device time (sized from a pilot of the cell, at least
`--calls`).  The median window is reported, per call and per frame step (call time / the longest entry's frames), with
the host's wall clock around the same window beside it.  What a call costs the HOST is measured apart, because inside a
window the ring of 8 list slots throttles the enqueue loop to the device's pace: bursts of 6 calls (the ring never
wraps) after a synchronise, host clock around the 6 calls alone, median of 50 bursts, as `host_us_per_api_call`.  A
cell whose device time per call is no larger than that figure is bound by the host.  Cells, all in one run:

  lockstep   AspNsBatch_AnalyzeProcess of 20 frames (the hand-off build): the step time everything else is set against
  lockstep_walk20, lockstep1   two more forms of the lock-step call, for what bounds (a) and (b): the 20 frames as ONE
             walk per workgroup (SetFlowWalk 20: the list form's shape, with the counters), and a call of one frame
  a          the identity list of all streams x 20 frames: the same work through the list form
  b1, b4     1024 random streams of the 4096, 1 and 4 frames each
  c          all streams, counts drawn from {0, 1, 1, 1, 2, 3} (max_frames 3): one jitter-buffer tick

One JSON line per cell goes to --out (default profiles/ns_list_perf.jsonl) and to stdout.  No threshold is set here."""
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
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window, at least")
    ap.add_argument("--window-ms", type=float, default=250.0, help="device time a timed window is sized to")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ns_list_perf.jsonl"))
    args = ap.parse_args()

    import torch

    from audiosignalprocess_amd.ns import NsBatch, device_count
    from audiosignalprocess_amd.synth import ns_frames

    if device_count() < 1 or not torch.cuda.is_available():
        sys.exit("ns_list_perf: no HIP device (nothing is measured without one)")
    S, F = args.streams, 20
    x = ns_frames(S, F, frame0=50)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.empty_like(d_in)
    ns = NsBatch(S, policy=1)
    ns.lib.AspNsBatch_GetStream.restype = C.c_void_p
    stream = torch.cuda.ExternalStream(ns.lib.AspNsBatch_GetStream(ns.h))
    for _ in range(13):  # 260 frames: past both start-up windows
        ns.analyze_process_device(d_in.data_ptr(), d_out.data_ptr(), F)
    ns.synchronize()

    rng = np.random.RandomState(1)
    ident = np.arange(S, dtype=np.int32)
    quarter = np.sort(rng.choice(S, S // 4, replace=False)).astype(np.int32)
    ragged = rng.choice(np.array([0, 1, 1, 1, 2, 3], np.int32), S).astype(np.int32)
    cells = [
        ("lockstep", F, S * F, lambda: ns.analyze_process_device(d_in.data_ptr(), d_out.data_ptr(), F)),
        ("lockstep_walk20", F, S * F, lambda: ns.analyze_process_device(d_in.data_ptr(), d_out.data_ptr(), F)),
        ("lockstep1", 1, S, lambda: ns.analyze_process_device(d_in.data_ptr(), d_out.data_ptr(), 1)),
        ("a", F, S * F, lambda: ns.analyze_process_list_device(ident, None, d_in.data_ptr(), d_out.data_ptr(), F)),
        ("b1", 1, len(quarter), lambda: ns.analyze_process_list_device(quarter, None, d_in.data_ptr(), d_out.data_ptr(), 1)),
        ("b4", 4, 4 * len(quarter), lambda: ns.analyze_process_list_device(quarter, None, d_in.data_ptr(), d_out.data_ptr(), 4)),
        ("c", 3, int(ragged.sum()), lambda: ns.analyze_process_list_device(ident, ragged, d_in.data_ptr(), d_out.data_ptr(), 3)),
    ]
    lines = []
    for name, longest, stream_steps, call in cells:
        ns.set_flow_walk(F if name == "lockstep_walk20" else 0)
        for _ in range(max(10, args.calls // 4)):
            call()
        ns.synchronize()
        t0 = time.perf_counter()  # pilot: the window's length
        for _ in range(args.calls):
            call()
        ns.synchronize()
        pilot_us = (time.perf_counter() - t0) * 1e6 / args.calls
        calls = int(min(50000, max(args.calls, args.window_ms * 1e3 / pilot_us)))
        host_us = []  # the host's cost of one call, ring not wrapped
        for _ in range(50):
            ns.synchronize()
            t0 = time.perf_counter()
            for _ in range(6):
                call()
            host_us.append((time.perf_counter() - t0) * 1e6 / 6)
        ns.synchronize()
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
        ns.synchronize()
        us = float(np.median(ev_us))
        lines.append({"tool": "ns_list_perf", "cell": name, "streams": S, "longest_entry_frames": longest,
                      "stream_steps_per_call": stream_steps, "calls_per_window": calls, "windows": args.windows,
                      "us_per_call": round(us, 3), "us_per_call_min": round(float(np.min(ev_us)), 3),
                      "us_per_call_max": round(float(np.max(ev_us)), 3), "us_per_frame_step": round(us / longest, 3),
                      "host_wall_us_per_call": round(float(np.median(wall_us)), 3),
                      "host_us_per_api_call": round(float(np.median(host_us)), 3)})
    if not torch.isfinite(d_out).all():
        sys.exit("ns_list_perf: non-finite output")
    base = lines[0]["us_per_frame_step"]
    for ln in lines:
        ln["lockstep_us_per_frame_step"] = base
        ln["call_over_lockstep_step"] = round(ln["us_per_call"] / base, 3)
    ns.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
