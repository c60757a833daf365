#!/usr/bin/env python3
"""What a list call of the BT batch costs next to the lock-step calls (needs an MI355X; run it as ONE command under its
own `timeout`).

4096 stream-channels, device buffers, 1024- and 256-sample windows, every stream primed by two macroblocks.  Each cell
is timed with device events on the batch's stream around a window of calls enqueued back to back, after a warm-up of the
same calls, `--windows` times; a window holds as many calls as fill `--window-ms` of device time (sized from a pilot of
the cell, at least `--calls`).  The median window is reported, per call and per macroblock step (call time / the longest
entry's macroblocks), with the host's wall clock around the same window beside it.  What a call costs the HOST is
measured apart, because inside a window the ring of 8 list slots throttles the enqueue loop to the device's pace: bursts
of 6 calls (the ring never wraps) after a synchronise, host clock around the 6 calls alone, median of 50 bursts, as
`host_us_per_api_call`.  A cell whose device time per call is no larger than that figure is bound by the host.  Cells,
per window, all in one run:

  lockstep   AspBtBatch_DenoiseBlocks of 8 macroblocks (the hand-off build): the step time everything else is set against
  lockstep1  one AspBtBatch_Denoise: a launch of one macroblock of every stream
  a          the identity list of all streams x 8 macroblocks: the same work through the list form
  b1, b2     1024 random streams of the 4096, 1 and 2 macroblocks each
  c          512 random streams x 1: one hop tick of a population with evenly spread phases (an eighth of the streams
             complete a macroblock)
  f          AspBtBatch_FlushList of all streams, hops drawn from 0 .. 7

One JSON line per cell goes to --out (default profiles/bt_list_perf.jsonl) and to stdout.  No threshold is set here."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(torch, bt, stream, call, args):
    for _ in range(max(10, args.calls // 4)):
        call()
    bt.synchronize()
    t0 = time.perf_counter()  # pilot: the window's length
    for _ in range(args.calls):
        call()
    bt.synchronize()
    pilot_us = (time.perf_counter() - t0) * 1e6 / args.calls
    calls = int(min(50000, max(args.calls, args.window_ms * 1e3 / pilot_us)))
    host_us = []  # the host's cost of one call, ring not wrapped
    for _ in range(50):
        bt.synchronize()
        t0 = time.perf_counter()
        for _ in range(6):
            call()
        host_us.append((time.perf_counter() - t0) * 1e6 / 6)
    bt.synchronize()
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
    bt.synchronize()
    return calls, ev_us, wall_us, host_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window, at least")
    ap.add_argument("--window-ms", type=float, default=150.0, help="device time a timed window is sized to")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bt_list_perf.jsonl"))
    args = ap.parse_args()

    import torch

    from audiosignalprocess_amd.bt import BtBatch
    from audiosignalprocess_amd.ns import device_count
    from audiosignalprocess_amd.synth import bt_samples

    if device_count() < 1 or not torch.cuda.is_available():
        sys.exit("bt_list_perf: no HIP device (nothing is measured without one)")
    S, K = args.streams, 8
    lines = []
    for win in (1024, 256):
        bt = BtBatch(S, win)
        bt.set_flow(1)
        macro, half = bt.macro, bt.half
        x = bt_samples(S, macro)
        d_in = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x, (K, S, macro)))).cuda()  # [K][S][macro]
        d_out = torch.zeros_like(d_in)  # (list calls leave most of it unwritten)
        pi, po = d_in.data_ptr(), d_out.data_ptr()
        stream = torch.cuda.ExternalStream(bt.lib.AspBtBatch_GetStream(bt.h))
        bt.denoise_blocks_device(pi, po, 2)
        bt.synchronize()

        rng = np.random.RandomState(1)
        ident = np.arange(S, dtype=np.int32)
        quarter = rng.choice(S, S // 4, replace=False).astype(np.int32)
        eighth = rng.choice(S, S // 8, replace=False).astype(np.int32)
        hops = rng.randint(0, 8, S).astype(np.int32)
        cells = [
            ("lockstep", K, S * K, lambda: bt.denoise_blocks_device(pi, po, K)),
            ("lockstep1", 1, S, lambda: bt.denoise_device(pi, po)),
            ("a", K, S * K, lambda: bt.denoise_list_device(ident, None, pi, po, K)),
            ("b1", 1, len(quarter), lambda: bt.denoise_list_device(quarter, None, pi, po, 1)),
            ("b2", 2, 2 * len(quarter), lambda: bt.denoise_list_device(quarter, None, pi, po, 2)),
            ("c", 1, len(eighth), lambda: bt.denoise_list_device(eighth, None, pi, po, 1)),
            ("f", 1, S, lambda: bt.flush_list_device(ident, hops, pi, po, 7)),
        ]
        first = len(lines)
        for name, longest, stream_blocks, call in cells:
            calls, ev_us, wall_us, host_us = measure(torch, bt, stream, call, args)
            us = float(np.median(ev_us))
            lines.append({"tool": "bt_list_perf", "win": win, "cell": name, "streams": S,
                          "longest_entry_macroblocks": longest, "stream_macroblocks_per_call": stream_blocks,
                          "calls_per_window": calls, "windows": args.windows, "us_per_call": round(us, 3),
                          "us_per_call_min": round(float(np.min(ev_us)), 3),
                          "us_per_call_max": round(float(np.max(ev_us)), 3),
                          "us_per_macroblock_step": round(us / longest, 3),
                          "host_wall_us_per_call": round(float(np.median(wall_us)), 3),
                          "host_us_per_api_call": round(float(np.median(host_us)), 3)})
        if not torch.isfinite(d_out).all():
            sys.exit("bt_list_perf: non-finite output")
        base = lines[first]["us_per_macroblock_step"]
        for ln in lines[first:]:
            ln["lockstep_us_per_macroblock_step"] = base
            ln["lockstep1_us_per_call"] = lines[first + 1]["us_per_call"]
            ln["call_over_lockstep_step"] = round(ln["us_per_call"] / base, 3)
        bt.close()
        del d_in, d_out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
