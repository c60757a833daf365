"""Times one 10 ms step of the legacy gain control on the GPU (device buffers, the fused ProcessFrames with
chained levels) next to the VAD's 16 kHz / 10 ms step at the same stream count, and writes one JSON line per
case to profiles/agc_perf.jsonl.

    timeout 600 python tools/agc_perf.py [--streams 4096 16384] [--repeats 30]

Cases: 8 kHz, 16 kHz and 48 kHz (3 bands) in adaptive-digital mode, 16 kHz in adaptive-analog mode; 1 and 100
frames per call.  Per case: warm-up calls, then `repeats` timed calls, each between synchronisations (the call
returns when its frames are done); the step time is the call time / F; median, min and max over the repeats;
vad_ratio is the step time over the yardstick's at that stream count.  Run it under a time limit, as above.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = [("adaptive_digital", 2, 8000, 1), ("adaptive_digital", 2, 16000, 1), ("adaptive_digital", 2, 48000, 3),
         ("adaptive_analog", 1, 16000, 1)]


def timed(fn, sync, warm, repeats):
    for _ in range(warm):
        fn()
    sync()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[4096, 16384], help="multiples of 256")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agc_perf.jsonl"))
    args = ap.parse_args()
    torch.zeros(1).cuda()
    from audiosignalprocess_amd.agc import MEM_DEVICE, AgcBatch, split
    from audiosignalprocess_amd.synth import agc_frames, vad_frames
    from audiosignalprocess_amd.vad import VadBatch

    rows = []
    for S in args.streams:
        F = 20
        x = torch.from_numpy(vad_frames(S, F, 16000, 10)).cuda()
        dec = torch.zeros((F, S), dtype=torch.int8, device="cuda")
        torch.cuda.synchronize()
        v = VadBatch(S, mode=1)
        med, lo, hi = timed(lambda: v.process_device(16000, x, dec), v.synchronize, 3, max(5, args.repeats // 3))
        v.close()
        yard = med / F * 1e6
        rows.append(dict(case="vad_16k_10ms_yardstick", streams=S, frames_per_call=F, buffers="device", step_us=yard,
                         min_us=lo / F * 1e6, max_us=hi / F * 1e6))
        for name, mode, fs, nb in CASES:
            n = 80 if fs == 8000 else 160
            for F in (1, 100):
                # 256 distinct streams, repeated over the batch
                low, high = split(np.tile(agc_frames(256, F, n, nb, seed=5, level=7000), (1, 1, S // 256, 1)))
                low = torch.from_numpy(low).cuda()
                high = torch.from_numpy(high).cuda() if nb > 1 else None
                lo_, ho_ = torch.zeros_like(low), (torch.zeros_like(high) if nb > 1 else None)
                lv = torch.zeros((F, S), dtype=torch.int32, device="cuda")
                sat = torch.zeros((F, S), dtype=torch.uint8, device="cuda")
                b = AgcBatch(S)
                assert b.init(0, 255, mode, fs) == 0 and b.set_mic_level(127) == 0
                torch.cuda.synchronize()
                ptr = lambda t: t.data_ptr() if t is not None else None

                def call():
                    assert b.lib.AspAgcBatch_ProcessFrames(b.h, F, None, ptr(low), ptr(high), ptr(lo_), ptr(ho_), nb, n, None,
                                                           None, ptr(lv), ptr(sat), MEM_DEVICE) == 0

                med, lo, hi = timed(call, lambda: None, 3, args.repeats if F == 1 else max(5, args.repeats // 5))
                rows.append(dict(case="agc", mode=name, fs=fs, bands=nb, streams=S, frames_per_call=F, buffers="device",
                                 step_us=med / F * 1e6, min_us=lo / F * 1e6, max_us=hi / F * 1e6,
                                 vad_ratio=med / F * 1e6 / yard, repeats=args.repeats))
                b.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
