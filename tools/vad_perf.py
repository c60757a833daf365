"""VAD throughput on device buffers: one JSON line per point (fs, frame length, frames per call, streams).

Each point warms up, then times calls of 100 frames back to back on the batch's stream over a region of at
least --min-seconds (wall clock between two synchronisations of that stream; torch ships its own HIP runtime,
so its events cannot time the library's stream); it reports us per frame step (one frame of every stream), M frames/s
(stream-frames), and the HBM fraction of the algorithmic bytes: int16 input + int8 decisions + int32
levels per stream-frame, plus the 736-byte state read and written once per call.

    python tools/vad_perf.py [--min-seconds 0.5] [--hbm-tbs 8.0]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POINTS = ((16000, 10, 100, 4096), (16000, 10, 100, 16384), (48000, 30, 100, 4096))


def run(fs, ms, F, S, min_seconds, hbm_tbs):
    import torch

    from audiosignalprocess_amd.synth import vad_frames
    from audiosignalprocess_amd.vad import VadBatch

    L = fs * ms // 1000
    x = torch.from_numpy(vad_frames(S, F, fs, ms, seed=1)).to("cuda:0")
    dec = torch.empty((F, S), dtype=torch.int8, device="cuda:0")
    lev = torch.empty((F, S), dtype=torch.int32, device="cuda:0")
    b = VadBatch(S, mode=2)
    torch.cuda.synchronize()
    for _ in range(3):
        b.process_device(fs, x, dec, lev)
    b.synchronize()
    calls, elapsed = 0, 0.0
    while elapsed < min_seconds:
        n = max(1, calls or 4)
        t0 = time.perf_counter()
        for _ in range(n):
            b.process_device(fs, x, dec, lev)
        b.synchronize()
        elapsed += time.perf_counter() - t0
        calls += n
    per_call = elapsed / calls
    us_step = per_call / F * 1e6
    bytes_call = F * S * (2 * L + 1 + 4) + 2 * 736 * S
    return {"metric": "vad", "fs": fs, "frame_ms": ms, "frames_per_call": F, "streams": S, "calls": calls,
            "region_s": round(elapsed, 3), "us_per_frame_step": round(us_step, 3),
            "mframes_per_s": round(S * F / per_call / 1e6, 2),
            "hbm_fraction": round(bytes_call / per_call / (hbm_tbs * 1e12), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="peak HBM bandwidth, TB/s")
    a = ap.parse_args()
    for fs, ms, F, S in POINTS:
        print(json.dumps(run(fs, ms, F, S, a.min_seconds, a.hbm_tbs)), flush=True)


if __name__ == "__main__":
    main()
