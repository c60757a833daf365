"""AECM time per 10 ms step on device buffers: one JSON line per point (fs, frames per call, streams),
appended to profiles/aecm_perf.jsonl.

Each point warms up, then times ProcessFrames calls back to back on the batch's stream over a region of at
least --min-seconds (wall clock between two synchronisations of that stream) and reports us per 10 ms step
(one frame of every stream) and M stream-frames/s.  F = 1 is the single-frame call; F = 100 runs 100
frames per call.

    python tools/aecm_perf.py [--min-seconds 0.5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = [(fs, F, S) for S in (4096, 16384) for fs in (8000, 16000) for F in (1, 100)]


def run(fs, F, S, min_seconds):
    import torch

    from audiosignalprocess_amd import aecm
    from audiosignalprocess_amd.synth import aecm_pair

    n = fs // 100
    far, near, _ = aecm_pair(S, F, n, delay=40, seed=1)
    d_far = torch.from_numpy(far).to("cuda:0")
    d_near = torch.from_numpy(near).to("cuda:0")
    d_out = torch.empty_like(d_near)
    ms = torch.full((F, S), 40, dtype=torch.int16).numpy()
    b = aecm.AecmBatch(S, fs=fs)
    lib = b.lib
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call():
        r = lib.AspAecmBatch_ProcessFrames(b.h, F, p(d_far), p(d_near), None, p(d_out), n,
                                           ms.ctypes.data_as(ctypes.c_void_p), None, 1)
        assert r == 0

    for _ in range(3):
        call()
    b.lib.AspAecmBatch_Synchronize(b.h)
    calls, elapsed = 0, 0.0
    while elapsed < min_seconds:
        k = max(1, calls or 2)
        t0 = time.perf_counter()
        for _ in range(k):
            call()
        b.lib.AspAecmBatch_Synchronize(b.h)
        elapsed += time.perf_counter() - t0
        calls += k
    per_call = elapsed / calls
    b.close()
    return {"metric": "aecm", "fs": fs, "frames_per_call": F, "streams": S, "calls": calls,
            "region_s": round(elapsed, 3), "us_per_10ms_step": round(per_call / F * 1e6, 2),
            "mframes_per_s": round(S * F / per_call / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aecm_perf.jsonl"))
    a = ap.parse_args()
    for fs, F, S in POINTS:
        line = json.dumps(run(fs, F, S, a.min_seconds))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
