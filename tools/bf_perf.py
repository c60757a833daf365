"""Times the batched beamformer (include/asp_bf.h) on device buffers: 2, 4 and 8 microphones, with and without the
high band, 4096 and 16384 streams, 1 and 100 chunks per call; median wall clock per call between synchronisations
(30 calls at one chunk per call, 6 at 100).  The float NS 16 kHz step is measured in the same process as the
yardstick.  Appends one JSON line per configuration to profiles/bf_perf.jsonl."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

torch.zeros(1).cuda()

from audiosignalprocess_amd.bf import MEM_DEVICE, BfBatch, linear_geometry  # noqa: E402
from audiosignalprocess_amd.ns import NsBatch  # noqa: E402
from audiosignalprocess_amd.synth import bf_chunks, ns_frames  # noqa: E402


def median_call(fn, calls):
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return float(np.median(times)) * 1e6


def ns_step(S):
    """The float NS step at 16 kHz, plain launches, device buffers, 60 frames per call (as tools/ts_perf.py)."""
    os.environ["ASP_NS_FLOW"] = "0"
    x = torch.from_numpy(np.ascontiguousarray(ns_frames(S, 60), np.float32)).cuda()
    y = torch.zeros_like(x)
    torch.cuda.synchronize()
    ns = NsBatch(S, device=0, policy=1)
    for _ in range(5):
        ns.analyze_process_device(x.data_ptr(), y.data_ptr(), 60)
    t = median_call(lambda: ns.analyze_process_device(x.data_ptr(), y.data_ptr(), 60), 10) / 60
    ns.close()
    return t


def main():
    out = open(os.path.join(ROOT, "profiles", "bf_perf.jsonl"), "a")
    for S in (4096, 16384):
        ns_us = ns_step(S)
        for M in (2, 4, 8):
            # four chunks of 64 streams with both sources live, tiled over the batch and the call
            base, base_hi = bf_chunks(64, 4, M, seed=5, broadside=((0, 4),), offaxis=((0, 4),), silent=())
            for high in (False, True):
                for F in (1, 100):
                    b = BfBatch(S)
                    assert b.initialize(linear_geometry(M, 0.04)) == 0
                    reps = (F // 4 + 1, S // 64, 1, 1)
                    x = torch.from_numpy(base).cuda().repeat(*reps)[:F].contiguous()
                    hi = torch.from_numpy(base_hi).cuda().repeat(*reps)[:F].contiguous() if high else None
                    y = torch.zeros((F, S, 160), dtype=torch.float32, device="cuda")
                    hy = torch.zeros_like(y) if high else None
                    tp = torch.zeros((F, S), dtype=torch.uint8, device="cuda")
                    call = lambda: b.lib.AspBfBatch_ProcessChunks(  # noqa: E731
                        b.h, F, x.data_ptr(), hi.data_ptr() if high else None, y.data_ptr(),
                        hy.data_ptr() if high else None, tp.data_ptr(), MEM_DEVICE)
                    for _ in range(3 if F == 1 else 1):
                        assert call() == 0
                    assert b.synchronize() == 0
                    # the wall clock must cover the batch's own stream: wait for it inside the timed call
                    us = median_call(lambda: (call(), b.synchronize()), 30 if F == 1 else 6)
                    assert bool(torch.isfinite(y).all())
                    rec = dict(module="bf", streams=S, mics=M, high_band=int(high), chunks_per_call=F,
                               us_per_call=round(us, 1), us_per_chunk=round(us / F, 2), ns16k_step_us=round(ns_us, 1),
                               ratio_to_ns_step=round(us / F / ns_us, 2))
                    print(json.dumps(rec), flush=True)
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
                    b.close()
                    del x, hi, y, hy, tp
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
