"""Times the batched transient suppressor (include/asp_ts.h) on device buffers: suppression enabled, soft
restoration, mono, each rate, 4096 and 16384 streams, 1 and 100 chunks per call; median wall clock per call between
synchronisations (30 calls at one chunk per call, 6 at 100).  The float NS 16 kHz step is measured in the same
process as the yardstick.  Appends one JSON line per configuration to profiles/ts_perf.jsonl."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

torch.zeros(1).cuda()

from audiosignalprocess_amd.ns import NsBatch  # noqa: E402
from audiosignalprocess_amd.synth import ns_frames, ts_chunks  # noqa: E402
from audiosignalprocess_amd.ts import MEM_DEVICE, TsBatch  # noqa: E402


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
    """The float NS step at 16 kHz, plain launches, device buffers, 60 frames per call (as tools/nsx_perf.py)."""
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
    out = open(os.path.join(ROOT, "profiles", "ts_perf.jsonl"), "a")
    for S in (4096, 16384):
        ns_us = ns_step(S)
        for rate in (8000, 16000, 32000, 48000):
            L = rate // 100
            base = ts_chunks(64, 4, rate, 1, seed=5)[0]
            for F in (1, 100):
                b = TsBatch(S)
                assert b.initialize(rate, rate, 1) == 0
                x = torch.from_numpy(np.ascontiguousarray(np.tile(base, (F // 4 + 1, S // 64, 1, 1))[:F])).cuda()
                keys = torch.ones((F, S), dtype=torch.uint8, device="cuda")
                voice = torch.full((F, S), 0.5, dtype=torch.float32, device="cuda")
                call = lambda: b.lib.AspTsBatch_SuppressFrames(b.h, F, x.data_ptr(), L, 1, None, L, None, 0, None,  # noqa: E731
                                                               voice.data_ptr(), keys.data_ptr(), None, MEM_DEVICE)
                for _ in range(3 if F == 1 else 1):   # keys on every chunk: enabled from the second chunk on
                    assert call() == 0
                us = median_call(call, 30 if F == 1 else 6)
                st = b.get_state(0)[0]
                assert st.suppression_enabled and not st.use_hard_restoration
                rec = dict(module="ts", streams=S, rate=rate, chunks_per_call=F, us_per_call=round(us, 1),
                           us_per_chunk=round(us / F, 2), ns16k_step_us=round(ns_us, 1), ratio_to_ns_step=round(us / F / ns_us, 2))
                print(json.dumps(rec))
                out.write(json.dumps(rec) + "\n")
                out.flush()
                b.close()


if __name__ == "__main__":
    main()
