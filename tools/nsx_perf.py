"""Times one 10 ms NSX step on the GPU (device buffers) next to the float NS step at the same stream count,
and appends one JSON line per case to profiles/nsx_perf.jsonl.

    python tools/nsx_perf.py [--streams 4096 16384] [--repeats 30]

Per case: warm-up calls, then `repeats` timed calls of ProcessFrames(F); the step time is the call time / F;
median, min and max over the repeats.  The yardstick is AspNsBatch (float NS, plain launches) in the same run.
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
    ap.add_argument("--streams", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nsx_perf.jsonl"))
    args = ap.parse_args()
    torch.zeros(1).cuda()
    from audiosignalprocess_amd.ns import NsBatch
    from audiosignalprocess_amd.nsx import MEM_DEVICE, NsxBatch
    from audiosignalprocess_amd.synth import ns_frames, nsx_frames

    rows = []
    for S in args.streams:
        # the yardstick: the float NS step, plain launches, 16 kHz
        os.environ["ASP_NS_FLOW"] = "0"
        x = torch.from_numpy(np.ascontiguousarray(ns_frames(S, 60), np.float32)).cuda()
        y = torch.zeros_like(x)
        torch.cuda.synchronize()
        g = NsBatch(S, device=0, policy=1)
        sync = lambda: g.lib.AspNsBatch_Synchronize(g.h)
        for _ in range(5):
            g.analyze_process_device(x.data_ptr(), y.data_ptr(), 60)
        sync()
        med, lo, hi = timed(lambda: g.analyze_process_device(x.data_ptr(), y.data_ptr(), 60), sync, 2, max(5, args.repeats // 3))
        g.close()
        rows.append(dict(case="float_ns_yardstick", fs=16000, streams=S, frames_per_call=60, buffers="device",
                         handoff="off", step_us=med / 60 * 1e6, min_us=lo / 60 * 1e6, max_us=hi / 60 * 1e6))
        for fs, nb in ((8000, 1), (16000, 1), (48000, 3)):
            n = 80 if fs == 8000 else 160
            for F in (1, 100):
                xs = nsx_frames(S, F, n, nb, seed=5)
                low = torch.from_numpy(np.ascontiguousarray(xs[:, 0])).cuda()
                high = torch.from_numpy(np.ascontiguousarray(xs[:, 1:])).cuda() if nb > 1 else None
                lo_o = torch.zeros_like(low)
                hi_o = torch.zeros_like(high) if nb > 1 else None
                b = NsxBatch(S)
                assert b.init(fs) == 0 and b.set_policy(1) == 0
                hp = high.data_ptr() if nb > 1 else None
                hop = hi_o.data_ptr() if nb > 1 else None

                def call():
                    rc = b.lib.AspNsxBatch_ProcessFrames(b.h, F, low.data_ptr(), hp, lo_o.data_ptr(), hop, nb, n, MEM_DEVICE)
                    assert rc == 0

                # 260 frames of history first, so that the steady-state branches are timed
                for _ in range(max(1, 260 // F)):
                    call()
                med, lo, hi = timed(call, lambda: None, 3, args.repeats if F == 1 else max(5, args.repeats // 5))
                rows.append(dict(case="nsx", fs=fs, bands=nb, streams=S, frames_per_call=F, buffers="device",
                                 step_us=med / F * 1e6, min_us=lo / F * 1e6, max_us=hi / F * 1e6, repeats=args.repeats))
                b.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
