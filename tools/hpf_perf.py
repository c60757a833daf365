"""Times one 10 ms step of the high-pass filter and of the level estimator on the GPU (device buffers) next to the
VAD's 16 kHz / 10 ms step at the same stream count, and writes one JSON line per case to profiles/hpf_perf.jsonl.

    timeout 600 python tools/hpf_perf.py [--streams 4096 16384] [--repeats 30]

Cases: the filter at 8 kHz / 80 samples and 16 kHz / 160 samples, one channel; the meter at 160 and 480 samples with
1 and 2 channels; 1 and 100 frames per call.  The batches run on torch's current HIP stream (SetStream), and a call
is timed with device events around it: warm-up calls, then `repeats` timed calls; the step time is the call time / F;
median, min and max over the repeats.  hbm_fraction is the bytes the step must move (2 x 2 x samples per channel-frame
for the filter, 2 x samples for the meter) over the step time, as a fraction of the 8 TB/s HBM peak.  The yardstick
is timed as tools/agc_perf.py times it (host clock between synchronisations); vad_ratio is the step time over it.
Run it under a time limit, as above.
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

HBM_PEAK = 8.0e12   # bytes / s


def timed_host(fn, sync, warm, repeats):
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


def timed_events(fn, warm, repeats):
    """Seconds per call between two device events on the current stream."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[4096, 16384], help="multiples of 256")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpf_perf.jsonl"))
    args = ap.parse_args()
    torch.zeros(1).cuda()
    from audiosignalprocess_amd.hpf import HpfBatch
    from audiosignalprocess_amd.level import LevelBatch
    from audiosignalprocess_amd.synth import vad_frames
    from audiosignalprocess_amd.vad import VadBatch

    # a stream of torch's own: the default stream's handle is NULL, which SetStream takes for "the batch's own stream"
    torch.cuda.set_stream(torch.cuda.Stream())
    cur = torch.cuda.current_stream().cuda_stream
    assert cur
    rows = []
    for S in args.streams:
        F = 20
        x = torch.from_numpy(vad_frames(S, F, 16000, 10)).cuda()
        dec = torch.zeros((F, S), dtype=torch.int8, device="cuda")
        torch.cuda.synchronize()
        v = VadBatch(S, mode=1)
        med, lo, hi = timed_host(lambda: v.process_device(16000, x, dec), v.synchronize, 3, max(5, args.repeats // 3))
        v.close()
        yard = med / F * 1e6
        rows.append(dict(case="vad_16k_10ms_yardstick", streams=S, frames_per_call=F, buffers="device", timing="host",
                         step_us=yard, min_us=lo / F * 1e6, max_us=hi / F * 1e6))
        rng = np.random.default_rng(5)
        for F in (1, 100):
            reps = args.repeats if F == 1 else max(5, args.repeats // 5)
            for rate, n in ((8000, 80), (16000, 160)):
                # 256 distinct streams of speech-level noise, repeated over the batch
                a = np.tile(rng.integers(-8000, 8000, (F, 256, 1, n)).astype(np.int16), (1, S // 256, 1, 1))
                src = torch.from_numpy(a).cuda()
                dst = torch.zeros_like(src)
                b = HpfBatch(S, 1)
                assert b.init(rate) == 0 and b.lib.AspHpfBatch_SetStream(b.h, cur) == 0
                torch.cuda.synchronize()
                med, lo, hi = timed_events(lambda: b.process_device(src.data_ptr(), dst.data_ptr(), F, n), 3, reps)
                step = med / F
                rows.append(dict(case="hpf", fs=rate, samples=n, channels=1, lanes_per_channel=1, streams=S,
                                 frames_per_call=F, buffers="device", timing="events", step_us=step * 1e6,
                                 min_us=lo / F * 1e6, max_us=hi / F * 1e6, vad_ratio=step * 1e6 / yard,
                                 hbm_fraction=2 * 2 * n * S / step / HBM_PEAK, repeats=reps))
                b.close()
            for n, C in ((160, 1), (160, 2), (480, 1), (480, 2)):
                a = np.tile(rng.integers(-8000, 8000, (F, 256, C, n)).astype(np.int16), (1, S // 256, 1, 1))
                src = torch.from_numpy(a).cuda()
                m = LevelBatch(S)
                assert m.lib.AspLevelBatch_SetStream(m.h, cur) == 0
                torch.cuda.synchronize()
                med, lo, hi = timed_events(lambda: m.process_device(src.data_ptr(), F, C, n), 3, reps)
                step = med / F
                rows.append(dict(case="level", samples=n, channels=C, lanes_per_stream=1, streams=S, frames_per_call=F,
                                 buffers="device", timing="events", step_us=step * 1e6, min_us=lo / F * 1e6,
                                 max_us=hi / F * 1e6, vad_ratio=step * 1e6 / yard,
                                 hbm_fraction=2 * n * C * S / step / HBM_PEAK, repeats=reps))
                m.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
