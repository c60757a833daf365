"""Times the audio buffer's calls on the GPU (device buffers, device events) and writes one JSON line per case to
profiles/ab_perf.jsonl.

    timeout 600 python tools/ab_perf.py [--streams 4096 16384] [--repeats 30]

Each line holds the call's time (median, min, max over the repeats, after warm-up calls), the bytes the operation
must move, computed from the shapes (every sample read once and written once at its own width), and the time of a
device-to-device copy of those bytes taken in the same run on the same stream (a copy of n bytes reads n and writes n,
so the copy is of half the operation's bytes); `copy_ratio`, the call time over that copy, is the honest bound for
these memory-bound kernels.  The batches run on a HIP stream of torch's (SetStream).

Cases: DeinterleaveFrom + InterleaveTo at 16 kHz mono, DeinterleaveFrom at 16 kHz stereo -> mono (the reference has no
InterleaveTo for that geometry); CopyFrom + CopyTo at 48 kHz stereo -> 16 kHz mono -> 48 kHz; the two refreshes of
the int16 / float pair at 160 samples x 2 channels; Split + Merge at 32 and 48 kHz through the buffer and, the same
shape in the same process, alternating with it, AspSplitBatch_Analysis + _Synthesis called directly: `rounds` holds
the per-round medians (buffer, direct, direct on the buffer's own arrays) so that the spread is on the line,
`excess_us` the difference of the first two; the third tells an effect of the arrays' addresses from one of the path.
Run it under a time limit, as above."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed_events(fn, warm, repeats):
    """Seconds per call between two device events on the current stream: (median, min, max)."""
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


def copy_time(nbytes, repeats):
    """A device-to-device copy that moves `nbytes` (reads half, writes half)."""
    src = torch.zeros(max(nbytes // 2, 16), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return timed_events(lambda: dst.copy_(src), 3, repeats)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of buffer / direct band split")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_perf.jsonl"))
    args = ap.parse_args()
    torch.zeros(1).cuda()
    from audiosignalprocess_amd import ab
    from audiosignalprocess_amd._abi import MEM_DEVICE
    from audiosignalprocess_amd.qmf import SplitBatch

    # a stream of torch's own: the default stream's handle is NULL, which SetStream takes for "the batch's own stream"
    torch.cuda.set_stream(torch.cuda.Stream())
    cur = torch.cuda.current_stream().cuda_stream
    assert cur
    rng = np.random.default_rng(5)
    rows = []

    def emit(case, S, t, nbytes, **more):
        med, lo, hi = t
        c = copy_time(nbytes, args.repeats)
        row = dict(case=case, streams=S, buffers="device", timing="events", call_us=med * 1e6, min_us=lo * 1e6,
                   max_us=hi * 1e6, bytes=nbytes, copy_us=c * 1e6, copy_ratio=med / c, repeats=args.repeats)
        row.update(more)
        rows.append(row)
        print(json.dumps(row), flush=True)

    def batch(S, *geom):
        b = ab.AudioBufferBatch(S, *geom)
        b.set_stream(cur)
        return b

    for S in args.streams:
        # DeinterleaveFrom + InterleaveTo, 16 kHz mono: int16 in, int16 planar, int16 out
        x = torch.from_numpy(rng.integers(-8000, 8000, (S, 160)).astype(np.int16)).cuda()
        y = torch.zeros_like(x)
        b = batch(S, 160, 1, 160, 1, 160)

        def io_mono():
            b.deinterleave_device(x.data_ptr())
            b.interleave_device(y.data_ptr())
        emit("deinterleave+interleave_16k_mono", S, timed_events(io_mono, 3, args.repeats), 4 * S * 160 * 2, launches=2)
        b.close()
        # DeinterleaveFrom, 16 kHz stereo -> mono
        x = torch.from_numpy(rng.integers(-8000, 8000, (S, 320)).astype(np.int16)).cuda()
        b = batch(S, 160, 2, 160, 1, 160)
        emit("deinterleave_16k_stereo_to_mono", S, timed_events(lambda: b.deinterleave_device(x.data_ptr()), 3, args.repeats),
             S * (320 + 160) * 2, launches=1)
        # the two refreshes at 160 samples x 2 channels: the non-const float view after an int16 write, and back
        b.close()
        b = batch(S, 160, 2, 160, 2, 160)
        b.deinterleave_device(x.data_ptr())

        def refreshes():
            b.view(ab.VIEW_F)
            b.view(ab.VIEW_I)
        emit("refresh_f+refresh_i_160x2", S, timed_events(refreshes, 3, args.repeats), 2 * S * 2 * 160 * (2 + 4), launches=2)
        b.close()
        # CopyFrom + CopyTo: 48 kHz stereo -> 16 kHz mono -> 48 kHz
        xf = torch.from_numpy(rng.uniform(-1, 1, (S, 2, 480)).astype(np.float32)).cuda()
        yf = torch.zeros((S, 1, 480), dtype=torch.float32, device="cuda")
        b = batch(S, 480, 2, 160, 1, 480)

        def copies():
            b.copy_from_device(xf.data_ptr(), ab.STEREO)
            b.copy_to_device(yf.data_ptr())
        # input, the float view written and read, output; the resamplers' buffers read and written by both calls
        nbytes = S * 4 * (2 * 480 + 160 + 160 + 480 + 2 * (480 + 32) + 2 * (160 + 32))
        emit("copy_from+copy_to_48st_16mono_48", S, timed_events(copies, 3, args.repeats), nbytes, launches=2)
        b.close()
        # Split + Merge through the buffer against AspSplitBatch called directly, alternating
        for P in (320, 480):
            nb = P // 160
            xi = torch.from_numpy(rng.integers(-8000, 8000, (S, 2 * P)).astype(np.int16)).cuda()
            b = batch(S, P, 2, P, 2, P)
            b.deinterleave_device(xi.data_ptr())
            d = SplitBatch(2 * S, nb)
            lib = ab.load_library()
            lib.AspSplitBatch_SetStream.argtypes = [C.c_void_p, C.c_void_p]
            assert lib.AspSplitBatch_SetStream(d.h, cur) == 0
            full = torch.from_numpy(rng.integers(-8000, 8000, (2 * S, P)).astype(np.int16)).cuda()
            bands = torch.zeros((nb, 2 * S, 160), dtype=torch.int16, device="cuda")

            def through():
                b.split()
                b.merge()

            def direct():
                assert lib.AspSplitBatch_Analysis(d.h, full.data_ptr(), bands.data_ptr(), MEM_DEVICE) == 0
                assert lib.AspSplitBatch_Synthesis(d.h, bands.data_ptr(), full.data_ptr(), MEM_DEVICE) == 0
            through()
            own_full, own_bands = b.view(ab.VIEW_I_CONST), b.view(ab.VIEW_I_CONST, 0)   # both sides valid: no launch

            def direct_on_buffer_storage():   # the direct batch on the buffer's own arrays: isolates the addresses
                assert lib.AspSplitBatch_Analysis(d.h, own_full, own_bands, MEM_DEVICE) == 0
                assert lib.AspSplitBatch_Synthesis(d.h, own_bands, own_full, MEM_DEVICE) == 0
            rounds = []
            for _ in range(args.rounds):
                rounds.append(tuple(timed_events(fn, 3, args.repeats)[0] * 1e6 for fn in (through, direct, direct_on_buffer_storage)))
            tb, td = float(np.median([r[0] for r in rounds])), float(np.median([r[1] for r in rounds]))
            spread = float(max(max(r[k] for r in rounds) - min(r[k] for r in rounds) for k in (0, 1)))
            emit("split+merge_%dk_stereo" % (P // 10), S, (tb * 1e-6, min(r[0] for r in rounds) * 1e-6, max(r[0] for r in rounds) * 1e-6),
                 4 * 2 * S * P * 2, direct_us=td, excess_us=tb - td, spread_us=spread,
                 direct_on_buffer_storage_us=float(np.median([r[2] for r in rounds])), rounds=rounds)
            b.close()
            d.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
