"""The transient-suppressor golden runs (tests/golden/make_ts_golden.py): synth arguments, key presses, voice
probabilities and snapshot chunks.  Shared by the golden writer and the tests, so both replay the same calls.

keys: chunks with key_pressed; voice: [(first chunk, probability)], each holding until the next entry;
det: "none" (no detection data: the first channel's newest chunk), "copy" (the first channel passed as
detection data) or "own" (a separate signal at the detection rate: seed + 50 of the same generator, whose
clicks fall in the same chunks); ref: the reference channel is passed (a chunk without a click has zero energy
there, which leaves using_reference_ false for that chunk)."""
import numpy as np

from audiosignalprocess_amd.synth import ts_chunks

RUNS = [
    # the long run: enabled by the second keypress, soft restoration, hard restoration from chunk 231 (more than
    # 80 unvoiced chunks), left at 304 (more than 3 voiced ones), disabled 400 chunks after the last key
    dict(rate=8000, det_rate=8000, channels=1, chunks=530, seed=0, keys=(5, 8, 30, 61, 62, 100),
         voice=((0, 0.9), (150, 0.0), (300, 0.9)), det="none", ref=True, snaps=(9, 120, 260, 529)),
    dict(rate=16000, det_rate=16000, channels=1, chunks=130, seed=1, keys=(1, 2, 40, 41), voice=((0, 0.0),),
         det="copy", ref=False, snaps=(3, 129)),
    dict(rate=32000, det_rate=32000, channels=1, chunks=100, seed=2, keys=(0, 1, 50), voice=((0, 0.01), (95, 0.5)),
         det="none", ref=True, snaps=(60, 99)),
    dict(rate=48000, det_rate=48000, channels=1, chunks=100, seed=3, keys=(2, 3), voice=((0, 0.3), (10, 0.0)),
         det="none", ref=True, snaps=(50, 99)),
    dict(rate=48000, det_rate=16000, channels=2, chunks=30, seed=4, keys=(0, 1), voice=((0, 0.6),),
         det="own", ref=False, snaps=(29,)),
    dict(rate=16000, det_rate=16000, channels=2, chunks=50, seed=5, keys=(3, 4, 5), voice=((0, 1.0),),
         det="none", ref=True, snaps=(20, 49)),
]


def inputs(spec):
    """(data [F][C][L], detection [F][D] or None, reference [F][L] or None, voice [F], keys [F])."""
    F = spec["chunks"]
    x, ref = ts_chunks(1, F, spec["rate"], spec["channels"], seed=spec["seed"])
    det = None
    if spec["det"] == "copy":
        det = x[:, 0, 0].copy()
    elif spec["det"] == "own":
        det = ts_chunks(1, F, spec["det_rate"], 1, seed=spec["seed"] + 50)[0][:, 0, 0]
    voice = np.zeros(F, np.float32)
    for start, p in spec["voice"]:
        voice[start:] = p
    keys = np.zeros(F, np.uint8)
    keys[list(spec["keys"])] = 1
    return x[:, 0], det, (ref[:, 0] if spec["ref"] else None), voice, keys


def replay(spec, ts):
    """Drives `ts` through the run.  ts: initialize(rate, det_rate, channels) -> rc, suppress(data [C][L], voice,
    key, detection, reference) -> (rc, data after), scalars() -> 1-D float64 array, snapshot(f).  Returns (outputs
    [F][C][L], scalars [F][k], return values)."""
    x, det, ref, voice, keys = inputs(spec)
    rcs = [ts.initialize(spec["rate"], spec["det_rate"], spec["channels"])]
    outs, scal = [], []
    for f in range(spec["chunks"]):
        rc, y = ts.suppress(x[f], voice[f], keys[f], None if det is None else det[f], None if ref is None else ref[f])
        rcs.append(rc)
        outs.append(y)
        scal.append(ts.scalars())
        if f in spec["snaps"]:
            ts.snapshot(f)
    return np.stack(outs), np.stack(scal), np.array(rcs, np.int32)


# the per-chunk scalars, in the order of scalars()
SCALARS = ("detector_smoothed", "detection_enabled", "suppression_enabled", "use_hard_restoration", "using_reference",
           "keypress_counter", "chunks_since_keypress", "chunks_since_voice_change", "seed")


def state_scalars(st):
    """scalars() of an AspTsState; detector_smoothed as its bit pattern."""
    return np.array([np.float32(st.detector_smoothed).view(np.uint32)] + [int(getattr(st, n)) for n in SCALARS[1:]],
                    np.int64)
