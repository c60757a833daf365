"""The NSX golden runs (tests/golden/make_nsx_golden.py): synth arguments, per-frame events and snapshot
frames.  Shared by the golden writer and the tests, so both replay the same call sequence."""
import numpy as np

from audiosignalprocess_amd.synth import nsx_frames

BANDS = {8000: 1, 16000: 1, 32000: 2, 48000: 3}

# events: "zeros" / "square" stretches, "quiet" (|x| <= 3), "mid" (set_policy and re-Init mid-run)
RUNS = [
    dict(fs=8000, mode=2, frames=1100, seed=0, snaps=(20, 120, 512, 1024, 1099), events="zeros", level=60),
    dict(fs=16000, mode=1, frames=1100, seed=1, snaps=(30, 150, 512, 1024, 1099), level=60),
    dict(fs=32000, mode=3, frames=206, seed=2, snaps=(10, 100, 205), events="square"),
    dict(fs=48000, mode=0, frames=64, seed=3, snaps=(40, 63), events="zeros"),
    dict(fs=8000, mode=3, frames=212, seed=4, snaps=(5, 60, 211), events="square"),
    dict(fs=16000, mode=0, frames=80, seed=6, snaps=(3, 70, 79), events="quiet"),
    dict(fs=16000, mode=1, frames=232, seed=7, snaps=(45, 120, 150, 199, 231), events="mid"),
]


def schedule(spec):
    """Per frame: dict(init=fs or None, mode=mode or None).  The sample count of a frame follows the rate."""
    out = []
    for f in range(spec["frames"]):
        ev = dict(init=None, mode=None)
        if f == 0:
            ev = dict(init=spec["fs"], mode=spec["mode"])
        if spec.get("events") == "mid":
            if f == 100:
                ev["mode"] = 3
            if f == 130:
                ev["init"] = 8000  # 16 -> 8 kHz; the policy is back to 0
            if f == 140:
                ev["mode"] = 2
            if f == 200:
                ev["init"] = 32000  # 8 -> 32 kHz, two bands from here
                ev["mode"] = 1
            if f == 220:
                ev["mode"] = 0
        out.append(ev)
    return out


def rates(spec):
    """The rate in force at each frame."""
    fs, out = spec["fs"], []
    for ev in schedule(spec):
        fs = ev["init"] or fs
        out.append(fs)
    return out


def inputs(spec):
    """One list entry per frame: int16 [bands][n] of stream 0 of synth.nsx_frames at the frame's rate."""
    F = spec["frames"]
    rs = rates(spec)
    gen = {}
    for fs in set(rs):
        n = 80 if fs == 8000 else 160
        gen[fs] = nsx_frames(1, F, n, BANDS[fs], seed=spec["seed"], level=spec.get("level", 800))[:, :, 0]
    e = spec.get("events")
    out = []
    for f in range(F):
        x = gen[rs[f]][f].copy()
        n = x.shape[1]
        if e == "zeros" and (60 <= f < 70 or 230 <= f < 240 or f < 3):
            x[:] = 0
        if e == "square" and (30 <= f < 45 or 204 <= f < 215):
            t = f * n + np.arange(n)
            x[:] = np.where((t // 37) % 2 == 0, 32767, -32768).astype(np.int16)
        if e == "quiet":
            x = (x.astype(np.int32) % 7 - 3).astype(np.int16)
        out.append(np.ascontiguousarray(x))
    return out
