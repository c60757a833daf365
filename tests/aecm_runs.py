"""The AECM golden runs (tests/golden/make_aecm_golden.py): synth arguments and per-frame schedules.
Shared by the golden writer and the tests, so both replay the same call sequence."""
import numpy as np

from audiosignalprocess_amd.synth import aecm_pair

# fs, n (samples per call), echoMode, cngMode, clean, frames, synth delay / seed, delay pattern, events
RUNS = [
    dict(fs=8000, n=80, echo=3, cng=1, clean=False, frames=700, delay=30, seed=0, ms="steady"),
    dict(fs=8000, n=160, echo=0, cng=1, clean=True, frames=600, delay=60, seed=1, ms="jitter"),
    dict(fs=16000, n=160, echo=1, cng=0, clean=False, frames=700, delay=50, seed=2, ms="jitter"),
    dict(fs=16000, n=160, echo=2, cng=1, clean=True, frames=600, delay=20, seed=3, ms="steady"),
    dict(fs=16000, n=80, echo=4, cng=1, clean=False, frames=300, delay=10, seed=4, ms="steady"),
    dict(fs=8000, n=80, echo=4, cng=0, clean=True, frames=600, delay=70, seed=5, ms="range"),
    dict(fs=16000, n=160, echo=3, cng=1, clean=False, frames=700, delay=40, seed=6, ms="jump"),
    dict(fs=8000, n=160, echo=3, cng=1, clean=False, frames=600, delay=40, seed=7, ms="steady", events="dry"),
    dict(fs=8000, n=80, echo=3, cng=1, clean=False, frames=700, delay=35, seed=8, ms="steady", events="mid"),
    dict(fs=16000, n=160, echo=3, cng=1, clean=False, frames=300, delay=40, seed=9, ms="steady", events="extreme"),
]


def inputs(spec):
    """far, near, clean as [frames][n] int16 of stream 0 of synth.aecm_pair."""
    far, near, clean = aecm_pair(1, spec["frames"], spec["n"], delay=spec["delay"], seed=spec["seed"])
    far, near, clean = far[:, 0], near[:, 0], clean[:, 0]
    if spec.get("events") == "extreme":
        F, n = far.shape
        t = np.arange(F * n).reshape(F, n)
        sq = np.where((t // 37) % 2 == 0, 32767, -32767).astype(np.int16)
        z = (np.arange(F) // 50) % 3
        far = np.where(z[:, None] == 0, 0, np.where(z[:, None] == 1, sq, far)).astype(np.int16)
        near = np.where(z[:, None] == 0, 0, np.where(z[:, None] == 1, sq, near)).astype(np.int16)
        clean = near.copy()
    return far, near, clean


def schedule(spec):
    """Per frame: dict(ms, far (bool: BufferFarend first), init, config (cng, echo), echo_path)."""
    F = spec["frames"]
    out = []
    for f in range(F):
        ev = dict(far=True, init=None, config=None, echo_path=None)
        p = spec["ms"]
        if p == "steady":
            ms = 40
        elif p == "jitter":
            ms = 40 + (f * 7919 % 23) - 11
        elif p == "range":
            ms = [-20, 40, 520, 60, 900, 30][f % 6] if f % 13 == 0 else 50 + (f % 5)
        else:  # jump: the delay steps from 40 to 300 ms and back
            ms = 300 if 250 <= f < 500 else 40
        ev["ms"] = ms
        if f == 0:
            ev["init"] = spec["fs"]
            ev["config"] = (spec["cng"], spec["echo"])
        e = spec.get("events")
        if e == "dry" and (f % 17 in (3, 4) or 300 <= f < 320):
            ev["far"] = False
        if e == "mid":
            if f == 200:
                ev["echo_path"] = np.arange(65, dtype=np.int16) * 40 + 500
            if f == 300:
                ev["config"] = (0, 1)
            if f == 350:
                ev["config"] = (1, 7)  # echoMode out of range: cngMode is set, the call fails
            if f == 400:
                ev["init"] = 16000  # 8 -> 16 kHz at 80 samples per call
            if f == 500:
                ev["init"] = 8000
        out.append(ev)
    return out
