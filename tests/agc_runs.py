"""The AGC golden runs (tests/golden/make_agc_golden.py): synth arguments, per-frame events and snapshot
frames.  Shared by the golden writer and the tests, so both replay the same call sequence.

Per frame a run calls AddFarend (runs with a far end), then AddMic (mode 1) or VirtualMic (mode 2) or neither,
then Process; the microphone level is fed back: Process of frame f + 1 gets the level frame f returned
(VirtualMic keeps getting the run's start level, the static physical level; Process gets what VirtualMic
returned)."""
import numpy as np

from audiosignalprocess_amd.synth import agc_frames

BANDS = {8000: 1, 16000: 1, 32000: 2, 48000: 3}

# init: (minLevel, maxLevel, mode, fs); start: the first frame's level; events: {frame: ("config", target,
# compression, limiter) | ("init", min, max, mode, fs) | ("level", v)}; echo: frames [a, b) with echo = 1
RUNS = [
    dict(init=(0, 255, 1, 16000), start=40, frames=620, seed=0, level=9000, far=True, echo=(100, 140), snaps=(20, 300, 619)),
    dict(init=(0, 255, 2, 16000), start=127, frames=700, seed=1, level=600, loud=(600, 14000), far=False,
         snaps=(15, 260, 640, 699)),
    dict(init=(0, 255, 1, 8000), start=200, frames=300, seed=2, level=3000, far=True, snaps=(10, 299)),
    dict(init=(0, 255, 2, 32000), start=127, frames=100, seed=3, level=12000, far=False, snaps=(40, 99)),
    dict(init=(0, 255, 3, 48000), start=100, frames=60, seed=4, level=6000, far=True, snaps=(7, 59),
         events={0: ("config", 6, 30, 0)}),
    dict(init=(0, 255, 0, 16000), start=120, frames=260, seed=5, level=9000, far=False, echo=(10, 40), snaps=(50, 259)),
    dict(init=(0, 255, 2, 8000), start=127, frames=200, seed=6, level=1500, far=True, snaps=(100, 199),
         events={0: ("config", 9, 20, 1)}),
    dict(init=(10, 800, 1, 16000), start=790, frames=440, seed=7, level=500, gaps=False, far=False,
         snaps=(60, 290, 350, 439),
         events={300: ("config", 5, 15, 1), 330: ("init", 0, 255, 2, 16000), 331: ("level", 127),
                 380: ("config", 2, 12, 0), 400: ("init", 0, 100, 1, 32000), 401: ("level", 100)}),
    # 80 dB of fixed gain on a faint input: gains above 2^23, the limiter's / 256 * 253 branch and the gate's >> 8 branch
    dict(init=(0, 255, 3, 16000), start=100, frames=80, seed=9, level=100, shift=75, far=False, snaps=(30, 79),
         events={0: ("config", 0, 80, 1)}),
]


def schedule(spec):
    """Per frame: the list of events before the frame's calls."""
    return [[spec.get("events", {})[f]] if f in spec.get("events", {}) else [] for f in range(spec["frames"])]


def rates(spec):
    """(fs, mode) in force at each frame."""
    fs, mode, out = spec["init"][3], spec["init"][2], []
    for evs in schedule(spec):
        for ev in evs:
            if ev[0] == "init":
                fs, mode = ev[4], ev[3]
        out.append((fs, mode))
    return out


def echo_flags(spec):
    a, b = spec.get("echo", (0, 0))
    return np.array([1 if a <= f < b else 0 for f in range(spec["frames"])], np.int16)


def inputs(spec):
    """Per frame (x int16 [bands][n], far int16 [n] or None): stream 0 of synth.agc_frames at the frame's rate."""
    F = spec["frames"]
    rs = rates(spec)
    gen, far = {}, {}
    for fs in set(r[0] for r in rs):
        n = 80 if fs == 8000 else 160
        gen[fs] = agc_frames(1, F, n, BANDS[fs], seed=spec["seed"], level=spec["level"], gaps=spec.get("gaps", True),
                             shift=spec.get("shift", 0))[:, :, 0]
        far[fs] = agc_frames(1, F, n, 1, seed=spec["seed"] + 100, level=4000, shift=40)[:, 0, 0]
        if "loud" in spec:   # from frame loud[0] on the talker is at level loud[1]
            g2 = agc_frames(1, F, n, BANDS[fs], seed=spec["seed"], level=spec["loud"][1])[:, :, 0]
            gen[fs] = np.concatenate([gen[fs][:spec["loud"][0]], g2[spec["loud"][0]:]])
    return [(np.ascontiguousarray(gen[rs[f][0]][f]), np.ascontiguousarray(far[rs[f][0]][f]) if spec["far"] else None)
            for f in range(F)]


def replay(spec, agc):
    """Drives `agc` through the run.  agc: init(min, max, mode, fs), set_config(t, c, l), far(x) -> rc,
    add_mic(x) -> (rc, x), virtual_mic(x, level) -> (rc, x, level), process(x, level, echo) -> (rc, out, level, sat), snapshot(f).
    Returns (outputs, levels, warnings, return values) as arrays."""
    outs, levels, sats, rcs = [], [], [], []
    rcs.append(agc.init(*spec["init"]))
    level = spec["start"]
    phys = level
    rs = rates(spec)
    echo = echo_flags(spec)
    for f, (x, far) in enumerate(inputs(spec)):
        for ev in schedule(spec)[f]:
            if ev[0] == "config":
                rcs.append(agc.set_config(*ev[1:]))
            elif ev[0] == "init":
                rcs.append(agc.init(*ev[1:]))
            else:
                level = phys = ev[1]
        mode = rs[f][1]
        if far is not None:
            rcs.append(agc.far(far))
        lv = level
        if mode == 1:
            rc, x = agc.add_mic(x)
            rcs.append(rc)
        elif mode == 2:
            rc, x, lv = agc.virtual_mic(x, phys)
            rcs.append(rc)
        rc, y, lo, sat = agc.process(x, lv, int(echo[f]))
        rcs.append(rc)
        outs.append(y.reshape(-1))
        levels.append(lo)
        sats.append(sat)
        if mode != 2:
            level = lo
        agc.snapshot(f)
    return np.concatenate(outs), np.array(levels, np.int32), np.array(sats, np.uint8), np.array(rcs, np.int32)
