"""The AGC golden runs (tests/golden/make_agc_golden.py): synth arguments, per-frame events and snapshot
frames.  Shared by the golden writer and the tests, so both replay the same call sequence.

Per frame a run calls AddFarend (runs with a far end), then AddMic (mode 1) or VirtualMic (mode 2) or neither,
then Process; the microphone level is fed back: Process of frame f + 1 gets the level frame f returned
(VirtualMic keeps getting the run's start level, the static physical level; Process gets what VirtualMic
returned)."""
import numpy as np

from audiosignalprocess_amd.synth import agc_frames
from tests.edge_pack import compare_outputs, kept_frames, pack_outputs  # noqa: F401

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

# The edge runs (tests/golden/agc_edges_golden.npz): the same schedule and snapshot conventions; each is there for lines of
# csrc/agc_core.h that no run above reaches (tools/core_branch_report.py agc both).  loop: the programme's first frames
# over and over; "shape": frames [a, b) reshaped by shaped() below.  Snapshots sit on frames where the level steps.
_TWICE = {300: ("level", 5), 301: ("level", 5)}
_TWICE.update({f: ("level", 40) for f in range(520, 600)})
EDGE_RUNS = [
    # a loud talker, held: the outer "too high" step, which shifts where the inner one divides (903, 907, 910), 15 times;
    # a level under minLevel from outside returns -1 (790), then the caller's 150 is taken over; silence from frame 586
    # on, right after a step down left zeroCtrlMax above micVol: ZeroCtrl's raise of 10 % is capped at zeroCtrlMax (855)
    dict(init=(20, 200, 1, 16000), start=190, frames=660, seed=14, level=12000, gaps=False, far=True, shape=[(586, 660, "gain", 0, 1)],
         events={400: ("level", 10), 401: ("level", 150)}, snaps=(254, 400, 401, 541, 585, 640, 659)),
    # a talker a little under the range: the inner "too low" step reads kOffset2 / kSlope2 (927), four times, and
    # exp_curve's 2621 < volume <= 5243 (776); echo = 1 over the second step: the raised level is taken back (951)
    dict(init=(0, 255, 1, 16000), start=100, frames=600, seed=11, level=2500, gaps=False, far=False, echo=(300, 320),
         snaps=(255, 307, 527, 579, 599)),
    # the same from level 30: the first call lifts the level to the 10 % point (794), exp_curve's lowest quarter (776-777)
    dict(init=(0, 255, 1, 16000), start=30, frames=620, seed=12, level=1200, gaps=False, far=False, snaps=(256, 290, 501, 604, 619)),
    # 8 kHz; level 5 from outside, under minOutput: the re-centre (798-800), twice; then 80 frames on which the caller
    # keeps passing 40 whatever comes back: after the step at 536 the same level arrives again (803-804)
    dict(init=(0, 255, 1, 8000), start=60, frames=600, seed=13, level=6000, gaps=False, far=True, events=_TWICE,
         snaps=(276, 300, 301, 520, 536, 537, 599)),
    # the virtual microphone: 30 frames of a +-6 square wave with 17 zero crossings, energy under the limit
    # (lowLevelSignal = 1, 671-672); from 600 on a loud talker with negative excursions only: a negative clip steps the
    # gain down (708-711), every frame or two
    dict(init=(0, 255, 2, 16000), start=127, frames=700, seed=1, level=600, loud=(600, 14000), far=False,
         shape=[(600, 700, "neg", 2, 1), (300, 330, "tick", 9, 6)], snaps=(300, 329, 364, 602, 603, 699)),
    # talk and pauses inside the range for 800 frames: the change to slow mode (935-939) at frame 800
    dict(init=(0, 255, 1, 16000), start=127, frames=820, seed=20, level=9000, loop=110, far=False, snaps=(400, 800, 801, 819)),
    # a faint talker from level 240: the level passes maxAnalog, AddMic's digital gain climbs to the end of its table and
    # micVol meets the maxLevel clamp (953-954); twenty times louder from 600 on: gainTableIdx-- (738-739)
    dict(init=(0, 255, 1, 16000), start=240, frames=860, seed=21, level=1500, loop=110, far=False, shape=[(600, 860, "gain", 20, 1)],
         snaps=(275, 367, 408, 614, 726, 849, 859)),
    # a steady talker: the near-end VAD's long-term deviation stays under 4000 and the slow capacitor does not decay (408-409)
    dict(init=(0, 255, 1, 16000), start=127, frames=600, seed=20, level=3500, loop=80, far=False, snaps=(450, 599)),
    # a talker under the range from level 150: exp_curve's 7864 < volume <= 12124 (773)
    dict(init=(0, 255, 1, 16000), start=150, frames=320, seed=11, level=2500, gaps=False, far=False, snaps=(255, 307, 319)),
]

# two bands: the virtual microphone's clipped frame scales the high band sample by sample with the stepping gain (714)
EDGE_RUNS.append(dict(init=(0, 255, 2, 32000), start=127, frames=640, seed=1, level=600, loud=(600, 14000), far=False,
                      shape=[(600, 640, "neg", 2, 1)], snaps=(364, 602, 603, 639)))

# One run per entry of the "too low" step's tables, from eight start levels that put exp_curve on its indices 0..7.  A
# range of 0..40000 (maxInit 50000: the index changes at 4000, 8000, 12000, 16000, 20000, 24000, 37000) makes
# micVol = weightFIX x level >> 14 move with a change of a few units in an entry.  The first call lifts a level to 4980,
# so index 0 is entered by a level from outside on frame 1.  Runs 10-17: the talker of run 2, whose first step (frame
# 256) is the outer one (kOffset1 / kSlope1).  Runs 18-25: the talker of run 1, whose second step (frame 307) is the
# inner one (kOffset2 / kSlope2, 927), taken from the level its outer step at 255 left: 3060 for index 0.
CURVE_LEVELS = (3000, 6000, 10000, 14000, 18000, 22000, 30000, 38500)
for _seed, _level, _frames, _snaps in ((12, 1200, 275, (256, 257, 274)), (11, 2500, 325, (255, 307, 308, 324))):
    for _start in CURVE_LEVELS:
        _first = 2200 if (_start, _seed) == (3000, 11) else _start
        EDGE_RUNS.append(dict(init=(0, 40000, 1, 16000), start=max(_first, 6000), frames=_frames, seed=_seed, level=_level, gaps=False,
                              far=False, snaps=_snaps, events={1: ("level", _first)} if _first < 6000 else {}))

# (compression, target, limiter, analogTarget) for CalculateGainTable called directly, beyond what set_config lets
# through: diffGain 127 with the limiter on (intPart > 127 at the table's low end, 303: the reference reads past
# kGenFuncTable there, the restatement clamps the index, and the limiter replaces those entries; with the limiter off
# the reference's entry 0 is whatever lies behind its table) and the extremes of what set_config allows.  A diffGain
# outside 0..127 stops the reference's debug build at an assert; the restatement's -1 there has no golden.
EDGE_GRID = [(190, 3, 1, 8), (0, 31, 0, 4), (90, 31, 1, 30), (90, 0, 0, 4)]


# Seeded case: EDGE_RUNS[base] up to frame `at`, the named fields written into the reference's LegacyAgc, then `frames`
# all-zero frames through AddMic and Process.  The reference can hold this state: zeroCtrlMax is the micVol of an
# earlier "too high" or saturation step (analog_agc.c, ProcessAnalog) and the "too low" steps since have lifted
# micVol (93 at frame 610) above it; msZero counts 10 per silent call and is reset above 500, so 480 is one of
# its values.  ZeroCtrl's cap at zeroCtrlMax (855, 1.1 x 93 > 80), which edge run 0 also reaches from Init by its
# input; this case is there for the path of a planted state through ImportState on the GPU.
SEEDED = [dict(base=2, at=610, frames=6, plant=dict(msZero=480, zeroCtrlMax=80))]


def replay_seeded(case, agc, level):
    """The seeded frames on an adapter as replay() takes; level: what the base run's last Process returned."""
    outs, levels, sats, rcs = [], [], [], []
    n = 80 if EDGE_RUNS[case["base"]]["init"][3] == 8000 else 160
    for _ in range(case["frames"]):
        rc, x = agc.add_mic(np.zeros((1, n), np.int16))
        rcs.append(rc)
        rc, y, level, sat = agc.process(x, level, 0)
        rcs.append(rc)
        outs.append(y.reshape(-1))
        levels.append(level)
        sats.append(sat)
    return np.concatenate(outs), np.array(levels, np.int32), np.array(sats, np.uint8), np.array(rcs, np.int32)


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
    out = []
    for f in range(F):
        x = gen[rs[f][0]][f if "loop" not in spec else f % spec["loop"]]   # loop: the first frames over and over, a steady talker
        for a, b, kind, *arg in spec.get("shape", ()):   # frames [a, b) of an edge run, reshaped in integer arithmetic
            if a <= f < b:
                x = shaped(x.astype(np.int64), f * x.shape[1] + np.arange(x.shape[1]), kind, arg)
        out.append((np.ascontiguousarray(x), np.ascontiguousarray(far[rs[f][0]][f]) if spec["far"] else None))
    return out


def shaped(x, t, kind, arg):
    """One frame of a "shape" stretch: x int64 [bands][n] from the synth, t the sample index in the run."""
    if kind == "neg":        # only negative excursions: -|x| * num // den
        y = -np.abs(x) * arg[0] // arg[1]
    elif kind == "gain":     # x * num // den
        y = x * arg[0] // arg[1]
    elif kind == "tick":     # a faint square wave: +-amp, the sign changing every `half` samples
        y = np.where((t // arg[0]) % 2 == 0, arg[1], -arg[1])[None, :] + 0 * x
    else:
        raise ValueError(kind)
    return np.clip(y, -32768, 32767).astype(np.int16)


def replay(spec, agc, stop=None):
    """Drives `agc` through the run.  agc: init(min, max, mode, fs), set_config(t, c, l), far(x) -> rc,
    add_mic(x) -> (rc, x), virtual_mic(x, level) -> (rc, x, level), process(x, level, echo) -> (rc, out, level, sat), snapshot(f).
    Returns (outputs, levels, warnings, return values) as arrays.  stop: the last frame to run (all when None)."""
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
        if f == stop:
            break
    return np.concatenate(outs), np.array(levels, np.int32), np.array(sats, np.uint8), np.array(rcs, np.int32)
