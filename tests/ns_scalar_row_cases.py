"""Inputs for tests/test_ns_scalar_row_oracle.py (CPU) and tests/test_ns_scalar_row_gpu.py: short runs from an imported
steady-state stream state that move the pair-layout NS frame step's scalar row (ns_layout.h: the per-stream scalars and
the bin-128 row tails) through every way it is read, written and handed from step to step in the hand-off build of
ns_kernels1.hip -- where the float scalars and most row tails live in the wave's LDS image and the integer scalars on
the lanes of a register (ScalarRow).  No tests in here.

A case is a list of operations on a batch of streams that starts from imported states:

    ("run", frames [n][S][160])     n frames in one call; the state of every stream is exported behind it
    ("policy", stream, mode)        set_policy of one stream
    ("init", stream)                Init of one stream (the policy of a fresh stream: mode 0)

`play(engine, case)` drives any engine that has the five methods of the adapters below and returns the outputs and the
exported states.  Every frame is integer valued (float-S16 rounded), so one oracle run serves the float and the int16
entry points."""
import ctypes as C

import numpy as np

from tests import ns_cases

S = 5              # two workgroups of the one-stream-per-wave kernel: the second has one live wave and three that return
BASE_FRAMES = 230  # past both start-up windows (50, 200); the feature window (500 frames) is open


def _frames(n_streams, n, frame0):
    """frames frame0 .. frame0 + n - 1 of the first n_streams signal families of ns_cases (speech bursts, white noise,
    level jumps, a tone, coloured noise, ...: features and priorSpeechProb move, unlike over synth.ns_frames), rounded
    and clipped to int16 values"""
    x = ns_cases.family_frames(frame0 + n)[frame0:, :n_streams]
    x = np.clip(np.rint(x), -32768, 32767).astype(np.float32)
    assert (np.abs(x).max(axis=2) > 0).all()
    return np.ascontiguousarray(x)


def base_states(oracle_cls, mode, n_streams=S, policy=1):
    """the streams' states after BASE_FRAMES frames from Init, in the association `mode`"""
    o = oracle_cls(n_streams, policy=policy, reduce_mode=mode)
    o.run(_frames(n_streams, BASE_FRAMES, 0), threads=n_streams)
    return [o.export_state(s) for s in range(n_streams)]


def uneven_calls(base):
    """40 frames in calls of 1, 2, 7, 13 and 17: walks end at odd places, the state is exported behind every call"""
    x = _frames(len(base), 40, BASE_FRAMES)
    ops, f0 = [], 0
    for n in (1, 2, 7, 13, 17):
        ops.append(("run", x[f0:f0 + n]))
        f0 += n
    return [ns_cases.copy_state(b) for b in base], ops


ZERO_FRAMES = (7, 8, 11, 12, 15, 16, 22, 23)   # stream 1: digital silence in these frames of a 24-frame call
ZERO_STEPS = (8, 12, 16, 23)                   # ... whose second frame of each pair is a zero-energy step (the first
#                                                still has the 96 carried samples).  Walks of 8 start at 0, 8, 16: step 8
#                                                and 16 are a walk's first, 12 a middle one, 23 a last; walks of 3 start
#                                                at 0, 3, ..: 8 and 23 are a walk's last, 12 a first, 16 a middle one


def zero_energy(base):
    x = _frames(len(base), 24, BASE_FRAMES)
    for f in ZERO_FRAMES:
        x[f, 1] = 0.0
    return [ns_cases.copy_state(b) for b in base], [("run", x)]


def generic_inside_walk(base):
    """Generic steps inside a walk, steady ones behind them in the same walk (one call of 16 frames, walks of 8 start at
    steps 0 and 8).  Stream 0: tracker 1 enters with its counter at 197, so steps 0 and 1 are steady, 2 (counter 199)
    and 3 (200: the tracker publishes its quantile) generic, 4.. steady.  Stream 2: a crafted feature window (the
    `peaks_ascending` entry of ns_cases) with 5 frames left: steps 0..2 steady, 3 and 4 generic, the window closes in
    step 4 and rewrites priorModelPars, step 5 is steady and reads them.  Stream 4 (alone in its workgroup): both."""
    table = dict(ns_cases.close_cases(base[2], close_step=5))
    states = [ns_cases.copy_state(b) for b in base]
    states[2] = ns_cases.copy_state(table["peaks_ascending"])
    table4 = dict(ns_cases.close_cases(base[4], close_step=5))
    states[4] = ns_cases.copy_state(table4["peaks_ascending"])
    for s in (0, 4):
        states[s].counter[1] = 197
    return states, [("run", _frames(len(base), 16, BASE_FRAMES))]


def scalars_between_launches(base):
    """set_policy of stream 2 (mode 3: overdrive 1.25, denoiseBound 0.09) and Init of stream 3 between two calls: the
    next walk's first step uses the new scalars"""
    x = _frames(len(base), 18, BASE_FRAMES)
    return [ns_cases.copy_state(b) for b in base], [("run", x[:9]), ("policy", 2, 3), ("init", 3), ("run", x[9:])]


def full_workgroups(base8):
    """8 streams (two full workgroups), 16 frames in one call: streams in different places of their counters"""
    states = [ns_cases.copy_state(b) for b in base8]
    states[1].counter[0] = 196
    states[3].counter[2] = 199
    states[5].modelUpdatePars[3] = 4
    states[6].counter[1] = 198
    states[6].modelUpdatePars[3] = 9
    return states, [("run", _frames(len(base8), 16, BASE_FRAMES))]


def steady_steps(st, live):
    """how many of the stream's next steps take the steady body (NS_STEADY_CONJUNCTS of ns_kernels1.hip), `live` =
    one bool per frame: False for a zero-energy step, which takes neither body.  The scalars move as ns_core.c:1084,
    262-272 and 766-790 move them."""
    bi, upd, cnt = st.blockInd, st.updates, list(st.counter)
    flag, mup1, mup3 = st.modelUpdatePars[0], st.modelUpdatePars[1], st.modelUpdatePars[3]
    steady = 0
    for is_live in live:
        if not is_live:
            continue
        bi += 1
        upd = min(upd + 1, 200)
        steady += (bi > 201 and upd >= 200 and all(0 <= c < 199 for c in cnt) and flag >= 1 and mup3 > 2
                   and st.gainmap == 1)
        cnt = [(0 if c >= 200 else c) + 1 for c in cnt]
        if flag >= 1:
            mup3 -= 1
            if mup3 == 0:
                mup3, flag = mup1, (0 if flag == 1 else flag)
    return steady


def play(engine, case):
    """-> (outputs [F][S][160], [[state of every stream] behind every "run"])"""
    states, ops = case
    for s, st in enumerate(states):
        engine.import_state(s, st)
    ys, exports = [], []
    for op in ops:
        if op[0] == "run":
            ys.append(engine.run(op[1]))
            exports.append([engine.export_state(s) for s in range(len(states))])
        elif op[0] == "policy":
            engine.set_policy_stream(op[1], op[2])
        else:
            engine.init_stream(op[1])
    return np.concatenate(ys), exports


class OracleEngine:
    """tests.oracle_lib.OracleNs behind play()'s five methods"""

    def __init__(self, oracle_cls, n_streams, mode, policy=1):
        self.o = oracle_cls(n_streams, policy=policy, reduce_mode=mode)
        self.import_state, self.export_state = self.o.import_state, self.o.export_state

    def run(self, x):
        return self.o.run(x)

    def set_policy_stream(self, stream, mode):
        self.o.set_policy(mode, stream=stream)

    def init_stream(self, stream):
        assert self.o.lib.asp_ns_oracle_init(C.byref(self.o.states[stream]), 16000) == 0


class RefEngine:
    """tests.oracle_lib.RefNs (the compiled reference) behind the same methods"""

    def __init__(self, ref_cls, n_streams, policy=1):
        self.r = ref_cls(n_streams, policy=policy)
        self.import_state, self.export_state = self.r.import_state, self.r.export_state

    def run(self, x):
        return self.r.run(x)

    def set_policy_stream(self, stream, mode):
        assert self.r.lib.WebRtcNs_set_policy_core(self.r._p(stream), mode) == 0

    def init_stream(self, stream):
        assert self.r.lib.WebRtcNs_InitCore(self.r._p(stream), 16000) == 0
