"""Writes tests/golden/nsx_golden.npz and tests/golden/nsx_edges_golden.npz from the reference NSX compiled in place
(oracle/Makefile: _ref/libnsx_ref.so, which build() makes where the reference is present):

    python tests/golden/make_nsx_golden.py [--edges] [--check] [libnsx_ref.so]

Without --edges: the golden runs (tests/nsx_runs.RUNS) into nsx_golden.npz.  With --edges: EDGE_RUNS and the SEEDED
cases into nsx_edges_golden.npz.  --check writes nothing: it regenerates every array and compares it with the
committed file.

Each run drives WebRtcNsx_Create / Init / set_policy / Process through ctypes on inputs from
synth.nsx_frames, following tests/nsx_runs.py.  The golden stores no audio input, only a sha256 of the
regenerated input, and per run every output frame of every band plus, at the run's snapshot frames, every
non-pointer field of NoiseSuppressionFixedC (read through a ctypes struct that mirrors it, pointers
included).  The instance is zeroed after Create, so the fields Init leaves alone are defined.

The edge golden holds the same per run, except that a run longer than 120 frames keeps its output samples only for
the 20 frames from each snapshot on, with a sha256 per block of 50 frames for the whole run (nsx_runs.pack_outputs).
A seeded case (nsx_runs.SEEDED) runs its base run to the frame named, writes the case's histograms into the
reference's struct and into nothing else, runs the case's frames and stores the planted state (sd<k>_in), the
outputs and the state after the last frame (sd<k>_s).  A state of the edge golden is one array, the fields laid
out as AspNsxState (tests/edge_pack.pack_state).
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from audiosignalprocess_amd.nsx import FIELDS, AspNsxState, state_dict  # noqa: E402
from tests import nsx_runs  # noqa: E402
from tests.edge_pack import pack_state  # noqa: E402
from tests.nsx_runs import EDGE_RUNS, RUNS, SEEDED, inputs, schedule  # noqa: E402

DEFAULT_LIB = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libnsx_ref.so")


def ref_struct():
    f = []
    for n, t, k in FIELDS:
        f.append((n, t if k == 1 else t * k))
        if n == "fs":
            f.append(("window", C.c_void_p))
        if n == "denoiseBound":
            f.append(("factor2Table", C.c_void_p))
    f.append(("real_fft", C.c_void_p))
    return type("NoiseSuppressionFixedC", (C.Structure,), {"_fields_": f})


def load(path):
    L = C.CDLL(path)
    P = C.c_void_p
    L.WebRtcNsx_Create.argtypes = [C.POINTER(P)]
    L.WebRtcNsx_Init.argtypes = [P, C.c_uint32]
    L.WebRtcNsx_set_policy.argtypes = [P, C.c_int]
    L.WebRtcNsx_Process.argtypes = [P, P, C.c_int, P]
    L.WebRtcNsx_Process.restype = None
    L.WebRtcNsx_Free.argtypes = [P]
    return L


def process(L, h, xi):
    P = C.c_void_p
    y = np.zeros_like(xi)
    nb = xi.shape[0]
    ip = (P * nb)(*[xi[b].ctypes.data for b in range(nb)])
    op = (P * nb)(*[y[b].ctypes.data for b in range(nb)])
    L.WebRtcNsx_Process(h, ip, nb, op)
    return y


def run(L, Ref, spec, stop=None):
    """Drives one run up to and including frame `stop` (all of it when None).  Returns (handle, outputs per frame,
    sha256 of the input, {(frame, field): array} at the snapshots)."""
    x = inputs(spec)
    h = C.c_void_p()
    assert L.WebRtcNsx_Create(C.byref(h)) == 0
    C.memset(h, 0, C.sizeof(Ref))
    sha = hashlib.sha256()
    outs, snaps = [], {}
    for f, ev in enumerate(schedule(spec)):
        if ev["init"]:
            assert L.WebRtcNsx_Init(h, ev["init"]) == 0
        if ev["mode"] is not None:
            assert L.WebRtcNsx_set_policy(h, ev["mode"]) == 0
        sha.update(x[f].tobytes())
        outs.append(process(L, h, x[f]).reshape(-1))
        if f in spec.get("snaps", ()):
            for n, v in state_dict(Ref.from_address(h.value)).items():
                snaps[(f, n)] = v
        if f == stop:
            break
    return h, outs, np.frombuffer(sha.digest(), np.uint8), snaps


def golden_arrays(L, Ref):
    data = {}
    for i, spec in enumerate(RUNS):
        h, outs, sha, snaps = run(L, Ref, spec)
        L.WebRtcNsx_Free(h)
        for (f, n), v in snaps.items():
            data["r%d_s%d_%s" % (i, f, n)] = v
        data["r%d_sha" % i] = sha
        data["r%d_out" % i] = np.concatenate(outs)
        print("run", i, "done")
    return data


def edge_arrays(L, Ref):
    data = {}
    for i, spec in enumerate(EDGE_RUNS):
        h, outs, sha, snaps = run(L, Ref, spec)
        L.WebRtcNsx_Free(h)
        for f in spec["snaps"]:
            data["e%d_s%d" % (i, f)] = pack_state(AspNsxState, {n: v for (g, n), v in snaps.items() if g == f})
        data["e%d_sha" % i] = sha
        data["e%d_keep" % i], data["e%d_blocks" % i] = nsx_runs.pack_outputs(spec, np.stack(outs))
        print("edge run", i, "done")
    for k, case in enumerate(SEEDED):
        h = run(L, Ref, RUNS[case["base"]], stop=case["at"])[0]
        st = Ref.from_address(h.value)
        nsx_runs.plant(st, case)
        data["sd%d_in" % k] = pack_state(AspNsxState, state_dict(st))
        data["sd%d_out" % k] = np.concatenate([process(L, h, x).reshape(-1) for x in nsx_runs.seeded_inputs(case)])
        data["sd%d_s" % k] = pack_state(AspNsxState, state_dict(st))
        L.WebRtcNsx_Free(h)
        print("seeded case", k, "done")
    return data


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    edges, check = "--edges" in sys.argv, "--check" in sys.argv
    L = load(args[0] if args else DEFAULT_LIB)
    data = (edge_arrays if edges else golden_arrays)(L, ref_struct())
    path = os.path.join(HERE, "nsx_edges_golden.npz" if edges else "nsx_golden.npz")
    if check:
        have = np.load(path)
        bad = sorted(set(have.files) ^ set(data)) + [k for k in data if k in have.files and not (
            have[k].dtype == data[k].dtype and np.array_equal(have[k], data[k]))]
        print("%s: %d arrays regenerated, %d differ" % (os.path.basename(path), len(data), len(bad)))
        if bad:
            raise SystemExit("differing arrays: %r" % bad[:12])
        return
    np.savez_compressed(path, **data)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
