"""Writes tests/golden/nsx_golden.npz from the reference NSX compiled in place:

    python tests/golden/make_nsx_golden.py <libnsxref.so>

Each run drives WebRtcNsx_Create / Init / set_policy / Process through ctypes on inputs from
synth.nsx_frames, following tests/nsx_runs.py.  The golden stores no audio input, only a sha256 of the
regenerated input, and per run every output frame of every band plus, at the run's snapshot frames, every
non-pointer field of NoiseSuppressionFixedC (read through a ctypes struct that mirrors it, pointers
included).  The instance is zeroed after Create, so the fields Init leaves alone are defined.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from audiosignalprocess_amd.nsx import FIELDS, state_dict  # noqa: E402
from tests.nsx_runs import RUNS, inputs, schedule  # noqa: E402


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


def main():
    L = C.CDLL(sys.argv[1])
    P = C.c_void_p
    L.WebRtcNsx_Create.argtypes = [C.POINTER(P)]
    L.WebRtcNsx_Init.argtypes = [P, C.c_uint32]
    L.WebRtcNsx_set_policy.argtypes = [P, C.c_int]
    L.WebRtcNsx_Process.argtypes = [P, P, C.c_int, P]
    L.WebRtcNsx_Process.restype = None
    L.WebRtcNsx_Free.argtypes = [P]
    Ref = ref_struct()
    data = {}
    for i, spec in enumerate(RUNS):
        x = inputs(spec)
        h = P()
        assert L.WebRtcNsx_Create(C.byref(h)) == 0
        C.memset(h, 0, C.sizeof(Ref))
        sha = hashlib.sha256()
        outs = []
        for f, ev in enumerate(schedule(spec)):
            if ev["init"]:
                assert L.WebRtcNsx_Init(h, ev["init"]) == 0
            if ev["mode"] is not None:
                assert L.WebRtcNsx_set_policy(h, ev["mode"]) == 0
            xi = x[f]
            sha.update(xi.tobytes())
            y = np.zeros_like(xi)
            nb = xi.shape[0]
            ip = (P * nb)(*[xi[b].ctypes.data for b in range(nb)])
            op = (P * nb)(*[y[b].ctypes.data for b in range(nb)])
            L.WebRtcNsx_Process(h, ip, nb, op)
            outs.append(y.reshape(-1))
            if f in spec["snaps"]:
                st = Ref.from_address(h.value)
                for n, v in state_dict(st).items():
                    data["r%d_s%d_%s" % (i, f, n)] = v
        L.WebRtcNsx_Free(h)
        data["r%d_sha" % i] = np.frombuffer(sha.digest(), np.uint8)
        data["r%d_out" % i] = np.concatenate(outs)
        print("run", i, "done")
    np.savez_compressed(os.path.join(HERE, "nsx_golden.npz"), **data)


if __name__ == "__main__":
    main()
