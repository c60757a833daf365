"""The gain control on a second GPU: a batch on device 1 gives device 0's bytes and leaves the caller's
current device alone.  Skipped on one-GPU boxes."""
import ctypes as C

import numpy as np
import pytest

from audiosignalprocess_amd.agc import AgcBatch, device_count
from audiosignalprocess_amd.synth import agc_frames

pytestmark = pytest.mark.gpu


def test_second_device_gives_the_same_bytes():
    if device_count() < 2:
        pytest.skip("one HIP device")
    x = agc_frames(9, 12, 160, 2, seed=90)
    a, b = AgcBatch(9, device=0), AgcBatch(9, device=1)
    hip = C.CDLL("libamdhip64.so")
    cur = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(cur)) == 0
    before = cur.value
    for q in (a, b):
        assert q.init(0, 255, 1, 32000) == 0 and q.set_mic_level(100) == 0
    ya, yb = a.process_frames(x), b.process_frames(x)
    assert all(np.array_equal(u, v) for u, v in zip(ya, yb))
    assert bytes(a.export_state(8)) == bytes(b.export_state(8))
    assert hip.hipGetDevice(C.byref(cur)) == 0 and cur.value == before
    a.close()
    b.close()
