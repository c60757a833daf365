"""The resampler on a second GPU: a batch on device 1 gives device 0's bytes and leaves the caller's
current device alone.  Skipped on one-GPU boxes."""
import ctypes as C

import numpy as np
import pytest

from audiosignalprocess_amd.splrs import ResamplerBatch, device_count
from audiosignalprocess_amd.synth import nsx_frames

pytestmark = pytest.mark.gpu


def test_second_device_gives_the_same_bytes():
    if device_count() < 2:
        pytest.skip("one HIP device")
    x = np.ascontiguousarray(nsx_frames(9, 6, 480, 1, seed=90)[:, 0])
    a, b = ResamplerBatch(9, device=0), ResamplerBatch(9, device=1)
    hip = C.CDLL("libamdhip64.so")
    cur = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(cur)) == 0
    before = cur.value
    for q in (a, b):
        assert q.reset(48000, 8000) == 0
    assert np.array_equal(a.push_frames(x), b.push_frames(x))
    assert bytes(a.export_state(8)) == bytes(b.export_state(8))
    assert hip.hipGetDevice(C.byref(cur)) == 0 and cur.value == before
    a.close()
    b.close()
