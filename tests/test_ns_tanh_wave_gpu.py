"""The pair-layout frame step's tanh (ns_device.h, tanh_f32_via_f64_wave: the small-argument series under a wave-level
branch, the reciprocal of 1 + u refined once) equals (float)tanh((double)x) for EVERY float bit pattern -- the contract
of tanh_f32_via_f64, whose own sweep is in tests/test_ns_gpu.py.  Consecutive patterns share a wave, so the sweep runs
waves that take the series on every lane, on no lane, and -- around +-2^-5 -- on some."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu


def test_tanh_wave_form_exhaustive():
    from audiosignalprocess_amd import ns

    assert ns.device_count() >= 1, "GPU tests need a HIP device"
    lib = ns.load_library()
    lib.AspNs_debug_compare.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.c_float, C.c_int]
    total, examples = 0, []
    step = 1 << 28
    for start in range(0, 1 << 32, step):
        n_bad, bad = C.c_uint32(0), (C.c_uint32 * 64)()
        assert lib.AspNs_debug_compare(23, 3, start, step, C.byref(n_bad), bad, 0.0, 0) == 0
        total += n_bad.value
        examples += list(bad[:min(n_bad.value, 64)])
    assert total == 0, (total, [hex(b) for b in examples[:8]])
    # the seam exists beside the libm form only
    n_bad, bad = C.c_uint32(0), (C.c_uint32 * 64)()
    assert lib.AspNs_debug_compare(23, 12, 0, 256, C.byref(n_bad), bad, 0.0, 0) != 0
