"""CPU suite: libasp_amd.so exports every function include/asp_agc.h declares with the header's prototypes,
the state struct has the ctypes mirror's size, and a batch (and a layer-1 handle) cannot be created without
a device; the layer-1 refusals the header lists that need no device."""
import ctypes as C
import os
import re

import pytest

from tests.test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported(built_lib):
    lib = C.CDLL(built_lib)
    names = declared_functions("asp_agc.h")
    assert len(names) == 33 and all(n.startswith(("AspAgc", "WebRtcAgc_")) for n in names)
    assert sum(n.startswith("WebRtcAgc_") for n in names) == 9
    assert [n for n in names if not hasattr(lib, n)] == []


def test_python_mirror_matches_the_header_prototypes(built_lib):
    from audiosignalprocess_amd import agc

    lib = agc.load_library()
    txt = open(os.path.join(ROOT, "include", "asp_agc.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = dict(re.findall(r"\b((?:AspAgc|WebRtcAgc_)\w+)\s*\(([^;{]*)\)\s*;", txt))
    assert len(protos) == 33
    for name, args in protos.items():
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(getattr(lib, name).argtypes) == n, name
    assert lib.AspAgc_state_size() == C.sizeof(agc.AspAgcState)
    assert C.sizeof(agc.AspAgcState) % 4 == 0 and C.sizeof(agc.WebRtcAgcConfig) == 6


def test_gain_table_entry_point_equals_the_restatement(built_lib):
    import numpy as np

    from audiosignalprocess_amd import agc

    lib = agc.load_library()
    t = np.zeros(32, np.int32)
    assert lib.AspAgc_gain_table(t.ctypes.data, 9, 3, 1, 8) == 0
    assert np.array_equal(t, agc.Restate.gain_table(9, 3, 1, 8)[1]) and 0 < t[0] < t[31]
    assert lib.AspAgc_gain_table(t.ctypes.data, 200, 3, 1, 8) == -1


def test_create_fails_loudly_without_a_device(built_lib):
    from audiosignalprocess_amd import agc

    lib = agc.load_library()
    h = C.c_void_p()
    assert lib.AspAgcBatch_Create(C.byref(h), 0, 0) == -1   # refused before a device is looked at
    assert "num_streams" in lib.AspNs_last_error().decode()
    if agc.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(agc.AspError) as exc:
        agc.AgcBatch(4)
    assert "no HIP device" in str(exc.value)
    assert lib.WebRtcAgc_Create(C.byref(h)) == -1 and not h.value


def test_layer1_refuses_null_handles(built_lib):
    from audiosignalprocess_amd import agc

    lib = agc.load_library()
    lv, sat, cfg = C.c_int32(7), C.c_uint8(7), agc.WebRtcAgcConfig(3, 9, 1)
    assert lib.WebRtcAgc_Create(None) == -1 and lib.WebRtcAgc_Free(None) == -1
    assert lib.WebRtcAgc_Init(None, 0, 255, 1, 16000) == -1
    assert lib.WebRtcAgc_set_config(None, cfg) == -1 and lib.WebRtcAgc_get_config(None, C.byref(cfg)) == -1
    assert lib.WebRtcAgc_AddFarend(None, None, 160) == -1 and lib.WebRtcAgc_AddMic(None, None, 1, 160) == -1
    assert lib.WebRtcAgc_VirtualMic(None, None, 1, 160, 100, C.byref(lv)) == -1
    assert lib.WebRtcAgc_Process(None, None, 1, 160, None, 100, C.byref(lv), 0, C.byref(sat)) == -1
    assert lv.value == 7 and sat.value == 7
