"""CPU suite: libasp_amd.so exports every function include/asp_nsx.h declares, the reference's five
WebRtcNsx_* names among them, and refuses to create an instance without a device."""
import ctypes as C

from tests.test_abi import declared_functions


def test_every_declared_symbol_is_exported(built_lib):
    lib = C.CDLL(built_lib)
    names = declared_functions("asp_nsx.h")
    assert len(names) >= 19
    assert [n for n in names if not hasattr(lib, n)] == []


def test_reference_symbol_names_present(built_lib):
    lib = C.CDLL(built_lib)
    for n in ["WebRtcNsx_Create", "WebRtcNsx_Free", "WebRtcNsx_Init", "WebRtcNsx_set_policy", "WebRtcNsx_Process"]:
        assert hasattr(lib, n), n


def test_state_size_matches_the_python_mirror(built_lib):
    from audiosignalprocess_amd import nsx

    assert nsx.load_library().AspNsx_state_size() == C.sizeof(nsx.AspNsxState)
