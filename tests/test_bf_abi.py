"""CPU suite: libasp_amd.so exports every function include/asp_bf.h declares with the header's prototypes, the
state struct has the ctypes mirror's size, asp_bf.h compiles as C, tests/bf_client.cpp compiles against
include/webrtc_beamformer.h, and a batch cannot be created without a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def test_every_declared_symbol_is_exported(built_lib):
    lib = C.CDLL(built_lib)
    names = declared_functions("asp_bf.h")
    assert len(names) == 16 and all(n.startswith("AspBf") for n in names)
    assert [n for n in names if not hasattr(lib, n)] == []


def test_python_mirror_matches_the_header_prototypes(built_lib):
    from audiosignalprocess_amd import bf

    lib = bf.load_library()
    txt = open(os.path.join(INCLUDE, "asp_bf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = dict(re.findall(r"\b(AspBf\w+)\s*\(([^;{]*)\)\s*;", txt))
    assert len(protos) == 16
    for name, args in protos.items():
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(getattr(lib, name).argtypes) == n, name
    assert lib.AspBf_state_size() == C.sizeof(bf.AspBfState)
    assert C.sizeof(bf.AspBfState) == 4 * (8 + 2 * 129)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use_bf.c"
    src.write_text('#include "asp_bf.h"\n'
                   "int use(AspBfBatch* b, const float* x, float* y) {\n"
                   "  AspBfState s;\n"
                   "  s.frame_offset = ASP_BF_BUFFER - ASP_BF_CHUNK - 224;\n"
                   "  return AspBfBatch_ProcessChunk(b, x, 0, y, 0, 0, ASP_MEM_HOST) + s.frame_offset;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + INCLUDE, "-c", str(src), "-o",
                    str(tmp_path / "use_bf.o")], check=True)


def test_cpp_client_compiles_against_the_header_only_class(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + INCLUDE, "-c",
                    os.path.join(ROOT, "tests", "bf_client.cpp"), "-o", str(tmp_path / "bf_client.o")], check=True)


def test_create_fails_loudly_without_a_device(built_lib):
    from audiosignalprocess_amd import bf

    lib = bf.load_library()
    h = C.c_void_p()
    assert lib.AspBfBatch_Create(C.byref(h), 0, 0) < 0   # refused before a device is looked at
    assert "num_streams" in lib.AspNs_last_error().decode()
    assert lib.AspBfBatch_Initialize(None, 4, None, 10, 16000) < 0 and lib.AspBfBatch_Free(None) < 0
    assert lib.AspBfBatch_state_floats(None) == -1
    if bf.device_count() > 0:
        return   # the GPU suite covers the rest
    with pytest.raises(bf.AspError) as exc:
        bf.BfBatch(4)
    assert "no HIP device" in str(exc.value)
