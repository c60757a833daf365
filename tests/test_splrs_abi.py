"""CPU suite: libasp_amd.so exports every function include/asp_resampler.h declares with the header's
prototypes, refuses to create a batch without a device, and include/webrtc_resampler.h compiles on its own."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported(built_lib):
    lib = C.CDLL(built_lib)
    names = declared_functions("asp_resampler.h")
    assert len(names) == 14 and all(n.startswith("AspResampler") for n in names)
    assert [n for n in names if not hasattr(lib, n)] == []


def test_python_mirror_matches_the_header_prototypes(built_lib):
    """Argument counts of the ctypes declarations against the header, and the state struct's size."""
    from audiosignalprocess_amd import splrs

    lib = splrs.load_library()
    txt = open(os.path.join(ROOT, "include", "asp_resampler.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = dict(re.findall(r"\b(AspResampler\w+)\s*\(([^;{]*)\)\s*;", txt))
    assert len(protos) == 14
    for name, args in protos.items():
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(getattr(lib, name).argtypes) == n, name
    assert lib.AspResampler_state_size() == C.sizeof(splrs.AspResamplerState) == 4 * (3 + 96)


def test_create_fails_loudly_without_a_device(built_lib):
    from audiosignalprocess_amd import splrs

    lib = splrs.load_library()
    h = C.c_void_p()
    assert lib.AspResamplerBatch_Create(C.byref(h), 0, 0) == -1   # refused before a device is looked at
    assert "num_streams" in lib.AspNs_last_error().decode()
    if splrs.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(splrs.AspError) as exc:
        splrs.ResamplerBatch(4)
    assert "no HIP device" in str(exc.value)


def test_class_header_compiles_standalone(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "webrtc_resampler.h"\n'
                   "int f() { webrtc::Resampler r; int n = 0; return r.Push(0, 0, 0, 0, n) + r.Insert(0, 0) + r.Pull(0, 0, n)\n"
                   "  + (webrtc::kResamplerSynchronous == 0x10 && webrtc::kResamplerInvalid == 0xff && webrtc::kResamplerMode11To8 == 20 ? 0 : 1); }\n")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
