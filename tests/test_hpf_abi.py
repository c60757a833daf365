"""CPU suite: libasp_amd.so exports every function include/asp_hpf.h and include/asp_level.h declare with the
headers' prototypes, the state structs have the ctypes mirrors' sizes, a batch (and a layer-1 handle) cannot be
created without a device, the refusals that need no device, and a C++ client of include/webrtc_rms_level.h compiles
and links."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = {"asp_hpf.h": ("AspHpf", 17), "asp_level.h": ("AspLevel", 15)}


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_every_declared_symbol_is_exported(built_lib, header):
    lib = C.CDLL(built_lib)
    prefix, count = HEADERS[header]
    names = declared_functions(header)
    assert len(names) == count and all(n.startswith(prefix) for n in names)
    assert [n for n in names if not hasattr(lib, n)] == []


@pytest.mark.parametrize("header", sorted(HEADERS))
def test_python_mirror_matches_the_header_prototypes(built_lib, header):
    from audiosignalprocess_amd import hpf, level

    lib = hpf.load_library() and level.load_library()
    prefix, count = HEADERS[header]
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = dict(re.findall(r"\b(%s\w+)\s*\(([^;{]*)\)\s*;" % prefix, txt))
    assert len(protos) == count
    for name, args in protos.items():
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(getattr(lib, name).argtypes) == n, name


def test_state_sizes(built_lib):
    from audiosignalprocess_amd import hpf, level

    assert hpf.load_library().AspHpf_state_size() == C.sizeof(hpf.AspHpfState) == 16
    assert level.load_library().AspLevel_state_size() == C.sizeof(level.AspLevelState) == 8
    assert hpf.AspHpfState.coeff_set.offset == 12 and level.AspLevelState.sample_count.offset == 4


def test_create_fails_loudly_without_a_device(built_lib):
    from audiosignalprocess_amd import hpf, level

    lib = level.load_library() and hpf.load_library()
    h = C.c_void_p()
    for args in ((0, 1, 0), (-3, 1, 0), (4, 0, 0)):   # refused before a device is looked at
        assert lib.AspHpfBatch_Create(C.byref(h), *args) == -1 and not h.value
        assert "num_streams" in lib.AspNs_last_error().decode()
    for n in (0, -1):
        assert lib.AspLevelBatch_Create(C.byref(h), n, 0) == -1 and not h.value
        assert "num_streams" in lib.AspNs_last_error().decode()
    assert lib.AspHpfBatch_Create(None, 1, 1, 0) == -1 and lib.AspLevelBatch_Create(None, 1, 0) == -1
    if hpf.device_count() > 0:
        return   # the rest needs a machine without a HIP device
    with pytest.raises(hpf.AspError) as exc:
        hpf.HpfBatch(4)
    assert "no HIP device" in str(exc.value)
    with pytest.raises(level.AspError) as exc:
        level.LevelBatch(4)
    assert "no HIP device" in str(exc.value)
    assert lib.AspHpf_Create(C.byref(h)) == -2 and not h.value


def test_null_handles_are_refused(built_lib):
    from audiosignalprocess_amd import hpf, level

    lib = level.load_library() and hpf.load_library()
    buf = (C.c_int16 * 160)()
    st = hpf.AspHpfState()
    out = C.c_int32(7)
    p = C.addressof(buf)
    assert lib.AspHpfBatch_Free(None) == -1 and lib.AspHpfBatch_num_streams(None) == -1
    assert lib.AspHpfBatch_num_channels(None) == -1
    assert lib.AspHpfBatch_Init(None, 16000) == -1 and lib.AspHpfBatch_InitStream(None, 0, 16000) == -1
    assert lib.AspHpfBatch_Process(None, p, p, 1, 160, 0) == -1
    assert lib.AspHpfBatch_ProcessFloatS16(None, p, p, 1, 80, 0) == -1
    assert lib.AspHpfBatch_ExportState(None, 0, 0, C.addressof(st)) == -1
    assert lib.AspHpfBatch_ImportState(None, 0, 0, C.addressof(st)) == -1
    assert lib.AspHpfBatch_SetStream(None, None) == -1 and lib.AspHpfBatch_Synchronize(None) == -1
    assert lib.AspHpf_Create(None) == -1 and lib.AspHpf_Init(None, 16000) == -1
    assert lib.AspHpf_Process(None, p, 160) == -1 and lib.AspHpf_Free(None) == -1
    assert lib.AspLevelBatch_Free(None) == -1 and lib.AspLevelBatch_num_streams(None) == -1
    assert lib.AspLevelBatch_Reset(None) == -1 and lib.AspLevelBatch_ResetStream(None, 0) == -1
    assert lib.AspLevelBatch_Process(None, p, 1, 1, 160, 0) == -1
    assert lib.AspLevelBatch_ProcessMuted(None, 160) == -1 and lib.AspLevelBatch_ProcessMutedStream(None, 0, 160) == -1
    assert lib.AspLevelBatch_RMS(None, C.addressof(out)) == -1 and lib.AspLevelBatch_RMS_stream(None, 0, C.addressof(out)) == -1
    assert lib.AspLevelBatch_ExportState(None, 0, p) == -1 and lib.AspLevelBatch_ImportState(None, 0, p) == -1
    assert lib.AspLevelBatch_SetStream(None, None) == -1 and lib.AspLevelBatch_Synchronize(None) == -1
    assert out.value == 7


def test_bad_rates_and_lengths_are_refused(built_lib):
    """The rate table and the length bounds, on the CPU build of the same checks and, with a device, on a batch."""
    from audiosignalprocess_amd import hpf, level

    r = hpf.Restate()
    for rate in (0, 11025, 22050, 44100, 96000, -8000):
        assert r.init(rate) == -1
    for rate, set_ in ((8000, 0), (16000, 1), (32000, 1), (48000, 1)):
        assert r.init(rate) == 0 and r.st.coeff_set == set_
    assert hpf.MAX_SAMPLES == 160 and level.MAX_SAMPLES == 480
    if hpf.device_count() < 1:
        return
    import numpy as np

    b, m = hpf.HpfBatch(2), level.LevelBatch(2)
    x = np.zeros((1, 2, 1, 481), np.int16)
    p = x.ctypes.data
    assert b.lib.AspHpfBatch_Process(b.h, p, p, 1, 160, 0) == -4   # before Init
    assert b.init(44100) == -1 and b.init(16000) == 0 and b.init(22050, stream=1) == -1 and b.init(8000, stream=2) == -1
    for n in (0, -1, 161):
        assert b.lib.AspHpfBatch_Process(b.h, p, p, 1, n, 0) == -1
        assert b.lib.AspHpfBatch_ProcessFloatS16(b.h, p, p, 1, n, 0) == -1
    assert b.lib.AspHpfBatch_Process(b.h, p, p, 1, 160, 2) == -1 and b.lib.AspHpfBatch_Process(b.h, None, p, 1, 160, 0) == -1
    for n in (0, -1, 481):
        assert m.lib.AspLevelBatch_Process(m.h, p, 1, 1, n, 0) == -1
    assert m.lib.AspLevelBatch_Process(m.h, p, 1, 0, 160, 0) == -1 and m.lib.AspLevelBatch_Process(m.h, p, 1, 17, 160, 0) == -1
    assert m.lib.AspLevelBatch_ProcessMuted(m.h, -1) == -1 and m.lib.AspLevelBatch_ResetStream(m.h, 2) == -1
    assert (m.rms() == 127).all()
    b.close()
    m.close()


def test_rms_level_client_compiles_and_links(built_lib, tmp_path):
    """tests/hpf_client.cpp: webrtc::RMSLevel and AspHpf_* from C++11, linked against the library."""
    from audiosignalprocess_amd.build import LIBDIR

    exe = str(tmp_path / "hpf_client")
    subprocess.run(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "hpf_client.cpp"), "-L" + LIBDIR, "-lasp_amd", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr
