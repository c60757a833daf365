"""CPU suite: libasp_amd.so exports every function include/asp_audio_buffer.h declares with the header's prototypes
(and the checkpoint entry points this module added to asp_split.h and asp_resample.h), a batch cannot be created
without a device, the refusals that need no device, and a C++ client of the header compiles and links."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 36   # functions the header declares


def test_every_declared_symbol_is_exported(built_lib):
    lib = C.CDLL(built_lib)
    names = declared_functions("asp_audio_buffer.h")
    assert len(names) == COUNT and all(n.startswith("AspAudioBufferBatch_") for n in names)
    assert [n for n in names if not hasattr(lib, n)] == []
    for n in ("AspSplitBatch_SetStream", "AspSplitBatch_Synchronize", "AspSplitBatch_ExportState", "AspSplitBatch_ImportState",
              "AspSincBatch_ExportState", "AspSincBatch_ImportState", "AspSincBatch_buffer_length"):
        assert n in declared_functions("asp_split.h") + declared_functions("asp_resample.h") and hasattr(lib, n), n


def test_python_mirror_matches_the_header_prototypes(built_lib):
    from audiosignalprocess_amd import ab

    lib = ab.load_library()
    txt = open(os.path.join(ROOT, "include", "asp_audio_buffer.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = dict(re.findall(r"\b(AspAudioBufferBatch_\w+)\s*\(([^;{]*)\)\s*;", txt))
    assert len(protos) == COUNT
    for name, args in protos.items():
        assert len(getattr(lib, name).argtypes) == args.count(",") + 1, name


def test_state_structs_have_the_documented_sizes(built_lib, tmp_path):
    """AspSincPos is 32 bytes, AspSplitState 5088, and ab.py's RECORD_BYTES is csrc/ab_layout.h's AbRecord."""
    from audiosignalprocess_amd import ab

    src = tmp_path / "sizes.cpp"
    src.write_text('#include <stdio.h>\n#include "asp_split.h"\n#include "ab_layout.h"\n'
                   'int main() { printf("%zu %zu %zu\\n", sizeof(AspSincPos), sizeof(AspSplitState), sizeof(aspab::AbRecord)); }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "audiosignalprocess_amd", "csrc"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [32, 288 + 64 + 4 * (512 + 672), ab.AudioBufferBatch.RECORD_BYTES]


def test_create_fails_loudly_without_a_device(built_lib):
    from audiosignalprocess_amd import ab

    lib = ab.load_library()
    h = C.c_void_p()
    refusals = [((1, 160, 3, 160, 1, 160, 0), "num_input_channels"),      # 3 input channels
                ((1, 160, 0, 160, 1, 160, 0), "num_input_channels"),
                ((1, 160, 1, 160, 2, 160, 0), "num_proc_channels"),       # proc > input channels
                ((1, 160, 2, 160, 0, 160, 0), "num_proc_channels"),
                ((1, 100, 1, 160, 1, 160, 0), "samples"),                 # frame length 100
                ((1, 160, 1, 100, 1, 160, 0), "proc_samples"),
                ((1, 160, 1, 441, 1, 160, 0), "proc_samples"),            # 441 is an I/O length only
                ((1, 160, 1, 160, 1, 100, 0), "samples"),
                ((0, 160, 1, 160, 1, 160, 0), "num_streams")]
    for args, text in refusals:   # refused before a device is looked at
        assert lib.AspAudioBufferBatch_Create(C.byref(h), *args) == -1 and not h.value, args
        assert text in lib.AspNs_last_error().decode(), args
    assert lib.AspAudioBufferBatch_Create(None, 1, 160, 1, 160, 1, 160, 0) == -1
    if ab.device_count() > 0:
        return   # the rest needs a machine without a HIP device
    with pytest.raises(ab.AspError) as exc:
        ab.AudioBufferBatch(4, 160, 1, 160, 1, 160)
    assert "no HIP device" in str(exc.value)
    assert lib.AspAudioBufferBatch_Create(C.byref(h), 4, 441, 1, 160, 1, 441, 0) == -2 and not h.value


def test_null_handles_are_refused(built_lib):
    from audiosignalprocess_amd import ab

    lib = ab.load_library()
    buf = (C.c_float * 1024)()
    p = C.addressof(buf)
    L = lambda n: getattr(lib, "AspAudioBufferBatch_" + n)   # noqa: E731
    assert L("Free")(None) == -1 and L("num_streams")(None) == -1
    assert L("DeinterleaveFrom")(None, p, None, 0) == -1 and L("InterleaveTo")(None, p, None, 1, 0) == -1
    assert L("CopyFrom")(None, p, 0, 0) == -1 and L("CopyTo")(None, p, 0) == -1
    for n in ("SplitIntoFrequencyBands", "MergeFrequencyBands", "CopyLowPassToReference", "num_channels", "num_bands",
              "samples_per_channel", "samples_per_split_channel", "samples_per_keyboard_channel", "Synchronize"):
        assert L(n)(None) == -1, n
    for n in ("low_pass_reference", "mixed_low_pass_data", "keyboard_data", "channels", "channels_const", "channels_f",
              "channels_const_f"):
        assert L(n)(None) is None, n
    for n in ("split_channels", "split_channels_const", "split_channels_f", "split_channels_const_f"):
        assert L(n)(None, 0) is None, n
    assert L("set_num_channels")(None, 1) == -1 and L("set_activity")(None, 0, 0) == -1 and L("activity")(None, 0) == -1
    assert L("Read")(None, 0, -1, p, None) == -1 and L("kernel_table")(None, 0, p, 1056) == 0
    assert L("SetStream")(None, None) == -1 and L("state_size")(None) == 0
    assert L("ExportState")(None, 0, p) == -1 and L("ImportState")(None, 0, p) == -1


@pytest.mark.gpu
def test_geometry_refusals_on_a_batch(built_lib):
    """DeinterleaveFrom / InterleaveTo on a resampling geometry, Split on a buffer without bands, a layout that
    does not fit: ASP_ERR_PARAM with a text.  Only a batch can refuse these, and a batch needs a device."""
    import numpy as np

    from audiosignalprocess_amd import ab

    b = ab.AudioBufferBatch(2, 480, 2, 160, 1, 480)
    x = np.zeros((2, 960), np.int16)
    assert b.lib.AspAudioBufferBatch_DeinterleaveFrom(b.h, x.ctypes.data, None, 0) == -1
    assert "resamples its input" in b.lib.AspNs_last_error().decode()
    assert b.lib.AspAudioBufferBatch_InterleaveTo(b.h, x.ctypes.data, None, 1, 0) == -1
    assert b.lib.AspAudioBufferBatch_SplitIntoFrequencyBands(b.h) == -1 and b.lib.AspAudioBufferBatch_MergeFrequencyBands(b.h) == -1
    f = np.zeros((2, 2, 480), np.float32)
    assert b.lib.AspAudioBufferBatch_CopyFrom(b.h, f.ctypes.data, ab.MONO, 0) == -1
    assert b.lib.AspAudioBufferBatch_CopyFrom(b.h, f.ctypes.data, 4, 0) == -1
    assert b.lib.AspAudioBufferBatch_CopyFrom(b.h, f.ctypes.data, ab.STEREO, 2) == -1
    assert b.lib.AspAudioBufferBatch_CopyFrom(b.h, f.ctypes.data, ab.STEREO, 0) == 0
    b.close()


def test_client_compiles_and_links(built_lib, tmp_path):
    """tests/ab_client.cpp from C++11 against the header alone; its device-free refusals run here."""
    from audiosignalprocess_amd.build import LIBDIR

    exe = str(tmp_path / "ab_client")
    subprocess.run(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "ab_client.cpp"), "-L" + LIBDIR, "-lasp_amd", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr


@pytest.mark.gpu
def test_client_round_trip(built_lib, tmp_path):
    """tests/ab_client.cpp on a device: deinterleave, both views, interleave of 16 kHz mono frames is the identity."""
    import numpy as np

    from audiosignalprocess_amd.build import LIBDIR

    exe = str(tmp_path / "ab_client")
    subprocess.run(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "ab_client.cpp"), "-L" + LIBDIR, "-lasp_amd", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    x = np.random.default_rng(2).integers(-32768, 32768, (4, 5, 160)).astype(np.int16)
    src, dst = tmp_path / "in.i16", tmp_path / "out.i16"
    x.tofile(src)
    r = subprocess.run([exe, "identity", "5", str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert np.array_equal(np.fromfile(dst, np.int16).reshape(x.shape), x)
