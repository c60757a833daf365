"""CPU suite: libasp_amd.so exports every function include/asp_ts.h declares with the header's prototypes, the
state struct has the ctypes mirror's size, the library's tables are the CPU build's, and a batch cannot be
created without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported(built_lib):
    lib = C.CDLL(built_lib)
    names = declared_functions("asp_ts.h")
    assert len(names) == 14 and all(n.startswith("AspTs") for n in names)
    assert [n for n in names if not hasattr(lib, n)] == []


def test_python_mirror_matches_the_header_prototypes(built_lib):
    from audiosignalprocess_amd import ts

    lib = ts.load_library()
    txt = open(os.path.join(ROOT, "include", "asp_ts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = dict(re.findall(r"\b(AspTs\w+)\s*\(([^;{]*)\)\s*;", txt))
    assert len(protos) == 14
    for name, args in protos.items():
        n = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(getattr(lib, name).argtypes) == n, name
    assert lib.AspTs_state_size() == C.sizeof(ts.AspTsState)
    assert C.sizeof(ts.AspTsState) == 4 * (15 + 3 + 4 * 8 + 1 + 8 * 180 + 7 * 15)


@pytest.mark.parametrize("n", (128, 256, 512, 1024))
def test_library_tables_are_the_cpu_builds(built_lib, n):
    from audiosignalprocess_amd import ts

    lib = ts.load_library()
    for which in range(3):
        a, b = ts.table(lib.AspTs_table, which, n), ts.table(ts.Restate.lib().TsRestate_table, which, n)
        assert a.size == (n, n // 2, n // 2 + 1)[which] and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert lib.AspTs_table(0, 64, np.zeros(64, np.float32).ctypes.data, 64) < 0
    assert lib.AspTs_table(0, n, np.zeros(8, np.float32).ctypes.data, 8) < 0


def test_create_fails_loudly_without_a_device(built_lib):
    from audiosignalprocess_amd import ts

    lib = ts.load_library()
    h = C.c_void_p()
    assert lib.AspTsBatch_Create(C.byref(h), 0, 0) < 0   # refused before a device is looked at
    assert "num_streams" in lib.AspNs_last_error().decode()
    assert lib.AspTsBatch_Initialize(None, 16000, 16000, 1) < 0 and lib.AspTsBatch_Free(None) < 0
    if ts.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(ts.AspError) as exc:
        ts.TsBatch(4)
    assert "no HIP device" in str(exc.value)
