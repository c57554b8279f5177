"""Device memory is held only by csrc/crt_devmem.h's types: what can be checked without a GPU.

1. the six HIP calls that allocate or release device memory, pinned memory and events appear in csrc/ only in that header.
2. crt_debug_live_allocations is declared, exported and bound, and the ABI version is still 3.
3. with no device the count is (0, 0), also after an entry that fails for lack of one.
"""
import ctypes as C
import fnmatch
import re
from pathlib import Path

import numpy as np

from crt_amd import _lib

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "raytracer-cuda_amd" / "csrc"
OWNING_CALLS = ("hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipEventCreate", "hipEventDestroy")
ENTRY = "crt_debug_live_allocations"
# use_device(): CRT_ERR_NO_DEVICE when HIP counts zero devices, CRT_ERR_HIP when hipGetDeviceCount itself fails, as it
# does where no driver is present
NO_DEVICE, HIP_FAILED = -4, -2


def test_the_owning_hip_calls_are_in_the_ownership_header_alone():
    call = re.compile(r"\b(" + "|".join(OWNING_CALLS) + r")\b")
    files = sorted(p for p in CSRC.iterdir() if p.is_file())
    assert CSRC / "crt_hip.hip" in files and CSRC / "crt_bvh_build.hip" in files and CSRC / "crt_trace.h" in files
    found = {}
    for p in files:
        hits = [(n + 1, m.group(1)) for n, line in enumerate(p.read_text().splitlines()) for m in call.finditer(line)]
        if hits:
            found[p.name] = hits
    assert set(found) == {"crt_devmem.h"}, {k: v[:5] for k, v in found.items() if k != "crt_devmem.h"}
    assert {name for _, name in found["crt_devmem.h"]} == set(OWNING_CALLS)


def test_the_live_count_entry_is_declared_exported_and_bound():
    header = (REPO / "include" / "crt_hip.h").read_text()
    assert re.search(r"^int\s+" + ENTRY + r"\(int64_t\* buffers, int64_t\* bytes\);", header, re.M)
    assert re.search(r"^#define CRT_ABI_VERSION 3$", header, re.M)
    exported = re.search(r"global:([^;]*);", (CSRC / "exports.map").read_text()).group(1).split()
    assert any(fnmatch.fnmatchcase(ENTRY, pattern) for pattern in exported)
    assert ENTRY in _lib.HIP_SYMBOLS and ENTRY in _lib.OPTIONAL_SYMBOLS
    L = _lib.hip()
    assert L.crt_abi_version() == 3 == _lib.ABI_VERSION
    fn = _lib.require(ENTRY)
    assert fn.restype is C.c_int and len(fn.argtypes) == 2


def _live():
    buffers, nbytes = C.c_int64(-1), C.c_int64(-1)
    assert _lib.require(ENTRY)(C.byref(buffers), C.byref(nbytes)) == 0
    return buffers.value, nbytes.value


def test_nothing_is_live_without_a_device():
    L = _lib.hip()
    n = C.c_int(0)
    assert L.crt_device_count(C.byref(n)) == 0
    if n.value:
        return                      # a GPU machine: tests/test_gpu_devmem.py checks the balance there
    assert _live() == (0, 0)
    a = np.ones(4, np.float32)
    out, out64 = np.zeros(16, np.float32), np.zeros(8, np.float64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.crt_selftest_math(p(a), p(a), 4, p(out), p(out64)) in (NO_DEVICE, HIP_FAILED)
    assert b"device" in L.crt_last_error()
    assert _live() == (0, 0)
    assert _lib.require(ENTRY)(None, None) == -1 and b"null" in L.crt_last_error()
