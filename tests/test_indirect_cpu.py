"""Device-side batch sizes, the host-only half (no GPU needed): header / exports / optional bindings of the three
indirect entries, and the argument checks of the C entries and of the Python front-ends, which all come before any
device use."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib, paths

REPO = Path(__file__).resolve().parents[1]
NEW = ("crt_scene_trace_indirect_device", "crt_scene_path_advance_indirect_device", "crt_renderer_render_wavefront_queued")
F32 = np.float32
INVALID = -1                        # CRT_ERR_INVALID_ARGUMENT


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _off(a, by):
    return C.c_void_p(a.ctypes.data + by)


def _msg():
    return _lib.hip().crt_last_error().decode()


# ------------------------------------------------------------------------------------------ header, exports, bindings
def test_new_names_declared_exported_bound():
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "crt_hip.h").read_text(), flags=re.S)
    L = _lib.hip()
    for lib in (_lib.HIP_LIB, REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert set(NEW) <= exported, (lib, set(NEW) - exported)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.HIP_SYMBOLS and name in _lib.OPTIONAL_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.crt_abi_version() == 3 and _lib.ABI_VERSION == 3 and re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", header)


class _OlderLibrary:
    """A library of the same ABI version from before the indirect entries: everything but them."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in NEW:
            raise AttributeError(name)
        return getattr(self._real, name)


def test_an_older_library_loads_and_the_front_ends_name_what_is_missing(monkeypatch):
    real = _lib.hip()
    monkeypatch.setattr(_lib, "_hip", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda *a, **k: _OlderLibrary(real))
    old = _lib.hip()
    assert isinstance(old, _OlderLibrary) and old.crt_abi_version() == 3
    assert not any(hasattr(old, n) for n in NEW) and hasattr(old, "crt_renderer_render_wavefront")
    for name in NEW:
        with pytest.raises(crt_amd.CrtError, match=name):
            _lib.require(name)
    scene = crt_amd.Scene(None, 0)
    renderer = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_render_wavefront_queued"):
        renderer.render_wavefront(scene, 1, sync_every=4)
    monkeypatch.setattr(_lib, "_hip", real)
    assert _lib.require(NEW[0]) is getattr(real, NEW[0])


# ------------------------------------------------------------------------------------------ C argument checks
def _fake(device=0):
    """Stands in for a handle: a zeroed block whose first int, the handle's device in both structs, is `device`.  Each
    call below is refused by a check that comes before anything else of the handle is read, except has_camera, which the
    zeroed block answers with "no camera"."""
    a = np.zeros(1 << 16, np.uint8)
    a[:4].view(np.int32)[0] = device
    return a


def test_indirect_trace_entry_rejects_bad_arguments_before_any_device_use():
    fn = _lib.hip().crt_scene_trace_indirect_device
    sc = _fake()
    rays, hits, n = np.zeros((16, 8), F32), np.zeros((16, 8), F32), np.zeros(4, np.uint32)
    assert fn(None, _p(rays), _p(n), 4, None, _p(hits), None, 0, None) == INVALID and "null scene" in _msg()
    assert fn(_p(sc), _p(rays), None, 4, None, _p(hits), None, 0, None) == INVALID and "count" in _msg()
    assert fn(_p(sc), _p(rays), _off(n, 2), 4, None, _p(hits), None, 0, None) == INVALID and "aligned" in _msg()
    assert fn(_p(sc), _p(rays), _p(n), -1, None, _p(hits), None, 0, None) == INVALID and "capacity" in _msg()
    assert fn(_p(sc), _p(rays), _p(n), (1 << 30) + 1, None, _p(hits), None, 0, None) == INVALID and "2^30" in _msg()
    # the count is checked even when there is nothing to trace; a good one with capacity 0 is a whole call
    assert fn(_p(sc), _p(rays), None, 0, None, _p(hits), None, 0, None) == INVALID and "count" in _msg()
    assert fn(_p(sc), _p(rays), _p(n), 0, None, _p(hits), None, 0, None) == 0
    assert fn(_p(sc), None, _p(n), 4, None, _p(hits), None, 0, None) == INVALID and "null rays" in _msg()
    assert fn(_p(sc), _p(rays), _p(n), 4, None, None, None, 0, None) == INVALID and "neither" in _msg()
    bad = _lib.TraceOptions()
    bad.mode = 3
    assert fn(_p(sc), _p(rays), _p(n), 4, C.byref(bad), _p(hits), None, 0, None) == INVALID and "mode" in _msg()
    assert fn(_p(sc), _off(rays, 4), _p(n), 4, None, _p(hits), None, 0, None) == INVALID and "16-byte" in _msg()
    assert not n.any() and not hits.any()


def test_indirect_advance_entry_rejects_bad_arguments_before_any_device_use():
    adv = _lib.hip().crt_scene_path_advance_indirect_device
    sc, rn = _fake(), _fake()
    a = np.zeros((5, 16, 8), F32)              # five 16-B aligned arrays of 16 entries
    cnt, rem, tot = np.zeros(4, np.uint32), np.zeros(8, np.int32), np.zeros(4, np.uint64)

    def call(scene=sc, r=rn, rays=a[0], hits=a[1], pth=a[2], d_n=cnt[1:], cap=4, mb=20, remaining=rem, rays_out=a[3],
             pth_out=a[4], count=cnt, totals=tot):
        q = lambda x: None if x is None else (x if isinstance(x, C.c_void_p) else _p(x))   # noqa: E731
        return adv(q(scene), q(r), q(rays), q(hits), q(pth), q(d_n), cap, mb, None, None, q(remaining), q(rays_out),
                   q(pth_out), q(count), q(totals), None)

    assert call(d_n=None) == INVALID and "null input count" in _msg()
    assert call(d_n=_off(cnt, 6)) == INVALID and "aligned" in _msg()
    assert call(scene=None) == INVALID and "null scene" in _msg()
    assert call(r=None) == INVALID and "null renderer" in _msg()
    for cap in (-1, 1 << 31):
        assert call(cap=cap) == INVALID and "2^31" in _msg()
    assert call(count=None) == INVALID and "null count" in _msg()
    assert call(d_n=cnt) == INVALID and "overlaps the input count" in _msg()
    for mb in (0, -1):
        assert call(mb=mb) == INVALID and "max_bounces" in _msg()
    # the arrays hold `capacity` entries: a[0][8:] is clear of a 4-entry input and inside a 16-entry one
    assert call(rays_out=a[0][8:], cap=4) == INVALID and "no camera" in _msg()
    assert call(rays_out=a[0][8:], cap=16) == INVALID and "overlaps" in _msg()
    assert call(pth_out=a[3], cap=16) == INVALID and "overlap" in _msg()
    assert call(totals=_off(tot, 4)) == INVALID and "8-byte" in _msg()
    assert call(scene=_fake(1)) == INVALID and "different devices" in _msg()
    assert call() == INVALID and "no camera" in _msg()
    assert call(totals=None) == INVALID and "no camera" in _msg()            # totals are optional
    assert not cnt.any() and not tot.any()


def test_queued_entry_rejects_bad_arguments_before_any_device_use():
    wf = _lib.hip().crt_renderer_render_wavefront_queued
    sc, rn = _fake(), _fake()
    assert wf(None, _p(sc), 1, 20, 0, None, 1, None, None) == INVALID and "null" in _msg()
    assert wf(_p(rn), None, 1, 20, 0, None, 1, None, None) == INVALID and "null" in _msg()
    assert wf(_p(rn), _p(sc), -1, 20, 0, None, 1, None, None) == INVALID and "spp" in _msg()
    for mb in (0, -3):
        assert wf(_p(rn), _p(sc), 1, mb, 0, None, 1, None, None) == INVALID and "max_bounces" in _msg()
    for k in (-1, -64):
        assert wf(_p(rn), _p(sc), 1, 20, 0, None, k, None, None) == INVALID and "sync_every" in _msg()
    assert wf(_p(rn), _p(sc), 1, 20, 4, None, 1, None, None) == INVALID and "flag" in _msg()
    assert wf(_p(rn), _p(_fake(1)), 1, 20, 0, None, 1, None, None) == INVALID and "different devices" in _msg()
    for k in (0, 1, 1000):                                                      # good values: the camera is the complaint
        assert wf(_p(rn), _p(sc), 1, 20, 0, None, k, None, None) == INVALID and "camera" in _msg()


# ------------------------------------------------------------------------------------------ Python argument checks
@pytest.fixture
def no_library(monkeypatch):
    """Any look-up of an entry fails the test: the checks below must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "require", boom)
    monkeypatch.setattr(_lib, "hip", boom)


def _handles():
    return crt_amd.Scene(None, 0), crt_amd.Renderer._borrow(None, 8, 4, 0, None)


@pytest.mark.parametrize("query", ["trace", "occluded"])
def test_count_rejects(no_library, query):
    import torch
    scene, _ = _handles()
    fn = getattr(scene, query)
    rays = torch.zeros((5, 8), dtype=torch.float32)
    good = torch.zeros((1,), dtype=torch.int32)
    with pytest.raises(ValueError, match="torch rays"):
        fn(np.zeros((5, 8), F32), count=good)
    with pytest.raises(ValueError, match="torch rays"):
        fn(np.zeros((5, 3), F32), np.ones((5, 3), F32), count=good)
    for bad in (torch.zeros((1,), dtype=torch.int64), torch.zeros((1,), dtype=torch.float32),
                torch.zeros((2,), dtype=torch.int32), torch.zeros((1, 1), dtype=torch.int32), 5, np.zeros(1, np.int32)):
        with pytest.raises(ValueError, match="1-element int32"):
            fn(rays, count=bad)
    for bad in (torch.zeros((4, 8)), torch.zeros((5, 8), dtype=torch.float64), torch.zeros((5,), dtype=torch.uint8)[:0]):
        with pytest.raises(ValueError, match="out must be"):
            fn(rays, count=good, out=bad)
    # right in all but the device (these are CPU tensors), which is the last thing checked
    out = torch.zeros((5, 8)) if query == "trace" else torch.zeros((5,), dtype=torch.uint8)
    with pytest.raises(ValueError, match="device"):
        fn(rays, count=good, out=out)


def _good(n=5, n_pix=32):
    import torch
    return dict(rays=torch.zeros((n, 8), dtype=torch.float32), hits=torch.zeros((n, 8), dtype=torch.float32),
                paths=torch.zeros((n, 8), dtype=torch.int32), max_bounces=20,
                remaining=torch.zeros(n_pix, dtype=torch.int32), count_in=torch.zeros((1,), dtype=torch.int32),
                totals=torch.zeros((2,), dtype=torch.int64))


def test_advance_count_in_and_totals_reject(no_library):
    import torch
    scene, renderer = _handles()
    for bad in (torch.zeros((1,), dtype=torch.int64), torch.zeros((3,), dtype=torch.int32), 7):
        with pytest.raises(ValueError, match="count_in"):
            scene.path_advance(renderer, **dict(_good(), count_in=bad))
    for bad in (torch.zeros((2,), dtype=torch.int32), torch.zeros((3,), dtype=torch.int64), torch.zeros((4,), dtype=torch.int64)[::2]):
        with pytest.raises(ValueError, match="totals"):
            scene.path_advance(renderer, **dict(_good(), totals=bad))
    with pytest.raises(ValueError, match="totals needs count_in"):
        paths.advance(scene, renderer, **dict(_good(), count_in=None))
    with pytest.raises(ValueError, match="cuda:0"):                              # all good but the device
        paths.advance(scene, renderer, **_good())


def test_driver_rejects_bad_sync_every(no_library):
    scene, renderer = _handles()
    for bad in (0, -1, -7, 1.5):
        with pytest.raises(ValueError, match="sync_every"):
            paths.render(scene, renderer, 1, compact="device", sync_every=bad)
    for k in (2, 64):
        with pytest.raises(ValueError, match="sync_every"):
            paths.render(scene, renderer, 1, compact="torch", sync_every=k)
        with pytest.raises(ValueError, match="sync_every"):
            paths.render(scene, renderer, 1, sync_every=k)
