"""Path finish, the host-only half (no GPU needed): header / exports / optional bindings of the two entries, and the
argument checks of the C entries and of the Python front-ends, which all come before any device use."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib, paths

REPO = Path(__file__).resolve().parents[1]
NEW = ("crt_scene_path_finish_device", "crt_renderer_render_wavefront_finish")
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
    assert callable(paths.finish) and callable(crt_amd.Scene.path_finish)


class _OlderLibrary:
    """A library of the same ABI version from before the finish entries: everything but them."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in NEW:
            raise AttributeError(name)
        return getattr(self._real, name)


def test_an_older_library_loads_and_the_front_ends_name_what_is_missing(monkeypatch):
    import torch
    real = _lib.hip()
    monkeypatch.setattr(_lib, "_hip", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda *a, **k: _OlderLibrary(real))
    old = _lib.hip()
    assert isinstance(old, _OlderLibrary) and old.crt_abi_version() == 3
    assert not any(hasattr(old, n) for n in NEW) and hasattr(old, "crt_renderer_render_wavefront_queued")
    for name in NEW:
        with pytest.raises(crt_amd.CrtError, match=name):
            _lib.require(name)
    scene = crt_amd.Scene(None, 0)
    renderer = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_render_wavefront_finish"):
        renderer.render_wavefront(scene, 1, finish_below=4)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_render_wavefront_finish"):
        renderer.render_wavefront(scene, 1, sync_every=2, finish_below=0)
    # all good but the library: the device check is the last of the front-end's own, so it is stubbed out here
    monkeypatch.setattr(paths, "_on_device", lambda *a, **k: None)
    with pytest.raises(crt_amd.CrtError, match="crt_scene_path_finish_device"):
        paths.finish(scene, renderer, torch.zeros((5, 8)), torch.zeros((5, 8), dtype=torch.int32), 20, None)
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


def test_finish_entry_rejects_bad_arguments_before_any_device_use():
    fin = _lib.hip().crt_scene_path_finish_device
    sc, rn = _fake(), _fake()
    a = np.zeros((2, 16, 8), F32)
    cnt, rem, tot = np.zeros(4, np.uint32), np.zeros(8, np.int32), np.zeros(4, np.uint64)
    rng, lin = np.zeros(64, np.uint32), np.zeros(64, F32)

    def call(scene=sc, r=rn, rays=a[0], pth=a[1], d_n=cnt, cap=4, mb=20, d_rng=None, d_lin=None, remaining=rem, totals=tot):
        q = lambda x: None if x is None else (x if isinstance(x, C.c_void_p) else _p(x))   # noqa: E731
        return fin(q(scene), q(r), q(rays), q(pth), q(d_n), cap, mb, q(d_rng), q(d_lin), q(remaining), q(totals), None)

    assert call(scene=None) == INVALID and "null scene" in _msg()
    assert call(r=None) == INVALID and "null renderer" in _msg()
    for cap in (-1, 1 << 31, 1 << 40):
        assert call(cap=cap) == INVALID and "2^31" in _msg()
    assert call(rays=None) == INVALID and "null array" in _msg()
    assert call(pth=None) == INVALID and "null array" in _msg()
    assert call(rays=_off(a[0], 4)) == INVALID and "16-byte" in _msg()
    assert call(pth=_off(a[1], 8)) == INVALID and "16-byte" in _msg()
    for mb in (0, -1):
        assert call(mb=mb) == INVALID and "max_bounces" in _msg()
    assert call(d_n=_off(cnt, 2)) == INVALID and "4-byte" in _msg()
    assert call(remaining=_off(rem, 1)) == INVALID and "4-byte" in _msg()
    assert call(d_rng=_off(rng, 3)) == INVALID and "4-byte" in _msg()
    assert call(d_lin=_off(lin, 2)) == INVALID and "4-byte" in _msg()
    assert call(totals=_off(tot, 4)) == INVALID and "8-byte" in _msg()
    assert call(scene=_fake(1)) == INVALID and "different devices" in _msg()
    # good values, optional ones absent or present, an empty batch too: the camera is the complaint
    for kw in ({}, {"d_n": None}, {"totals": None}, {"remaining": None}, {"d_rng": rng, "d_lin": lin}, {"cap": 0},
               {"cap": 0, "rays": None, "pth": None}, {"cap": (1 << 31) - 1}):
        assert call(**kw) == INVALID and "no camera" in _msg(), kw
    assert not cnt.any() and not tot.any() and not rem.any() and not a.any()


def test_wavefront_finish_entry_rejects_bad_arguments_before_any_device_use():
    wf = _lib.hip().crt_renderer_render_wavefront_finish
    sc, rn = _fake(), _fake()
    assert wf(None, _p(sc), 1, 20, 0, None, 1, 0, None, None) == INVALID and "null" in _msg()
    assert wf(_p(rn), None, 1, 20, 0, None, 1, 0, None, None) == INVALID and "null" in _msg()
    assert wf(_p(rn), _p(sc), -1, 20, 0, None, 1, 0, None, None) == INVALID and "spp" in _msg()
    for mb in (0, -3):
        assert wf(_p(rn), _p(sc), 1, mb, 0, None, 1, 0, None, None) == INVALID and "max_bounces" in _msg()
    for k in (-1, -64):
        assert wf(_p(rn), _p(sc), 1, 20, 0, None, k, 0, None, None) == INVALID and "sync_every" in _msg()
    for below in (-2, -3, -(1 << 40)):
        assert wf(_p(rn), _p(sc), 1, 20, 0, None, 1, below, None, None) == INVALID and "finish_below" in _msg()
    assert wf(_p(rn), _p(sc), 1, 20, 4, None, 1, 0, None, None) == INVALID and "flag" in _msg()
    assert wf(_p(rn), _p(_fake(1)), 1, 20, 0, None, 1, 0, None, None) == INVALID and "different devices" in _msg()
    for below in (-1, 0, 1, 1000, 1 << 40):                                     # good values: the camera is the complaint
        for k in (0, 1, 7):
            assert wf(_p(rn), _p(sc), 1, 20, 0, None, k, below, None, None) == INVALID and "camera" in _msg()


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


def _good(n=5, n_pix=32):
    import torch
    return dict(rays=torch.zeros((n, 8), dtype=torch.float32), paths=torch.zeros((n, 8), dtype=torch.int32),
                max_bounces=20, remaining=torch.zeros(n_pix, dtype=torch.int32),
                rng=torch.zeros((n_pix, 6), dtype=torch.int32), linear=torch.zeros(3 * n_pix, dtype=torch.float32),
                count_in=torch.zeros((1,), dtype=torch.int32), totals=torch.zeros((2,), dtype=torch.int64))


def test_finish_rejects(no_library):
    import torch
    scene, renderer = _handles()
    bad = {
        "rays": [np.zeros((5, 8), F32), torch.zeros((5, 8), dtype=torch.float64), torch.zeros((5, 7)), torch.zeros((8, 5)).T,
                 torch.zeros((40,))],
        "paths": [None, torch.zeros((5, 8), dtype=torch.int64), torch.zeros((5, 4), dtype=torch.int32),
                  torch.zeros((5, 16), dtype=torch.int32)[:, ::2]],
        "remaining": [torch.zeros(32, dtype=torch.int64), torch.zeros(31, dtype=torch.int32), np.zeros(32, np.int32),
                      torch.zeros(64, dtype=torch.int32)[::2]],
        "rng": [torch.zeros((32, 6), dtype=torch.int64), torch.zeros((31, 6), dtype=torch.int32)],
        "linear": [torch.zeros(96, dtype=torch.float64), torch.zeros(95, dtype=torch.float32)],
        "count_in": [torch.zeros((1,), dtype=torch.int64), torch.zeros((3,), dtype=torch.int32), 7],
        "totals": [torch.zeros((2,), dtype=torch.int32), torch.zeros((3,), dtype=torch.int64),
                   torch.zeros((4,), dtype=torch.int64)[::2]],
    }
    for name, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=name):
                scene.path_finish(renderer, **dict(_good(), **{name: v}))
    with pytest.raises(ValueError, match="differ in length"):
        paths.finish(scene, renderer, **dict(_good(), paths=torch.zeros((6, 8), dtype=torch.int32)))
    for mb in (0, -2):
        with pytest.raises(ValueError, match="max_bounces"):
            paths.finish(scene, renderer, **dict(_good(), max_bounces=mb))
    with pytest.raises(ValueError, match="Renderer"):
        paths.finish(scene, None, **_good())
    with pytest.raises(ValueError, match="another device"):
        paths.finish(scene, crt_amd.Renderer._borrow(None, 8, 4, 1, None), **_good())
    # all good but the device (these are CPU tensors), which is the last thing checked; the optional ones absent too
    with pytest.raises(ValueError, match="cuda:0"):
        paths.finish(scene, renderer, **_good())
    with pytest.raises(ValueError, match="cuda:0"):
        paths.finish(scene, renderer, **dict(_good(), remaining=None, rng=None, linear=None, count_in=None, totals=None))


def test_driver_rejects_bad_finish_below(no_library):
    scene, renderer = _handles()
    for bad in (-1, -7, 1.5):
        with pytest.raises(ValueError, match="finish_below"):
            paths.render(scene, renderer, 1, compact="device", finish_below=bad)
    for k in (1, 4096):
        with pytest.raises(ValueError, match="finish_below"):
            paths.render(scene, renderer, 1, compact="torch", finish_below=k)
        with pytest.raises(ValueError, match="finish_below"):
            paths.render(scene, renderer, 1, finish_below=k)
