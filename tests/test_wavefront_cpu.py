"""Path queues, the host-only half (no GPU needed): header / exports / optional bindings of the advance and wavefront
entries, crt_wavefront_stats' layout on both sides, and the argument checks of the C entries and of the Python
front-end, which all come before any device use."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib, paths

from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
NEW = ("crt_scene_path_advance_device", "crt_renderer_render_wavefront", "crt_path_advance_entries")
F32 = np.float32
INVALID = -1                        # CRT_ERR_INVALID_ARGUMENT


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _header():
    return re.sub(r"/\*.*?\*/", "", (REPO / "include" / "crt_hip.h").read_text(), flags=re.S)


def _code(name):
    m = re.search(r"\b%s\s*=\s*(-?\d+)" % name, _header()) or re.search(r"#define\s+%s\s+\(?(-?\d+)" % name, _header())
    assert m, name
    return int(m.group(1))


# ------------------------------------------------------------------------------------------ header, exports, bindings
def test_new_names_declared_exported_bound():
    header = _header()
    L = _lib.hip()
    libs = [_lib.HIP_LIB, REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"]
    for lib in libs:
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
        assert set(NEW) <= exported, (lib, set(NEW) - exported)
    assert re.search(r"global:\s*crt_\*;", (REPO / "raytracer-cuda_amd" / "csrc" / "exports.map").read_text())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.HIP_SYMBOLS and name in _lib.OPTIONAL_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"typedef\s+struct\s+crt_wavefront_stats\s*\{", header)
    assert L.crt_abi_version() == 3 and _lib.ABI_VERSION == 3 and re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", header)
    assert L.crt_path_advance_entries() in (64, 256, 512, 768, 1024)
    assert callable(paths.advance) and callable(crt_amd.Scene.path_advance) and callable(crt_amd.Renderer.render_wavefront)


def test_wavefront_stats_layout(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "crt_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   "sizeof(crt_wavefront_stats), offsetof(crt_wavefront_stats, rays), "
                   "offsetof(crt_wavefront_stats, iterations), offsetof(crt_wavefront_stats, ms)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-I", str(REPO / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [16, 0, 8, 12]
    assert C.sizeof(_lib.WavefrontStats) == 16
    assert [getattr(_lib.WavefrontStats, k).offset for k in ("rays", "iterations", "ms")] == got[1:]


class _OlderLibrary:
    """A library of the same ABI version from before the path queues: everything but the new entries."""

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
    assert not any(hasattr(old, n) for n in NEW) and hasattr(old, "crt_scene_path_step_device")
    for name in NEW:
        with pytest.raises(crt_amd.CrtError, match=name):
            _lib.require(name)
    scene = crt_amd.Scene(None, 0)
    renderer = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_render_wavefront"):
        renderer.render_wavefront(scene, 1)
    # the advance front-end reaches the library only with device tensors, which this machine may not have: its look-up
    # is the first thing after the argument checks (test_advance_rejects shows that none comes before them)
    if torch.cuda.is_available():
        z = lambda dt: torch.zeros((5, 8), dtype=dt, device="cuda:0")   # noqa: E731
        with pytest.raises(crt_amd.CrtError, match="crt_scene_path_advance_device"):
            paths.advance(scene, renderer, z(torch.float32), z(torch.float32), z(torch.int32), 20, None)
    monkeypatch.setattr(_lib, "_hip", real)
    assert _lib.require(NEW[0]) is getattr(real, NEW[0])


# ------------------------------------------------------------------------------------------ Python argument checks
@pytest.fixture
def no_library(monkeypatch):
    """Any look-up of an entry fails the test: the checks below must come first."""
    def boom(name, lib=None):
        raise AssertionError(f"{name} looked up before the arguments were checked")
    monkeypatch.setattr(_lib, "require", boom)


def _handles():
    return crt_amd.Scene(None, 0), crt_amd.Renderer._borrow(None, 8, 4, 0, None)


def _good(n=5, n_pix=32):
    import torch
    return dict(rays=torch.zeros((n, 8), dtype=torch.float32), hits=torch.zeros((n, 8), dtype=torch.float32),
                paths=torch.zeros((n, 8), dtype=torch.int32), max_bounces=20,
                remaining=torch.zeros(n_pix, dtype=torch.int32), rng=torch.zeros((n_pix, 6), dtype=torch.int32),
                linear=torch.zeros((n_pix, 3), dtype=torch.float32),
                out=(torch.zeros((n, 8), dtype=torch.float32), torch.zeros((n, 8), dtype=torch.int32)))


def _bad_advance_cases():
    import torch
    t = torch
    g = _good()
    shared = t.zeros((10, 8), dtype=t.float32)
    return {
        "rays_dtype": dict(rays=t.zeros((5, 8), dtype=t.float64)), "rays_shape": dict(rays=t.zeros((5, 7))),
        "rays_strided": dict(rays=t.zeros((10, 8))[::2]), "rays_numpy": dict(rays=np.zeros((5, 8), F32)),
        "hits_dtype": dict(hits=t.zeros((5, 8), dtype=t.int64)), "hits_length": dict(hits=t.zeros((6, 8))),
        "paths_dtype": dict(paths=t.zeros((5, 8), dtype=t.int16)), "paths_length": dict(paths=t.zeros((4, 8), dtype=t.int32)),
        "paths_strided": dict(paths=t.zeros((8, 5), dtype=t.int32).t()),
        "max_bounces": dict(max_bounces=0),
        "remaining_dtype": dict(remaining=t.zeros(32, dtype=t.int64)), "remaining_count": dict(remaining=t.zeros(31, dtype=t.int32)),
        "remaining_strided": dict(remaining=t.zeros(64, dtype=t.int32)[::2]),
        "rng_dtype": dict(rng=t.zeros((32, 6), dtype=t.int64)), "rng_count": dict(rng=t.zeros((31, 6), dtype=t.int32)),
        "linear_dtype": dict(linear=t.zeros((32, 3), dtype=t.float16)), "linear_count": dict(linear=t.zeros(95)),
        "out_single": dict(out=g["out"][0]), "out_dtype": dict(out=(g["out"][0], t.zeros((5, 8), dtype=t.int64))),
        "out_shape": dict(out=(t.zeros((5, 4)), g["out"][1])), "out_strided": dict(out=(t.zeros((10, 8))[::2], g["out"][1])),
        "out_length": dict(out=(t.zeros((4, 8)), g["out"][1])),
        "out_alias_rays": dict(rays=g["rays"], out=(g["rays"], g["out"][1])),
        "out_alias_hits": dict(hits=g["hits"], out=(g["hits"], g["out"][1])),
        "out_alias_paths": dict(paths=g["paths"], out=(g["out"][0], g["paths"])),
        "out_alias_view": dict(rays=shared[:5], out=(shared[3:8], g["out"][1])),
        "out_alias_each_other": dict(out=(shared[:5], shared[:5].view(t.int32))),
        "all_cpu": dict(),
    }


@pytest.mark.parametrize("case", ["rays_dtype", "rays_shape", "rays_strided", "rays_numpy", "hits_dtype", "hits_length",
                                  "paths_dtype", "paths_length", "paths_strided", "max_bounces", "remaining_dtype",
                                  "remaining_count", "remaining_strided", "rng_dtype", "rng_count", "linear_dtype",
                                  "linear_count", "out_single", "out_dtype", "out_shape", "out_strided", "out_length",
                                  "out_alias_rays", "out_alias_hits", "out_alias_paths", "out_alias_view",
                                  "out_alias_each_other", "all_cpu"])
def test_advance_rejects(no_library, case):
    """Every case is wrong in one way; "all_cpu" is right in all but the device (these are CPU tensors), which is the
    last thing checked, so the other cases' errors are about what they name."""
    scene, renderer = _handles()
    kw = dict(_good(), **_bad_advance_cases()[case])
    with pytest.raises(ValueError) as e:
        scene.path_advance(renderer, **kw)
    msg = str(e.value)
    if case == "all_cpu":
        assert "cuda:0" in msg
    elif "alias" in case:
        assert "aliases" in msg
    elif case.endswith("length"):
        assert "length" in msg
    else:
        assert case.split("_")[0].replace("max", "max_bounces") in msg and "cuda" not in msg, msg


def test_advance_wants_a_renderer_on_the_scenes_device(no_library):
    scene, renderer = _handles()
    kw = _good()
    with pytest.raises(ValueError, match="Renderer"):
        paths.advance(scene, None, **kw)
    with pytest.raises(ValueError, match="another device"):
        paths.advance(scene, crt_amd.Renderer._borrow(None, 8, 4, 1, None), **kw)
    for optional in ("remaining", "rng", "linear", "out"):      # None for each is fine: the device is the complaint
        with pytest.raises(ValueError, match="cuda:0"):
            paths.advance(scene, renderer, **dict(kw, **{optional: None}))


def test_driver_rejects_an_unknown_compaction(no_library):
    scene, renderer = _handles()
    with pytest.raises(ValueError, match="compact"):
        paths.render(scene, renderer, 1, compact="nonsense")
    with pytest.raises(ValueError, match="max_bounces"):
        paths.render(scene, renderer, 1, max_bounces=0, compact="device")


# ------------------------------------------------------------------------------------------ C argument checks
def _fake(device=0):
    """Stands in for a handle: a zeroed block whose first int, the handle's device in both structs, is `device`.  Each
    call below is refused by a check that comes before anything else of the handle is read, except has_camera, which the
    zeroed block answers with "no camera"."""
    a = np.zeros(1 << 16, np.uint8)
    a[:4].view(np.int32)[0] = device
    return a


def test_advance_entry_rejects_bad_arguments_before_any_device_use():
    L = _lib.hip()
    adv = L.crt_scene_path_advance_device
    sc, rn = _fake(), _fake()
    a = np.zeros((5, 16, 8), F32)              # five 16-B aligned arrays of 16 entries
    cnt, rem = np.zeros(4, np.uint32), np.zeros(8, np.int32)
    msg = lambda: L.crt_last_error().decode()   # noqa: E731

    def call(scene=sc, r=rn, rays=a[0], hits=a[1], pth=a[2], n=4, mb=20, rng=None, lin=None, remaining=rem,
             rays_out=a[3], pth_out=a[4], count=cnt):
        q = lambda x: None if x is None else (x if isinstance(x, C.c_void_p) else _p(x))   # noqa: E731
        return adv(q(scene), q(r), q(rays), q(hits), q(pth), n, mb, q(rng), q(lin), q(remaining), q(rays_out),
                   q(pth_out), q(count), None)

    assert call(scene=None) == INVALID and "null scene" in msg()
    assert call(r=None) == INVALID and "null renderer" in msg()
    for n in (-1, 1 << 31, 1 << 40):
        assert call(n=n) == INVALID and "2^31" in msg()
    for k in ("rays", "hits", "pth", "rays_out", "pth_out", "count"):
        assert call(**{k: None}) == INVALID and "null" in msg(), k
    off = lambda x, by=4: C.c_void_p(x.ctypes.data + by)   # noqa: E731
    for k, arr in (("rays", a[0]), ("hits", a[1]), ("pth", a[2]), ("rays_out", a[3]), ("pth_out", a[4])):
        assert call(**{k: off(arr)}) == INVALID and "aligned" in msg(), k
    for k, arr in (("remaining", rem), ("count", cnt)):
        assert call(**{k: off(arr, 2)}) == INVALID and "aligned" in msg(), k
    for mb in (0, -1):
        assert call(mb=mb) == INVALID and "max_bounces" in msg()
    assert call(rays_out=a[0]) == INVALID and "overlaps" in msg()
    assert call(pth_out=a[1]) == INVALID and "overlaps" in msg()
    assert call(rays_out=off(a[2], 64)) == INVALID and "overlaps" in msg()       # partly inside the input paths
    assert call(pth_out=a[3]) == INVALID and "overlap" in msg()
    assert call(scene=_fake(1)) == INVALID and "different devices" in msg()
    assert call() == INVALID and "no camera" in msg()
    assert call(n=0) == INVALID and "no camera" in msg()                         # n == 0 zeroes the count on the device: a whole call
    assert not cnt.any()


def test_wavefront_entry_rejects_bad_arguments_before_any_device_use():
    L = _lib.hip()
    wf = L.crt_renderer_render_wavefront
    sc, rn = _fake(), _fake()
    msg = lambda: L.crt_last_error().decode()   # noqa: E731
    assert wf(None, _p(sc), 1, 20, 0, None, None, None) == INVALID and "null" in msg()
    assert wf(_p(rn), None, 1, 20, 0, None, None, None) == INVALID and "null" in msg()
    assert wf(_p(rn), _p(sc), -1, 20, 0, None, None, None) == INVALID and "spp" in msg()
    for mb in (0, -3):
        assert wf(_p(rn), _p(sc), 1, mb, 0, None, None, None) == INVALID and "max_bounces" in msg()
    assert wf(_p(rn), _p(sc), 1, 20, 4, None, None, None) == INVALID and "flag" in msg()
    assert wf(_p(rn), _p(_fake(1)), 1, 20, 0, None, None, None) == INVALID and "different devices" in msg()
    assert wf(_p(rn), _p(sc), 1, 20, 0, None, None, None) == INVALID and "camera" in msg()
    assert _code("CRT_ERR_INVALID_ARGUMENT") == INVALID and _code("CRT_ERR_UNSUPPORTED") < 0
