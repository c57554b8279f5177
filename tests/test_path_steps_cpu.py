"""Path steps, the host-only half (no GPU needed): header / exports / optional bindings, crt_path's layout, the
per-material rows the step kernel reads (crt_scene_export_shade_rows) against a float32 restatement, and the argument
checks of the Python front-end and of the C entries, which come before any device use.

The render kernels' per-rank shading records, whose payload rows the material rows repeat, are not among the arrays
crt_scene_export returns, so no rank's record is reachable on the host; that the two agree is what the GPU tests'
bit-exact frames show (tests/test_gpu_path_steps.py), and in the library both come from one function."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib, paths

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import custom_scene  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
NEW = ("crt_renderer_camera_rays_device", "crt_scene_path_step_device", "crt_scene_export_shade_rows")
F32 = np.float32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------ header, exports, bindings
def test_new_names_declared_exported_bound():
    raw = (REPO / "include" / "crt_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.HIP_LIB)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    L = _lib.hip()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported and name in _lib.HIP_SYMBOLS and name in _lib.OPTIONAL_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"typedef\s+struct\s+crt_path\s*\{", header)
    assert re.search(r"#define\s+CRT_PATH_ACTIVE\s+0\b", header) and re.search(r"#define\s+CRT_PATH_ENDED\s+1\b", header)
    assert (_lib.PATH_ACTIVE, _lib.PATH_ENDED) == (0, 1)
    assert L.crt_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", header)
    checked = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
    out = subprocess.run(["nm", "-D", "--defined-only", str(checked)], capture_output=True, text=True, check=True).stdout
    assert all(name in out for name in NEW)


def test_crt_path_is_two_rows(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "crt_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(crt_path), offsetof(crt_path, throughput), offsetof(crt_path, bounce), "
                   "offsetof(crt_path, pixel), offsetof(crt_path, status)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-I", str(REPO / "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 0, 12, 16, 20]
    assert C.sizeof(_lib.Path) == 32
    assert [getattr(_lib.Path, k).offset for k in ("throughput", "bounce", "pixel", "status")] == got[1:]
    assert (4 * paths.PATH_BOUNCE, 4 * paths.PATH_PIXEL, 4 * paths.PATH_STATUS) == tuple(got[2:])


class _OlderLibrary:
    """A library of the same ABI version from before the path steps: everything but the optional entries."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in _lib.OPTIONAL_SYMBOLS:
            raise AttributeError(name)
        return getattr(self._real, name)


def test_an_older_library_loads_and_the_front_end_names_what_is_missing(monkeypatch):
    real = _lib.hip()
    monkeypatch.setattr(_lib, "_hip", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda *a, **k: _OlderLibrary(real))
    old = _lib.hip()                                   # the binding loop passes over the entries it does not find
    assert isinstance(old, _OlderLibrary) and old.crt_abi_version() == 3
    assert not any(hasattr(old, n) for n in NEW) and hasattr(old, "crt_scene_trace_device")
    for name in NEW:
        with pytest.raises(crt_amd.CrtError, match=name):
            _lib.require(name)
    with pytest.raises(crt_amd.CrtError, match="crt_scene_export_shade_rows"):
        paths.shade_rows(_lib.SceneDesc())
    monkeypatch.setattr(_lib, "_hip", real)
    assert _lib.require(NEW[0]) is getattr(real, NEW[0])


# ------------------------------------------------------------------------------------------ the material rows
def _rows_f32(desc):
    """The rows in numpy float32: the Metal ctor's fuzz clamp (Material.cuh:86), ri = 1 / ior for the front face
    (:113), Schlick's r0 = ((1 - ri) / (1 + ri))^2 for both faces (:133-134), the light's emission."""
    mats = C.cast(desc.materials, C.POINTER(_lib.MaterialDesc))
    out = np.zeros((desc.n_materials, 2, 4), F32)
    code = np.zeros(desc.n_materials, np.int32)
    def r0(r):
        x = F32(F32(F32(1) - r) / F32(F32(1) + r))
        return F32(x * x)
    for i in range(desc.n_materials):
        m = mats[i]
        alb, emi = np.array(m.albedo[:], F32), np.array(m.emission[:], F32)
        if m.type == 0:
            code[i], out[i, 1, :3] = 0, alb
        elif m.type == 1:
            code[i], out[i, 1, :3], out[i, 1, 3] = 1, alb, F32(m.roughness) if F32(m.roughness) < 1 else F32(1)
        elif m.type == 2:
            ior = F32(m.ior)
            inv = F32(F32(1) / ior)
            code[i], out[i, 1] = 2, [ior, inv, r0(inv), r0(ior)]
        elif m.type == 3:
            code[i], out[i, 1, :3] = 3, emi
        else:
            code[i] = 4
    out[:, 0, 0] = code.view(F32)
    return out


def _check_rows(desc):
    got = paths.shade_rows(desc)
    assert got.shape == (desc.n_materials, 2, 4) and got.dtype == F32
    want = _rows_f32(desc)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    n = C.c_int64(-1)
    assert _lib.hip().crt_scene_export_shade_rows(C.byref(desc), None, C.byref(n)) == 0 and n.value == desc.n_materials
    return got


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    return custom_scene.synth_worlds(custom_scene.family_files(tmp_path_factory.mktemp("ps_synth")))


@pytest.mark.parametrize("name", custom_scene.FAMILIES + custom_scene.WORLDS + custom_scene.ONLY)
def test_shade_rows_synth(worlds, name):
    rows = _check_rows(worlds[name].desc)
    kinds = set(rows[:, 0, 0].view(np.int32).tolist())
    assert kinds <= {0, 1, 2, 3, 4}
    if name == "soup":
        assert kinds >= {0, 1, 2, 3}, kinds         # white / red, steel, glass, lamp


@pytest.mark.parametrize("name", ["cornell", "cornell_bunny"])
def test_shade_rows_assets(scenes, name):
    rows = _check_rows(crt_amd.HostScene(scenes[name]).desc())
    glass = rows[rows[:, 0, 0].view(np.int32) == 2]
    assert name == "cornell" or len(glass) >= 1
    for g in glass[:, 1]:                             # (ior, 1 / ior, r0(1 / ior), r0(ior)): the two r0 agree to rounding
        assert g[1] == F32(1) / g[0] and abs(float(g[2]) - float(g[3])) < 1e-6


def test_shade_rows_edge_materials(scenes):
    """Fuzz above 1 and NaN clamp to 1, an unknown type is code 4 with a zero payload, ior 1 gives r0 = 0."""
    one = scenes["cornell"]
    mats = [custom_scene.mat_row(1, (0.9, 0.8, 0.7), roughness=1.5), custom_scene.mat_row(1, (0.9, 0.8, 0.7), roughness=float("nan")),
            custom_scene.mat_row(1, (0.9, 0.8, 0.7), roughness=1.0), custom_scene.mat_row(7, (0.3, 0.3, 0.3), (1, 1, 1)),
            custom_scene.mat_row(2, ior=1.0), custom_scene.mat_row(2, ior=2.4), custom_scene.mat_row(-1)]
    cs = custom_scene.CustomScene(one, [((0.0, 0.0, 0.0), 0.05, k) for k in range(len(mats))], mats)
    rows = _check_rows(cs.desc)[-len(mats):]
    assert rows[:3, 1, 3].tolist() == [1.0, 1.0, 1.0]
    assert rows[3, 0, 0].view(np.int32) == 4 and not rows[3, 1].any() and rows[6, 0, 0].view(np.int32) == 4
    assert rows[4, 1].tolist() == [1.0, 1.0, 0.0, 0.0]


def test_shade_rows_null_arguments():
    L = _lib.hip()
    n = C.c_int64(0)
    assert L.crt_scene_export_shade_rows(None, None, C.byref(n)) == -1
    assert L.crt_scene_export_shade_rows(C.byref(_lib.SceneDesc()), None, None) == -1
    d = _lib.SceneDesc()
    d.n_materials = 3                                 # materials == NULL
    assert L.crt_scene_export_shade_rows(C.byref(d), None, C.byref(n)) == -1


# ------------------------------------------------------------------------------------------ Python argument checks
@pytest.fixture
def no_library(monkeypatch):
    """Any look-up of a path-step entry fails the test: the checks below must come first."""
    def boom(name, lib=None):
        raise AssertionError(f"{name} looked up before the arguments were checked")
    monkeypatch.setattr(_lib, "require", boom)


def _handles():
    scene = crt_amd.Scene(None, 0)
    renderer = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    return scene, renderer


def _good(n=5, n_pix=32):
    import torch
    return dict(rays=torch.zeros((n, 8), dtype=torch.float32), hits=torch.zeros((n, 8), dtype=torch.float32),
                paths=torch.zeros((n, 8), dtype=torch.int32), max_bounces=20,
                rng=torch.zeros((n_pix, 6), dtype=torch.int32), linear=torch.zeros((n_pix, 3), dtype=torch.float32))


def _bad_step_cases():
    import torch
    t = torch
    return {
        "rays_dtype": dict(rays=t.zeros((5, 8), dtype=t.float64)), "rays_shape": dict(rays=t.zeros((5, 7))),
        "rays_1d": dict(rays=t.zeros(40)), "rays_strided": dict(rays=t.zeros((10, 8))[::2]),
        "rays_numpy": dict(rays=np.zeros((5, 8), F32)), "rays_cpu": dict(),
        "hits_dtype": dict(hits=t.zeros((5, 8), dtype=t.int64)), "hits_shape": dict(hits=t.zeros((5, 4))),
        "hits_strided": dict(hits=t.zeros((5, 16))[:, :8]), "hits_length": dict(hits=t.zeros((6, 8))),
        "paths_dtype": dict(paths=t.zeros((5, 8), dtype=t.int16)), "paths_shape": dict(paths=t.zeros((5, 2, 4), dtype=t.int32)),
        "paths_strided": dict(paths=t.zeros((8, 5), dtype=t.int32).t()), "paths_length": dict(paths=t.zeros((4, 8), dtype=t.int32)),
        "rng_dtype": dict(rng=t.zeros((32, 6), dtype=t.int64)), "rng_count": dict(rng=t.zeros(191, dtype=t.int32)),
        "rng_strided": dict(rng=t.zeros((32, 12), dtype=t.int32)[:, :6]), "rng_none": dict(rng=None),
        "linear_dtype": dict(linear=t.zeros((32, 3), dtype=t.float16)), "linear_count": dict(linear=t.zeros(95)),
        "linear_pixels": dict(linear=t.zeros((31, 3))), "linear_strided": dict(linear=t.zeros((32, 6))[:, :3]),
        "max_bounces": dict(max_bounces=0),
    }


@pytest.mark.parametrize("case", ["rays_dtype", "rays_shape", "rays_1d", "rays_strided", "rays_numpy", "rays_cpu",
                                  "hits_dtype", "hits_shape", "hits_strided", "hits_length", "paths_dtype", "paths_shape",
                                  "paths_strided", "paths_length", "rng_dtype", "rng_count", "rng_strided", "rng_none",
                                  "linear_dtype", "linear_count", "linear_pixels", "linear_strided", "max_bounces"])
def test_path_step_rejects(no_library, case):
    """Every case is wrong in one way; "rays_cpu" is right in all but the device (these are CPU tensors), which is the
    last thing checked, so the other cases' errors are about what they name."""
    scene, _ = _handles()
    kw = dict(_good(), **_bad_step_cases()[case])
    with pytest.raises(ValueError) as e:
        scene.path_step(**kw)
    what = case.split("_")[0]
    if case == "rays_cpu":
        assert "cuda:0" in str(e.value)
    elif case.endswith("length"):
        assert "length" in str(e.value)
    elif case == "linear_pixels":
        assert "pixels" in str(e.value)
    else:
        assert what.replace("max", "max_bounces") in str(e.value) and "cuda" not in str(e.value), str(e.value)


def test_path_step_takes_the_renderer_for_its_own_buffers(no_library):
    """rng / linear = the Renderer: its frame's pixel count is checked against the other argument's."""
    scene, renderer = _handles()
    kw = dict(_good(n_pix=31), rng=renderer)
    with pytest.raises(ValueError, match="pixels"):
        scene.path_step(**kw)
    kw = dict(_good(), rng=renderer, linear=renderer)      # consistent: the first complaint is the rays' device
    with pytest.raises(ValueError, match="cuda:0"):
        scene.path_step(**kw)
    other = crt_amd.Renderer._borrow(None, 8, 4, 1, None)
    with pytest.raises(ValueError, match="another device"):
        scene.path_step(**dict(_good(), rng=other, rays=_good()["rays"]))


def test_camera_rays_rejects(no_library):
    import torch
    _, renderer = _handles()
    bad = {"dtype": torch.zeros(4, dtype=torch.int64), "2d": torch.zeros((2, 2), dtype=torch.int32),
           "strided": torch.zeros(8, dtype=torch.int32)[::2], "cpu": torch.zeros(4, dtype=torch.int32),
           "list": [0, 1, 2]}
    for name, pixels in bad.items():
        with pytest.raises(ValueError):
            crt_amd.camera_rays(renderer, pixels)
    for rng in (torch.zeros((31, 6), dtype=torch.int32), torch.zeros((32, 6), dtype=torch.float32),
                torch.zeros((32, 6), dtype=torch.int32)):       # too short, wrong dtype, on the CPU
        with pytest.raises(ValueError):
            crt_amd.camera_rays(renderer, None, rng)


def test_driver_rejects_max_bounces_below_one(no_library):
    scene, renderer = _handles()
    with pytest.raises(ValueError, match="max_bounces"):
        paths.render(scene, renderer, 1, max_bounces=0)


# ------------------------------------------------------------------------------------------ C argument checks
def test_c_entries_reject_bad_arguments_before_any_device_use():
    """No device is needed to be told CRT_ERR_INVALID_ARGUMENT.  `fake` stands in for a handle: each call below is
    refused by a check that comes before the handle is read (the camera entry reads has_camera last: the zeroed block
    is a renderer without a camera)."""
    L = _lib.hip()
    fake = np.zeros(1 << 16, np.uint8)
    a = np.zeros((3, 16, 8), F32)            # three 16-B aligned arrays
    rays, hits, pth = a[0], a[1], a[2]
    rng, lin = np.zeros((8, 6), np.uint32), np.zeros((8, 3), F32)
    step, cam = L.crt_scene_path_step_device, L.crt_renderer_camera_rays_device
    msg = lambda: L.crt_last_error().decode()   # noqa: E731
    assert step(None, _p(rays), _p(hits), _p(pth), 4, 20, _p(rng), _p(lin), 8, None) == -1 and "null scene" in msg()
    assert cam(None, None, 4, None, _p(rays), _p(pth), None) == -1 and "null renderer" in msg()
    for n in (-1, 1 << 31, 1 << 40):
        assert step(_p(fake), _p(rays), _p(hits), _p(pth), n, 20, _p(rng), _p(lin), 8, None) == -1 and "2^31" in msg()
        assert cam(_p(fake), None, n, None, _p(rays), _p(pth), None) == -1 and "2^31" in msg()
    for k in range(3):                       # each array null in turn
        args = [_p(rays), _p(hits), _p(pth)]
        args[k] = None
        assert step(_p(fake), *args, 4, 20, _p(rng), _p(lin), 8, None) == -1 and "null" in msg()
    assert cam(_p(fake), None, 4, None, None, _p(pth), None) == -1 and "null" in msg()
    assert cam(_p(fake), None, 4, None, _p(rays), None, None) == -1 and "null" in msg()
    for mb in (0, -1):
        assert step(_p(fake), _p(rays), _p(hits), _p(pth), 4, mb, _p(rng), _p(lin), 8, None) == -1 and "max_bounces" in msg()
    assert step(_p(fake), _p(rays), _p(hits), _p(pth), 4, 20, None, _p(lin), 8, None) == -1 and "null" in msg()
    assert step(_p(fake), _p(rays), _p(hits), _p(pth), 4, 20, _p(rng), None, 8, None) == -1 and "null" in msg()
    assert step(_p(fake), _p(rays), _p(hits), _p(pth), 4, 20, _p(rng), _p(lin), -1, None) == -1 and "n_pixels" in msg()
    off = C.c_void_p(rays.ctypes.data + 4)   # not 16-B aligned
    assert step(_p(fake), off, _p(hits), _p(pth), 4, 20, _p(rng), _p(lin), 8, None) == -1 and "aligned" in msg()
    assert cam(_p(fake), None, 4, None, off, _p(pth), None) == -1 and "aligned" in msg()
    assert cam(_p(fake), None, 4, None, _p(rays), _p(pth), None) == -1 and "no camera" in msg()
    # n == 0: CRT_OK, nothing launched, whatever the pointers
    assert step(_p(fake), None, None, None, 0, 20, None, None, 8, None) == 0
    assert cam(_p(fake), None, 0, None, None, None, None) == 0
