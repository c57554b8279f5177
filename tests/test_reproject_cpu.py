"""The reprojection, the host-only half (no GPU needed): header / exports / optional bindings of the
entries, the argument checks of the C entries and of the Python front-end, which all come before any device use, the numpy
model of the rule (helpers/reproject_model.py) on cases worked out by hand, and the history's effect on oracle frames."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import denoise_model as dm  # noqa: E402
import reproject_model as rm  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
NEW = ("crt_renderer_reproject", "crt_renderer_reset_history", "crt_renderer_denoise_history", "crt_renderer_resolve_history",
       "crt_renderer_read_history", "crt_renderer_history_device_ptr", "crt_selftest_reproject")
NEW_HOST = ("crth_viewer_set_reproject",)
F32 = np.float32
INVALID, UNSUPPORTED = -1, -5
INF = float("inf")
NAN = float("nan")
TOL, CAP = 0.05, 32.0


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _msg():
    return _lib.hip().crt_last_error().decode()


# ------------------------------------------------------------------------------------------ header, exports, bindings
def _exports(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_new_names_declared_exported_bound():
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "crt_hip.h").read_text(), flags=re.S)
    L = _lib.hip()
    for lib in (_lib.HIP_LIB, REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"):
        assert set(NEW) <= _exports(lib), (lib, set(NEW) - _exports(lib))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.HIP_SYMBOLS and name in _lib.OPTIONAL_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    flat = re.sub(r"\s+", " ", header)
    assert re.search(r"typedef struct crt_reproject_options \{ float position_tolerance; float normal_min; float max_history; "
                     r"uint32_t flags; int32_t reserved; \} crt_reproject_options;", flat)
    assert re.search(r"typedef struct crt_reproject_stats \{ float reproject_ms; uint32_t pixels_reprojected, pixels_hit; \}", flat)
    assert C.sizeof(_lib.ReprojectOptions) == 20 and C.sizeof(_lib.ReprojectStats) == 12
    assert [f[0] for f in _lib.ReprojectOptions._fields_] == ["position_tolerance", "normal_min", "max_history", "flags",
                                                             "reserved"]
    assert L.crt_abi_version() == 3 and _lib.ABI_VERSION == 3 and re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", header)
    for name in ("reproject", "history", "resolve_history", "history_device_ptr", "reset_history", "denoise_history",
                 "selftest_reproject"):
        assert callable(getattr(crt_amd.Renderer, name)), name
    # the header's words: the naming, no defaults, the bias
    text = (REPO / "include" / "crt_hip.h").read_text()
    block = text[text.index("---- reprojection"):text.index("typedef struct crt_reproject_options")]
    for word in ("temporal tile order", "no defaults", "pixel footprints", "biased", "fminf(hist.len + 1.f, max_history)",
                 "s = LN / dot(d, N)"):
        assert word in block, word
    # the host library and the viewer
    host_header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "crt_host.h").read_text(), flags=re.S)
    for name in NEW_HOST:
        assert name in _exports(_lib.HOST_LIB) and name in _lib.HOST_SYMBOLS and re.search(r"\b%s\s*\(" % name, host_header)
        assert getattr(_lib.host(), name).argtypes is not None
    assert callable(crt_amd.Viewer.set_reproject)


class _OlderLibrary:
    """A library of the same ABI version from before the reprojection's entries: everything but them."""

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
    assert not any(hasattr(old, n) for n in NEW) and hasattr(old, "crt_renderer_denoise")
    for name in NEW:
        with pytest.raises(crt_amd.CrtError, match=name):
            _lib.require(name)
    r = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_reproject"):
        r.reproject(TOL, max_history=CAP, scale=1.0)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_read_history"):
        r.history()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_resolve_history"):
        r.resolve_history()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_history_device_ptr"):
        r.history_device_ptr()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_reset_history"):
        r.reset_history()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_denoise_history"):
        r.denoise_history(1.0, 1.0, 1.0)
    with pytest.raises(crt_amd.CrtError, match="crt_selftest_reproject"):
        r.selftest_reproject(np.zeros((4, 8, 3), F32), np.zeros((4, 8, 8), F32), np.zeros((4, 8, 8), F32), None,
                             np.zeros(19, F32), TOL, max_history=CAP)
    monkeypatch.setattr(_lib, "_hip", real)
    assert _lib.require(NEW[0]) is getattr(real, NEW[0])


# ------------------------------------------------------------------------------------------ C argument checks
def _fake(device=0):
    """Stands in for a handle: a zeroed block whose first int is the handle's device.  Each call below is refused by a
    check that comes before anything else of the handle is read, except the pixel shard, the denoiser state and the
    reprojection state, which the zeroed block answers with (0, 0) and "none"."""
    a = np.zeros(1 << 16, np.uint8)
    a[:4].view(np.int32)[0] = device
    return a


BAD_TOL = (NAN, 0.0, -1.0, -INF, 2.0 ** -51, float(np.nextafter(F32(2.0 ** -50), F32(0))), 2.0 ** 51,
           float(np.nextafter(F32(2.0 ** 50), F32(INF))))
GOOD_TOL = (INF, 2.0 ** -50, 2.0 ** 50, 1.0, 0.05)
BAD_NMIN = (NAN, INF, -1.5, 1.5, float(np.nextafter(F32(1), F32(2))), float(np.nextafter(F32(-1), F32(-2))))
GOOD_NMIN = (-INF, -1.0, 1.0, 0.0, 0.9)
BAD_CAP = (NAN, 0.0, -1.0, INF, -INF, float(np.nextafter(F32(1), F32(0))), 2.0 ** 24 + 2, 2.0 ** 30)
GOOD_CAP = (1.0, 2.0 ** 24, 32.0, 8.5)


def test_reproject_rejects_bad_arguments_before_any_device_use():
    fn = _lib.hip().crt_renderer_reproject
    rn = _fake()
    stats = _lib.ReprojectStats()

    def call(r=rn, tol=TOL, nmin=-INF, cap=CAP, flags=0, reserved=0, scale=1.0, opts=True):
        o = _lib.ReprojectOptions(tol, nmin, cap, flags, reserved)
        return fn(None if r is None else _p(r), C.byref(o) if opts else None, C.c_float(scale), C.byref(stats), None)

    assert call(r=None) == INVALID and "null" in _msg()
    assert call(opts=False) == INVALID and "null" in _msg()
    for bad in BAD_TOL:
        assert call(tol=bad) == INVALID and "position_tolerance" in _msg(), bad
    for bad in BAD_NMIN:
        assert call(nmin=bad) == INVALID and "normal_min" in _msg(), bad
    for bad in BAD_CAP:
        assert call(cap=bad) == INVALID and "max_history" in _msg(), bad
    for flags in (1, 2, 1 << 31, 0xffffffff):
        assert call(flags=flags) == INVALID and "flag" in _msg(), flags
    for reserved in (1, -1, 1 << 20):
        assert call(reserved=reserved) == INVALID and "reserved" in _msg()
    for scale in (NAN, 0.0, -0.0, -1.0, -INF):
        assert call(scale=scale) == INVALID and "scale" in _msg(), scale
    # good values: the missing guides are the complaint
    for kw in ({}, {"scale": 1 / 16}, {"scale": INF}, *({"tol": v} for v in GOOD_TOL), *({"nmin": v} for v in GOOD_NMIN),
               *({"cap": v} for v in GOOD_CAP)):
        assert call(**kw) == INVALID and "no guides" in _msg(), kw
    assert stats.pixels_reprojected == 0 and stats.reproject_ms == 0 and not rn[4:].any()
    # CRT_ERR_UNSUPPORTED for a pixel shard other than (0, 1) needs a handle that has one: tests/test_gpu_reproject.py


def test_readers_consumers_and_selftest_reject_before_any_device_use():
    L = _lib.hip()
    rn = _fake()
    out = np.zeros(64, F32)
    assert L.crt_renderer_read_history(_p(rn), _p(out)) == INVALID and "no history" in _msg()
    assert L.crt_renderer_read_history(None, _p(out)) == INVALID
    assert L.crt_renderer_read_history(_p(rn), None) == INVALID
    assert L.crt_renderer_resolve_history(_p(rn), None) == INVALID and "no history" in _msg()
    assert L.crt_renderer_resolve_history(None, None) == INVALID
    assert L.crt_renderer_history_device_ptr(None) is None and L.crt_renderer_history_device_ptr(_p(rn)) is None
    assert L.crt_renderer_reset_history(None) == INVALID and "null" in _msg()
    assert L.crt_renderer_reset_history(_p(rn)) == 0                  # nothing to reset
    dh = L.crt_renderer_denoise_history
    good = _lib.DenoiseOptions(5, 4.0, INF, 0.05, 0, 0)
    assert dh(None, C.byref(good), None, None) == INVALID and "null" in _msg()
    assert dh(_p(rn), None, None, None) == INVALID and "null" in _msg()
    assert dh(_p(rn), C.byref(good), None, None) == INVALID and "no history" in _msg()
    for bad, word in ((_lib.DenoiseOptions(9, 4.0, INF, 0.05, 0, 0), "iterations"),
                      (_lib.DenoiseOptions(5, 0.0, INF, 0.05, 0, 0), "sigma_color"),
                      (_lib.DenoiseOptions(5, 4.0, INF, 0.05, 2, 0), "flag"),
                      (_lib.DenoiseOptions(5, 4.0, INF, 0.05, 0, 7), "reserved"),
                      (_lib.DenoiseOptions(5, 4.0, INF, 0.05, 1, 0), "tile scale")):
        assert dh(_p(rn), C.byref(bad), None, None) == INVALID and word in _msg(), word
    st = L.crt_selftest_reproject
    o = _lib.ReprojectOptions(TOL, -INF, CAP, 0, 0)
    cam = _lib.CameraDesc()
    full = [_p(rn), _p(out), _p(out), _p(out), _p(out), C.byref(cam), C.byref(o), _p(out)]
    for k in (0, 1, 2, 3, 5, 6, 7):                                    # 4, the previous history, may be NULL
        args = list(full)
        args[k] = None
        assert st(*args) == INVALID and "null" in _msg(), k
    for bad, word in ((_lib.ReprojectOptions(0.0, -INF, CAP, 0, 0), "position_tolerance"),
                      (_lib.ReprojectOptions(TOL, 2.0, CAP, 0, 0), "normal_min"),
                      (_lib.ReprojectOptions(TOL, -INF, 0.0, 0, 0), "max_history"),
                      (_lib.ReprojectOptions(TOL, -INF, CAP, 4, 0), "flag"),
                      (_lib.ReprojectOptions(TOL, -INF, CAP, 0, 1), "reserved")):
        args = list(full)
        args[6] = C.byref(bad)
        assert st(*args) == INVALID and word in _msg(), word
    assert not rn[4:].any()


def test_viewer_entry_rejects_null_arguments():
    fn = _lib.host().crth_viewer_set_reproject
    o = _lib.ReprojectOptions(TOL, -INF, CAP, 0, 0)
    assert fn(None, C.byref(o), None) != 0 and b"null" in _lib.host().crth_last_error()


# ------------------------------------------------------------------------------------------ Python argument checks
@pytest.fixture
def no_library(monkeypatch):
    """Any look-up of an entry fails the test: the checks below must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "require", boom)
    monkeypatch.setattr(_lib, "hip", boom)
    monkeypatch.setattr(_lib, "host", boom)


def test_python_front_end_rejects(no_library):
    r = crt_amd.Renderer._borrow(None, 16, 8, 0, None)
    c, g, hst, cam = np.zeros((8, 16, 3), F32), np.zeros((8, 16, 8), F32), np.zeros((8, 16, 4), F32), np.zeros(19, F32)
    for name, bads in (("position_tolerance", BAD_TOL), ("normal_min", BAD_NMIN), ("max_history", BAD_CAP)):
        for bad in bads + (None, "x"):
            kw = dict(position_tolerance=TOL, normal_min=-INF, max_history=CAP)
            kw[name] = bad
            with pytest.raises(ValueError, match=name):
                r.reproject(scale=1.0, **kw)
            with pytest.raises(ValueError, match=name):
                r.selftest_reproject(c, g, g, hst, cam, **kw)
    with pytest.raises(TypeError):
        r.reproject(TOL, scale=1.0)                               # no default cap
    with pytest.raises(TypeError):
        r.reproject(max_history=CAP, scale=1.0)                   # no default tolerance
    with pytest.raises(TypeError):
        r.reproject(TOL, -INF, CAP, 1.0)                          # the cap and the scale by keyword only
    for scale in (None, NAN, 0.0, -1.0, "x"):
        with pytest.raises(ValueError, match="scale"):
            r.reproject(TOL, max_history=CAP, scale=scale)
    for name in ("sigma_color", "sigma_normal", "sigma_position"):
        kw = dict(sigma_color=4.0, sigma_normal=INF, sigma_position=0.05)
        kw[name] = 0.0
        with pytest.raises(ValueError, match=name):
            r.denoise_history(**kw)
    with pytest.raises(ValueError, match="iterations"):
        r.denoise_history(4.0, INF, 0.05, iterations=9)
    with pytest.raises(TypeError):
        r.denoise_history(4.0, INF, 0.05, tile_scale=True)        # no tile scale here
    with pytest.raises(ValueError, match="color"):
        r.selftest_reproject(np.zeros((8, 8, 3), F32), g, g, hst, cam, TOL, max_history=CAP)
    with pytest.raises(ValueError, match="guides"):
        r.selftest_reproject(c, g, np.zeros((8, 16, 7), F32), hst, cam, TOL, max_history=CAP)
    with pytest.raises(ValueError, match="prev_history"):
        r.selftest_reproject(c, g, g, np.zeros((8, 16, 3), F32), cam, TOL, max_history=CAP)
    with pytest.raises(ValueError, match="prev_camera"):
        r.selftest_reproject(c, g, g, hst, np.zeros(3, F32), TOL, max_history=CAP)
    v = crt_amd.Viewer.__new__(crt_amd.Viewer)
    v.h = None
    for kw, word in ((dict(position_tolerance=0.0, max_history=CAP), "position_tolerance"),
                     (dict(position_tolerance=TOL, max_history=0.0), "max_history"),
                     (dict(position_tolerance=TOL, max_history=CAP, denoise=(4.0, INF)), "denoise"),
                     (dict(position_tolerance=TOL, max_history=CAP, denoise=(0.0, INF, 0.05)), "sigma_color")):
        with pytest.raises(ValueError, match=word):
            v.set_reproject(**kw)


# ------------------------------------------------------------------------------------------ the model, by hand
W, H = 16, 9


def _cam(**kw):
    import pyoracle
    return pyoracle.camera(**kw)


def _wall(cam, w=W, h=H, key=0, normal=(0, 0, 1), z=-1.0):
    """Guides of the wall at height z seen from `cam` (at z = 0.3, looking down -z): fronto-parallel for the default
    camera."""
    o, d = dm.centre_rays(cam, w, h)
    t = ((F32(z) - o[:, 2]) / d[:, 2]).astype(F32).reshape(h, w)
    return rm.camera_guides(cam, w, h, t, normal, np.full((h, w), key, np.int32))


def _const(v, length=None, w=W, h=H):
    a = np.full((h, w, 3 if length is None else 4), v, F32)
    if length is not None:
        a[..., 3] = length
    return a


def test_model_first_call_is_the_frame_itself():
    g = np.random.default_rng(3)
    c = (g.random((H, W, 3)) * 4 - 1).astype(F32)
    c[2, 3, 1], c[4, 5, 0] = NAN, INF
    out, taken = rm.reproject(c, _wall(_cam()), None, None, None, TOL, -INF, CAP)
    assert np.array_equal(dm.canon(out[..., 0:3]), dm.canon(c)) and (out[..., 3].view(np.uint32) == 0x3f800000).all()
    assert not taken.any()


def test_model_projection_of_an_unchanged_camera_is_the_pixel_itself_within_a_few_ulps():
    for w, h in ((W, H), (64, 36), (37, 19), (264, 260)):
        cam = _cam()
        g = _wall(cam, w, h)
        s, fx, fy = rm.project(g[..., 4:7], cam, w, h)
        ys, xs = np.mgrid[0:h, 0:w]
        # u and v each come out of about 16 roundings of relative size 2^-24 on values of size <= 1 (d, s, q, two dots,
        # a quotient), then scale by the frame's size: 2^-20 of it, plus one ulp of the result
        assert np.abs(fx - xs).max() <= w * 2.0 ** -20 and np.abs(fy - ys).max() <= h * 2.0 ** -20, (w, h)
        assert (s > 0).all()


def test_model_unchanged_camera_blends_constant_images_exactly():
    cam = _cam()
    g = _wall(cam)
    out, taken = rm.reproject(_const(4.0), g, g, _const(2.0, 1.0), cam, TOL, -INF, CAP)
    assert taken.all()
    assert (out[..., 0:3].view(np.uint32) == F32(3).view(np.uint32)).all()        # 2 + (4 - 2) * (1 / 2)
    assert (out[..., 3].view(np.uint32) == F32(2).view(np.uint32)).all()
    # other powers of two, and a longer history whose length is one too: 8 + (0.5 - 8) / 4, with m = 3 + 1 from len = 3
    # only up to the rounding of w * 3 in the taps' sum (a few ulps), so take len = 1 and a cap of 1.5: a = 1 / 1.5
    out, _ = rm.reproject(_const(0.5), g, g, _const(8.0, 2.0), cam, TOL, 0.5, CAP)
    assert (out[..., 0:3] == F32(F32(8) + F32(F32(-7.5) * F32(F32(1) / F32(3))))).all() and (out[..., 3] == 3).all()
    out, _ = rm.reproject(_const(0.5), g, g, _const(8.0, 1.0), cam, TOL, 0.5, 1.5)
    assert (out[..., 0:3] == F32(F32(8) + F32(F32(-7.5) * F32(F32(1) / F32(1.5))))).all() and (out[..., 3] == 1.5).all()


def test_model_length_stops_at_the_cap():
    cam = _cam()
    g = _wall(cam)
    hist, lengths = None, []
    for k in range(7):
        hist, _ = rm.reproject(_const(1.0), g, g, hist, cam, TOL, -INF, 4.0)
        lengths.append(float(hist[3, 5, 3]))
        # 1, 2 and 3 are exact (w * 1 and w * 2 are); from there the taps' sum of w * len rounds: a few ulps
        assert np.abs(hist[..., 3] - hist[3, 5, 3]).max() <= 4 * 2.0 ** -22 and (hist[..., 0:3] == 1).all()
        assert (hist[..., 3] <= 4).all()
    assert lengths[:3] == [1, 2, 3] and all(abs(v - 4) <= 4 * 2.0 ** -22 for v in lengths[3:])
    # at the cap the blend weight stays 1 / max_history: an exponential mean.  2 -> 2 + (6 - 2) / 4 = 3
    out, _ = rm.reproject(_const(6.0), g, g, _const(2.0, 4.0), cam, TOL, -INF, 4.0)
    assert (out[..., 0:3] == 3).all() and (out[..., 3] == 4).all()
    out, _ = rm.reproject(_const(6.0), g, g, _const(2.0, 4.0), cam, TOL, -INF, 1.0)
    assert (out[..., 0:3] == 6).all() and (out[..., 3] == 1).all()          # a cap of 1: the frame itself


def test_model_a_camera_moved_by_one_pixel_footprint_shifts_the_history_by_one_pixel():
    cam = _cam()
    g = _wall(cam)
    footprint = float(g[0, 1, 4] - g[0, 0, 4])                  # of a pixel on the wall, signed: world x per pixel
    assert abs(footprint) > 0.01
    prev_cam = _cam(pos=(-footprint, 0.0, 0.3))                 # every point was one pixel further along x
    pg = _wall(prev_cam)
    hist = _const(0.0, 1.0)
    hist[..., 0:3] = (np.arange(W, dtype=F32) * 2)[None, :, None]
    out, taken = rm.reproject(_const(0.0), g, pg, hist, prev_cam, TOL, -INF, CAP)
    s, fx, fy = rm.project(g[..., 4:7], prev_cam, W, H)
    xs = np.arange(W)[None, :]
    assert np.abs(fx - (xs + 1)).max() < 1e-4 and np.abs(fy - np.arange(H)[:, None]).max() < 1e-4
    assert taken[:, :W - 1].all()
    # out = hist(x + 1) / 2 up to the bilinear weights' few ulps
    assert np.abs(out[:, :W - 1, 0] - (xs[:, :W - 1] + 1)).max() < 1e-4 and (out[:, :W - 1, 3] == 2).all()


def test_model_each_failed_test_restarts_the_pixel():
    cam = _cam()
    g = _wall(cam)
    hist, c = _const(2.0, 5.0), _const(4.0)

    def restarted(out, taken):
        return not taken.any() and (out[..., 0:3] == 4).all() and (out[..., 3] == 1).all()

    assert rm.reproject(c, g, g, hist, cam, TOL, 0.0, CAP)[1].all()                         # the base case takes it all
    assert restarted(*rm.reproject(c, g, _wall(cam, key=1), hist, cam, TOL, -INF, CAP))     # another key
    far = _wall(cam, z=-2.0)                                                                # the same pixels, 1 further
    assert restarted(*rm.reproject(c, g, far, hist, cam, TOL, -INF, CAP))
    assert rm.reproject(c, g, far, hist, cam, INF, -INF, CAP)[1].all()                      # ... unless the term is off
    flipped = _wall(cam, normal=(0, 0, -1))
    assert restarted(*rm.reproject(c, g, flipped, hist, cam, TOL, 0.0, CAP))
    assert rm.reproject(c, g, flipped, hist, cam, TOL, -1.0, CAP)[1].all()                  # dot = -1 >= -1
    assert rm.reproject(c, g, flipped, hist, cam, TOL, -INF, CAP)[1].all()
    behind = _cam(yaw=90.0)                                                                 # looks the other way
    s, _, _ = rm.project(g[..., 4:7], behind, W, H)
    assert (s < 0).all() and restarted(*rm.reproject(c, g, g, hist, behind, INF, -INF, CAP))
    narrow, turned = _cam(vfov=30.0), _cam(vfov=30.0, yaw=-30.0)                            # 60 degrees apart, in front
    gn = _wall(narrow)
    s, fx, fy = rm.project(gn[..., 4:7], turned, W, H)
    assert (s > 0).all() and ((fx <= -1) | (fx >= W)).all()
    assert restarted(*rm.reproject(c, gn, gn, hist, turned, INF, -INF, CAP))


def test_model_a_term_that_is_off_ignores_an_infinite_guide():
    cam = _cam()
    g = _wall(cam)
    hist, c = _const(2.0, 1.0), _const(4.0)
    pg = g.copy()
    pg[3, 4, 4:7] = [INF, 0, -INF]                      # an infinite previous position
    pg[5, 6, 0:3] = [NAN, INF, 0]                       # and a previous normal that is no number
    base, _ = rm.reproject(c, g, g, hist, cam, INF, -INF, CAP)
    out, taken = rm.reproject(c, g, pg, hist, cam, INF, -INF, CAP)
    assert taken.all() and np.array_equal(out.view(np.uint32), base.view(np.uint32))
    out, taken = rm.reproject(c, g, pg, hist, cam, TOL, 0.0, CAP)       # on: those two taps fail, nothing else does
    assert np.isfinite(out).all() and (out[..., 0:3][taken] == 3).all() and taken.sum() >= W * H - 2


def test_model_a_bad_sample_lives_for_one_frame():
    cam = _cam()
    g = _wall(cam)
    for bad in (NAN, INF, -INF):
        c = _const(4.0)
        c[4, 7, 1] = bad
        h1, _ = rm.reproject(c, g, g, _const(2.0, 1.0), cam, TOL, -INF, CAP)
        assert np.array_equal(dm.canon(h1[4, 7]), dm.canon(np.array([4, bad, 4, 1], F32)))      # shown as it is, len 1
        others = np.ones((H, W), bool)
        others[4, 7] = False
        assert (h1[others][:, 0:3] == 3).all()
        h2, taken = rm.reproject(_const(4.0), g, g, h1, cam, TOL, -INF, CAP)
        assert np.isfinite(h2).all()                                  # gone: no tap took it
        assert (h2[others][:, 3] == 3).all() and h2[4, 7, 3] <= 3      # len 2 -> 3 everywhere else
        assert h2[4, 7, 3] == 1 or taken[4, 7]                        # restarted, or served by its neighbours' few ulps


def test_model_a_nan_history_tap_is_skipped_and_the_others_serve():
    cam = _cam()
    g = _wall(cam)
    footprint = float(g[0, 1, 4] - g[0, 0, 4])
    prev_cam = _cam(pos=(-footprint / 2, 0.0, 0.3))     # half a pixel: two taps of about equal weight
    pg = _wall(prev_cam)
    hist = _const(2.0, 1.0)
    hist[:, 5, 0] = NAN
    # the taps lie half a footprint from the point: a tolerance above that (at 16 pixels' width a footprint is wide)
    assert 0.5 * abs(footprint) < 0.2 * 1.3
    out, taken = rm.reproject(_const(2.0), g, pg, hist, prev_cam, 0.2, -INF, CAP)
    assert np.isfinite(out).all() and taken[:, 3:7].all()
    assert np.abs(out[:, 3:7, 0:3] - 2).max() < 1e-6 and (np.abs(out[:, 3:7, 3] - 2) < 1e-6).all()


def test_model_misses_never_take_or_give_history():
    cam = _cam()
    g, pg = _wall(cam), _wall(cam)
    g[2, 3], pg[2, 3] = dm.miss_record(), dm.miss_record()      # a miss in both frames: equal keys, still no history
    pg[6, 10] = dm.miss_record()                                # a miss then, a hit now
    g[1, 12] = dm.miss_record()                                 # a hit then, a miss now
    out, taken = rm.reproject(_const(4.0), g, pg, _const(2.0, 7.0), cam, INF, -INF, CAP)
    for y, x in ((2, 3), (1, 12)):
        assert not taken[y, x] and (out[y, x] == [4, 4, 4, 1]).all()
    # the hit whose own previous pixel was a miss takes at most its neighbours' few ulps, never the miss's row
    hist = _const(2.0, 7.0)
    hist[6, 10] = [1000, 1000, 1000, 1]
    out, taken = rm.reproject(_const(4.0), g, pg, hist, cam, INF, -INF, CAP)
    assert out[6, 10, 0] <= 4 and (out[6, 10, 3] == 1 or taken[6, 10])


# ------------------------------------------------------------------------------------------ quality against the oracle
@pytest.mark.parametrize("name", ["cornell_bunny", "cornell"])
def test_the_history_lowers_the_error_of_a_moving_oracle_camera(oracle_scenes, name):
    """8 frames of 1 spp, seeds 41 .. 48, yaw -93.5 .. -90 in steps of 0.5, guides from the oracle's trace with zero
    normals, tolerance 0.05, cap 32; RMS on linear values against 512 spp (seed 1234) from the last camera."""
    import pyoracle
    w, h = 64, 36
    o = oracle_scenes[name]
    hist = prev = None
    for k in range(8):
        cam = pyoracle.camera(yaw=-93.5 + 0.5 * k)
        raw = o.render(cam, w, h, 1, 20, seed=41 + k)[0].astype(F32)
        ro, rd = dm.centre_rays(cam, w, h)
        t, prim = o.trace(ro, rd)
        hit = t >= 0
        key = np.where(hit, prim[:, 0], dm.MISS_KEY).astype(np.int32)
        pos = (ro + (t[:, None] * rd).astype(F32)).astype(F32)
        pos[~hit] = 0
        guides = dm.pack_guides(np.zeros((h, w, 3), F32), t.reshape(h, w), pos.reshape(h, w, 3), key.reshape(h, w))
        hist, taken = rm.reproject(raw, guides, None if prev is None else prev[0], hist, None if prev is None else prev[1],
                                   TOL, -INF, CAP)
        prev = (guides, cam)
    ref = o.render(cam, w, h, 512, 20, seed=1234)[0].astype(np.float64) / 512
    filtered = dm.denoise(hist[..., 0:3], guides, 4.0, INF, 0.05, 4)

    def rms(a):
        return float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))

    print(f"{name}: raw RMS {rms(raw):.4f}, history {rms(hist[..., 0:3]):.4f}, a-trous of raw "
          f"{rms(dm.denoise(raw, guides, 4.0, INF, 0.05, 4)):.4f}, a-trous of history {rms(filtered):.4f}, "
          f"reprojected {int(taken.sum())} / hit {int(hit.sum())}")
    assert np.isfinite(filtered).all()
    assert rms(hist[..., 0:3]) < rms(raw) and rms(filtered) < rms(hist[..., 0:3])
    assert taken.sum() >= 0.99 * hit.sum()
