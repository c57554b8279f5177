"""The variance-guided filtering of the history, the host-only half (no GPU needed): header / exports /
optional bindings of the entries, the argument checks of the C entries and of the Python front-end, which all come before
any device use, and the numpy model of the rule (helpers/variance_model.py) on cases worked out by hand."""
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
import variance_model as vm  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
NEW = ("crt_renderer_reproject_moments", "crt_renderer_read_moments", "crt_renderer_denoise_history_variance",
       "crt_renderer_read_variance", "crt_selftest_reproject_moments", "crt_selftest_denoise_variance")
NEW_HOST = ("crth_viewer_set_denoise_variance",)
F32 = np.float32
INVALID, UNSUPPORTED = -1, -5
INF = float("inf")
NAN = float("nan")
TOL, CAP = 0.05, 32.0
DIRECT_ONLY = 0x80000000


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _msg():
    return _lib.hip().crt_last_error().decode()


# ------------------------------------------------------------------------------------------ header, exports, bindings
def _exports(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_new_names_declared_exported_bound():
    text = (REPO / "include" / "crt_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.hip()
    for lib in (_lib.HIP_LIB, REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"):
        assert set(NEW) <= _exports(lib), (lib, set(NEW) - _exports(lib))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.HIP_SYMBOLS and name in _lib.OPTIONAL_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    flat = re.sub(r"\s+", " ", header)
    assert re.search(r"typedef struct crt_denoise_variance_options \{ int32_t iterations; float sigma_luminance, sigma_normal, "
                     r"sigma_position; float min_history; uint32_t flags; int32_t reserved; \} crt_denoise_variance_options;", flat)
    assert C.sizeof(_lib.DenoiseVarianceOptions) == 28
    assert [f[0] for f in _lib.DenoiseVarianceOptions._fields_] == ["iterations", "sigma_luminance", "sigma_normal",
                                                                    "sigma_position", "min_history", "flags", "reserved"]
    # the existing structs and the ABI version stay as they were
    assert C.sizeof(_lib.ReprojectOptions) == 20 and C.sizeof(_lib.DenoiseOptions) == 24
    assert L.crt_abi_version() == 3 and _lib.ABI_VERSION == 3 and re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", header)
    for name in ("reproject_moments", "moments", "denoise_history_variance", "variance", "selftest_reproject_moments",
                 "selftest_denoise_variance"):
        assert callable(getattr(crt_amd.Renderer, name)), name
    # the header's words: every operation of the rule, the validity rule, what +inf does, what is out of scope
    block = text[text.index("---- variance-guided filtering"):text.index("typedef struct crt_denoise_variance_options")]
    for word in ("(0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z", "am = am + w * prev_m", "starts the whole history over",
                 "fmaxf(0.f, m2 - m1 * m1)", "(min_history / len)", "7 x 7", "hg = (1/4, 1/2, 1/4)",
                 "sigma_luminance * sqrtf(g) + 0x1p-20f", "av = av + (kw * kw) * qc.w", "av / (sw * sw)", "not halved",
                 "+inf", "no default", "crt_renderer_render_adaptive", "albedo"):
        assert word in block, word
    # the host library and the viewer
    host_header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "crt_host.h").read_text(), flags=re.S)
    for name in NEW_HOST:
        assert name in _exports(_lib.HOST_LIB) and name in _lib.HOST_SYMBOLS and re.search(r"\b%s\s*\(" % name, host_header)
        assert getattr(_lib.host(), name).argtypes is not None
    assert callable(crt_amd.Viewer.set_denoise_variance)


class _OlderLibrary:
    """A library of the same ABI version from before these entries: everything but them."""

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
    assert not any(hasattr(old, n) for n in NEW) and hasattr(old, "crt_renderer_reproject")
    for name in NEW:
        with pytest.raises(crt_amd.CrtError, match=name):
            _lib.require(name)
    r = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    z = lambda *s: np.zeros(s, F32)  # noqa: E731
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_reproject_moments"):
        r.reproject_moments(TOL, max_history=CAP, scale=1.0)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_read_moments"):
        r.moments()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_denoise_history_variance"):
        r.denoise_history_variance(4.0, INF, 0.05, min_history=4)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_read_variance"):
        r.variance()
    with pytest.raises(crt_amd.CrtError, match="crt_selftest_reproject_moments"):
        r.selftest_reproject_moments(z(4, 8, 3), z(4, 8, 8), z(4, 8, 8), None, None, z(19), TOL, max_history=CAP)
    with pytest.raises(crt_amd.CrtError, match="crt_selftest_denoise_variance"):
        r.selftest_denoise_variance(z(4, 8, 4), z(4, 8, 2), z(4, 8, 8), 4.0, INF, 0.05, min_history=4)
    monkeypatch.setattr(_lib, "_hip", real)
    assert _lib.require(NEW[0]) is getattr(real, NEW[0])


# ------------------------------------------------------------------------------------------ C argument checks
def _fake(device=0):
    """Stands in for a handle: a zeroed block whose first int is the handle's device.  Each call below is refused by a
    check that comes before anything else of the handle is read, except the pixel shard and the denoiser, reprojection
    and variance states, which the zeroed block answers with (0, 0) and "none"."""
    a = np.zeros(1 << 16, np.uint8)
    a[:4].view(np.int32)[0] = device
    return a


BAD_SIGMA = (NAN, 0.0, -1.0, -INF, 2.0 ** -51, float(np.nextafter(F32(2.0 ** -50), F32(0))), 2.0 ** 51,
             float(np.nextafter(F32(2.0 ** 50), F32(INF))))
GOOD_SIGMA = (INF, 2.0 ** -50, 2.0 ** 50, 1.0, 0.05)
BAD_TOL = BAD_SIGMA
BAD_NMIN = (NAN, INF, -1.5, 1.5, float(np.nextafter(F32(1), F32(2))), float(np.nextafter(F32(-1), F32(-2))))
BAD_CAP = (NAN, 0.0, -1.0, INF, -INF, float(np.nextafter(F32(1), F32(0))), 2.0 ** 24 + 2, 2.0 ** 30)
GOOD_CAP = (1.0, 2.0 ** 24, 32.0, 8.5)
BAD_MINH, GOOD_MINH = BAD_CAP, GOOD_CAP


def test_reproject_moments_rejects_what_reproject_rejects_before_any_device_use():
    fn = _lib.hip().crt_renderer_reproject_moments
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
    for kw in ({}, {"scale": 1 / 16}, {"tol": INF}, {"nmin": 0.9}, *({"cap": v} for v in GOOD_CAP)):
        assert call(**kw) == INVALID and "no guides" in _msg(), kw
    assert stats.pixels_reprojected == 0 and stats.reproject_ms == 0 and not rn[4:].any()


def test_denoise_history_variance_rejects_bad_arguments_before_any_device_use():
    fn = _lib.hip().crt_renderer_denoise_history_variance
    rn = _fake()
    stats = _lib.DenoiseStats()

    def call(r=rn, it=5, sl=4.0, sn=INF, sx=0.05, mh=4.0, flags=0, reserved=0, opts=True):
        o = _lib.DenoiseVarianceOptions(it, sl, sn, sx, mh, flags, reserved)
        return fn(None if r is None else _p(r), C.byref(o) if opts else None, C.byref(stats), None)

    assert call(r=None) == INVALID and "null" in _msg()
    assert call(opts=False) == INVALID and "null" in _msg()
    for it in (-1, 9, 100, -(1 << 31)):
        assert call(it=it) == INVALID and "iterations" in _msg(), it
    for name, key in (("sigma_luminance", "sl"), ("sigma_normal", "sn"), ("sigma_position", "sx")):
        for bad in BAD_SIGMA:
            assert call(**{key: bad}) == INVALID and name in _msg(), (name, bad)
    for bad in BAD_MINH:
        assert call(mh=bad) == INVALID and "min_history" in _msg(), bad
    for flags in (1, 2, 4, 1 << 30, 0xffffffff, DIRECT_ONLY | 1):
        assert call(flags=flags) == INVALID and "flag" in _msg(), flags
    for reserved in (1, -1, 1 << 20):
        assert call(reserved=reserved) == INVALID and "reserved" in _msg()
    # good values: the missing history is the complaint, and it names the entry that makes one
    for kw in ({}, {"it": 0}, {"it": 1}, {"it": 8}, {"flags": DIRECT_ONLY}, *({"sl": v} for v in GOOD_SIGMA),
               *({"sn": v} for v in GOOD_SIGMA), *({"sx": v} for v in GOOD_SIGMA), *({"mh": v} for v in GOOD_MINH)):
        assert call(**kw) == INVALID and "no history" in _msg() and "crt_renderer_reproject_moments" in _msg(), kw
    assert stats.filter_ms == 0 and stats.iterations == 0 and not rn[4:].any()
    # a history without valid moments and CRT_ERR_UNSUPPORTED for a pixel shard need a real handle: test_gpu_variance.py


def test_readers_and_selftests_reject_before_any_device_use():
    L = _lib.hip()
    rn = _fake()
    out = np.zeros(64, F32)
    assert L.crt_renderer_read_moments(_p(rn), _p(out)) == INVALID and "moments" in _msg()
    assert L.crt_renderer_read_moments(None, _p(out)) == INVALID and "null" in _msg()
    assert L.crt_renderer_read_moments(_p(rn), None) == INVALID and "null" in _msg()
    assert L.crt_renderer_read_variance(_p(rn), _p(out)) == INVALID and "no variance" in _msg()
    assert L.crt_renderer_read_variance(None, _p(out)) == INVALID and "null" in _msg()
    assert L.crt_renderer_read_variance(_p(rn), None) == INVALID and "null" in _msg()
    st = L.crt_selftest_reproject_moments
    o = _lib.ReprojectOptions(TOL, -INF, CAP, 0, 0)
    cam = _lib.CameraDesc()
    full = [_p(rn), _p(out), _p(out), _p(out), _p(out), _p(out), C.byref(cam), C.byref(o), _p(out), _p(out)]
    for k in (0, 1, 2, 3, 6, 7, 8, 9):                                 # 4 and 5, the previous frame, may be NULL together
        args = list(full)
        args[k] = None
        assert st(*args) == INVALID and "null" in _msg(), k
    args = list(full)
    args[5] = None                                                     # a previous history without its moments
    assert st(*args) == INVALID and "prev_moments" in _msg()
    for bad, word in ((_lib.ReprojectOptions(0.0, -INF, CAP, 0, 0), "position_tolerance"),
                      (_lib.ReprojectOptions(TOL, 2.0, CAP, 0, 0), "normal_min"),
                      (_lib.ReprojectOptions(TOL, -INF, 0.0, 0, 0), "max_history"),
                      (_lib.ReprojectOptions(TOL, -INF, CAP, 4, 0), "flag"),
                      (_lib.ReprojectOptions(TOL, -INF, CAP, 0, 1), "reserved")):
        args = list(full)
        args[7] = C.byref(bad)
        assert st(*args) == INVALID and word in _msg(), word
    sv = L.crt_selftest_denoise_variance
    good = _lib.DenoiseVarianceOptions(5, 4.0, INF, 0.05, 4.0, 0, 0)
    full = [_p(rn), _p(out), _p(out), _p(out), C.byref(good), _p(out), _p(out)]
    for k in range(7):
        args = list(full)
        args[k] = None
        assert sv(*args) == INVALID and "null" in _msg(), k
    for bad, word in ((_lib.DenoiseVarianceOptions(9, 4.0, INF, 0.05, 4.0, 0, 0), "iterations"),
                      (_lib.DenoiseVarianceOptions(5, 0.0, INF, 0.05, 4.0, 0, 0), "sigma_luminance"),
                      (_lib.DenoiseVarianceOptions(5, 4.0, NAN, 0.05, 4.0, 0, 0), "sigma_normal"),
                      (_lib.DenoiseVarianceOptions(5, 4.0, INF, -1.0, 4.0, 0, 0), "sigma_position"),
                      (_lib.DenoiseVarianceOptions(5, 4.0, INF, 0.05, 0.5, 0, 0), "min_history"),
                      (_lib.DenoiseVarianceOptions(5, 4.0, INF, 0.05, 4.0, 1, 0), "flag"),
                      (_lib.DenoiseVarianceOptions(5, 4.0, INF, 0.05, 4.0, 0, 7), "reserved")):
        args = list(full)
        args[4] = C.byref(bad)
        assert sv(*args) == INVALID and word in _msg(), word
    assert not rn[4:].any()


def test_existing_entries_still_refuse_their_flag_bits():
    """The feature added no bit to the existing option structs."""
    L = _lib.hip()
    rn = _fake()
    o = _lib.ReprojectOptions(TOL, -INF, CAP, 1, 0)
    assert L.crt_renderer_reproject(_p(rn), C.byref(o), C.c_float(1.0), None, None) == INVALID and "flag" in _msg()
    for flags in (2, 4, 1 << 30):
        d = _lib.DenoiseOptions(5, 4.0, INF, 0.05, flags, 0)
        assert L.crt_renderer_denoise_history(_p(rn), C.byref(d), None, None) == INVALID and "flag" in _msg()


def test_viewer_entry_and_cli_say_what_the_mode_needs():
    fn = _lib.host().crth_viewer_set_denoise_variance
    o = _lib.DenoiseVarianceOptions(5, 4.0, INF, 0.05, 4.0, 0, 0)
    assert fn(None, C.byref(o)) != 0 and b"null" in _lib.host().crth_last_error()
    viewer = REPO / "raytracer-cuda_amd" / "bin" / "crt_viewer"
    for args, word in ((["-denoise-variance", "4:inf:0.05:4"], "needs -reproject"),
                       (["-reproject", "0.05:-inf:32", "-denoise", "4:inf:0.05", "-denoise-variance", "4:inf:0.05:4"],
                        "exclude each other"),
                       (["-reproject", "0.05:-inf:32", "-denoise-variance", "4:inf:0.05"], "SL:SN:SX:MINH"),
                       (["-reproject", "0.05:-inf:32", "-denoise-iters", "3"], "needs -denoise")):
        res = subprocess.run([str(viewer), *args], capture_output=True, text=True)      # refused while parsing: no device
        assert res.returncode == 2 and word in res.stderr, (args, res.stderr)


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
    z = lambda *s: np.zeros(s, F32)  # noqa: E731
    c, g, hst, mom, cam = z(8, 16, 3), z(8, 16, 8), z(8, 16, 4), z(8, 16, 2), z(19)
    for name, bads in (("position_tolerance", BAD_TOL), ("normal_min", BAD_NMIN), ("max_history", BAD_CAP)):
        for bad in bads + (None, "x"):
            kw = dict(position_tolerance=TOL, normal_min=-INF, max_history=CAP)
            kw[name] = bad
            with pytest.raises(ValueError, match=name):
                r.reproject_moments(scale=1.0, **kw)
            with pytest.raises(ValueError, match=name):
                r.selftest_reproject_moments(c, g, g, hst, mom, cam, **kw)
    with pytest.raises(TypeError):
        r.reproject_moments(TOL, scale=1.0)                       # no default cap
    with pytest.raises(TypeError):
        r.reproject_moments(TOL, -INF, CAP, 1.0)                  # the cap and the scale by keyword only
    for scale in (None, NAN, 0.0, -1.0, "x"):
        with pytest.raises(ValueError, match="scale"):
            r.reproject_moments(TOL, max_history=CAP, scale=scale)
    for name, bads in (("sigma_luminance", BAD_SIGMA), ("sigma_normal", BAD_SIGMA), ("sigma_position", BAD_SIGMA),
                       ("min_history", BAD_MINH)):
        for bad in bads + (None, "x"):
            kw = dict(sigma_luminance=4.0, sigma_normal=INF, sigma_position=0.05, min_history=4.0)
            kw[name] = bad
            with pytest.raises(ValueError, match=name):
                r.denoise_history_variance(**kw)
            with pytest.raises(ValueError, match=name):
                r.selftest_denoise_variance(hst, mom, g, **kw)
    for bad in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="iterations"):
            r.denoise_history_variance(4.0, INF, 0.05, min_history=4, iterations=bad)
    with pytest.raises(TypeError):
        r.denoise_history_variance(4.0, INF, 0.05)                # no default min_history
    with pytest.raises(TypeError):
        r.denoise_history_variance(4.0, INF, 0.05, 4.0)           # and by keyword only
    with pytest.raises(TypeError):
        r.denoise_history_variance(4.0, INF, min_history=4.0)     # no default sigmas
    with pytest.raises(ValueError, match="history"):
        r.selftest_denoise_variance(z(8, 16, 3), mom, g, 4.0, INF, 0.05, min_history=4)
    with pytest.raises(ValueError, match="moments"):
        r.selftest_denoise_variance(hst, z(8, 16, 1), g, 4.0, INF, 0.05, min_history=4)
    with pytest.raises(ValueError, match="guides"):
        r.selftest_denoise_variance(hst, mom, z(8, 16, 7), 4.0, INF, 0.05, min_history=4)
    with pytest.raises(ValueError, match="color"):
        r.selftest_reproject_moments(z(8, 8, 3), g, g, hst, mom, cam, TOL, max_history=CAP)
    with pytest.raises(ValueError, match="prev_moments"):
        r.selftest_reproject_moments(c, g, g, hst, None, cam, TOL, max_history=CAP)
    with pytest.raises(ValueError, match="prev_moments"):
        r.selftest_reproject_moments(c, g, g, hst, z(8, 16, 3), cam, TOL, max_history=CAP)
    with pytest.raises(ValueError, match="prev_camera"):
        r.selftest_reproject_moments(c, g, g, hst, mom, z(3), TOL, max_history=CAP)
    v = crt_amd.Viewer.__new__(crt_amd.Viewer)
    v.h = None
    for kw, word in ((dict(sigma_luminance=0.0, sigma_normal=INF, sigma_position=0.05, min_history=4), "sigma_luminance"),
                     (dict(sigma_luminance=4.0, sigma_normal=INF, sigma_position=None, min_history=4), "sigma_position"),
                     (dict(sigma_luminance=4.0, sigma_normal=INF, sigma_position=0.05), "min_history"),
                     (dict(sigma_luminance=4.0, sigma_normal=INF, sigma_position=0.05, min_history=4, iterations=0),
                      "iterations")):
        with pytest.raises(ValueError, match=word):
            v.set_denoise_variance(**kw)


# ------------------------------------------------------------------------------------------ the model, by hand
W, H = 16, 9


def _cam(**kw):
    import pyoracle
    return pyoracle.camera(**kw)


def _wall(cam, w=W, h=H, key=0, normal=(0, 0, 1), z=-1.0):
    o, d = dm.centre_rays(cam, w, h)
    t = ((F32(z) - o[:, 2]) / d[:, 2]).astype(F32).reshape(h, w)
    return rm.camera_guides(cam, w, h, t, normal, np.full((h, w), key, np.int32))


def _flat_guides(w, h, key=0):
    """One key, equal normals and positions: with the normal and position terms on or off every geometric X is 0."""
    k = np.full((h, w), key, np.int32) if np.isscalar(key) else np.asarray(key, np.int32)
    return dm.pack_guides(np.zeros((h, w, 3), F32), np.ones((h, w), F32), np.zeros((h, w, 3), F32), k)


def _rows(c, length):
    c = np.asarray(c, F32)
    return np.concatenate([c, np.broadcast_to(np.asarray(length, F32), c.shape[:2])[..., None]], axis=-1).astype(F32)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_model_lum_and_first_call_moments_are_exact():
    g = np.random.default_rng(5)
    c = (g.random((H, W, 3)) * 4).astype(F32)
    l = vm.lum(c)
    by_hand = F32(F32(F32(0.2126) * c[2, 3, 0]) + F32(F32(0.7152) * c[2, 3, 1])) + F32(F32(0.0722) * c[2, 3, 2])
    assert l[2, 3] == F32(by_hand)
    hist, mom, taken = vm.reproject_moments(c, _wall(_cam()), None, None, None, None, TOL, -INF, CAP)
    assert not taken.any() and np.array_equal(_bits(hist[..., 0:3]), _bits(c)) and (hist[..., 3] == 1).all()
    assert np.array_equal(_bits(mom[..., 0]), _bits(l)) and np.array_equal(_bits(mom[..., 1]), _bits((l * l).astype(F32)))


def test_model_still_camera_blends_the_moments_with_the_colours_weight():
    cam = _cam()
    g = _wall(cam)
    prev_c, new_c = np.full((H, W, 3), 2.0, F32), np.full((H, W, 3), 4.0, F32)      # lum of a grey c is c up to a few ulps
    pm = vm.frame_moments(prev_c)
    hist, mom, taken = vm.reproject_moments(new_c, g, g, _rows(prev_c, 1.0), pm, cam, TOL, -INF, CAP)
    ref, _ = rm.reproject(new_c, g, g, _rows(prev_c, 1.0), cam, TOL, -INF, CAP)
    assert taken.all() and np.array_equal(_bits(hist), _bits(ref))                  # the history is the plain entry's
    assert (hist[..., 0:3] == 3).all() and (hist[..., 3] == 2).all()                # a = 1 / 2
    nm = vm.frame_moments(new_c)
    # the taps' weights sum to 1 within a few ulps and every tap holds the same row: hm = pm within 4 ulps, a = 1 / 2
    want = pm.astype(np.float64) + (nm.astype(np.float64) - pm) * 0.5
    assert np.abs(mom - want).max() <= 8 * 2.0 ** -24 * want.max()
    # a longer history: len 3 -> m = 4, a = 1 / 4, for the moments as for the colours
    hist, mom, _ = vm.reproject_moments(new_c, g, g, _rows(prev_c, 3.0), pm, cam, TOL, -INF, CAP)
    a = 1.0 / hist[..., 3].astype(np.float64)
    assert np.abs(a - 0.25).max() < 1e-6
    want = pm.astype(np.float64) + (nm.astype(np.float64) - pm) * a[..., None]
    assert np.abs(mom - want).max() <= 8 * 2.0 ** -24 * want.max()
    # a restarted pixel (another key in the previous frame) takes the frame's own moments
    hist, mom, taken = vm.reproject_moments(new_c, g, _wall(cam, key=1), _rows(prev_c, 3.0), pm, cam, TOL, -INF, CAP)
    assert not taken.any() and np.array_equal(_bits(mom), _bits(nm)) and (hist[..., 3] == 1).all()


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6, 7, 8])
def test_model_a_constant_frame_without_variance_comes_back_exactly(iterations):
    w, h = 40, 23
    hist = _rows(np.ones((h, w, 3), F32), 8.0)
    l1 = vm.lum(np.ones((1, 1, 3), F32))[0, 0]
    mom = np.broadcast_to(np.array([l1, F32(l1 * l1)], F32), (h, w, 2)).copy()
    out, v0 = vm.denoise_variance(hist, mom, _flat_guides(w, h), 4.0, 1.0, 1.0, 4.0, iterations)
    # m2 - m1 * m1 = RN(l1 * l1) - RN(l1 * l1) = 0; every tap has X = 0, w = 1, kw = k: acc and sw are the same sums of
    # multiples of 1/256, exact in float32, so acc / sw = 1
    assert (v0 == 0).all() and (_bits(out) == _bits(F32(1))).all()


def test_model_flat_interior_scales_the_variance_by_the_squared_kernel_sum():
    w, h = 15, 13
    v = F32(0.37)
    g = _flat_guides(w, h)
    c = np.full((h, w, 3), 0.5, F32)
    res = vm.filter_steps(c, np.full((h, w), v, F32), g, INF, INF, INF, (1,))[1]
    want = float(v) * (70.0 / 256.0) ** 2
    inner = res[1][2:-2, 2:-2]
    # sw = 1 exactly (sums of multiples of 1/256), so v' = av: 25 products (k * k) * v, each rounded once (k * k is
    # exact), and 25 additions, each rounding a partial sum that is at most the result: a relative error of at most
    # 26 * 2^-24 in all, plus half an ulp of the division by sw * sw = 1 (exact): 27 half-ulps bound it
    assert np.abs(inner.astype(np.float64) - want).max() <= 27 * 2.0 ** -24 * want
    assert (res[0] == F32(0.5)).all()
    # with the luminance term on and every colour equal, xc = 0: the same bits
    res_l = vm.filter_steps(c, np.full((h, w), v, F32), g, 4.0, INF, INF, (1,))[1]
    assert np.array_equal(_bits(res_l[1]), _bits(res[1]))
    # near the border the taken taps are fewer: sw < 1 and v' is larger than in the interior
    assert res[1][0, 0] > inner[0, 0]


def test_model_a_luminance_step_is_kept_or_blurred_as_the_variance_says():
    w, h, edge = 24, 9, 12
    c = np.full((h, w, 3), 0.2, F32)
    c[:, edge:] = 0.8
    g = _flat_guides(w, h)
    at = []
    vs = (1e-8, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 10.0)
    for v in vs:
        out = vm.filter_steps(c, np.full((h, w), v, F32), g, 4.0, INF, INF, (1,))[1][0]
        at.append(float(out[4, edge - 1, 0]))
    # v = 1e-8: den = 4e-4 + 2^-20, xc = 0.6 / den > 1000: !(X < 80), every tap of the far side is skipped
    assert abs(at[0] - 0.2) <= 4 * 2.0 ** -24 and at[-1] > 0.35
    assert all(b >= a for a, b in zip(at, at[1:])) and at[-1] > at[0] + 0.15
    # v = 10: den = 12.6, xc = 0.047, w = 0.95: close to the plain 5 x 5 mean of the step at that pixel, (11 * 0.2 + 5 * 0.8) / 16
    assert abs(at[-1] - (11 * 0.2 + 5 * 0.8) / 16) < 0.02
    # with the term off the step is blurred whatever v says
    off = vm.filter_steps(c, np.full((h, w), 1e-8, F32), g, INF, INF, INF, (1,))[1][0]
    assert abs(float(off[4, edge - 1, 0]) - (11 * 0.2 + 5 * 0.8) / 16) < 1e-6


def test_model_short_history_takes_the_window_and_long_history_its_own_moments():
    w, h = 20, 14
    rng = np.random.default_rng(11)
    m1 = (rng.random((h, w)) + 0.5).astype(F32)
    mom = np.stack([m1, (m1 * m1 + rng.random((h, w)) * 0.3).astype(F32)], axis=-1).astype(F32)
    key = np.zeros((h, w), np.int32)
    key[:, 13:] = 3
    length = np.full((h, w), 8.0, F32)
    length[6, 9], length[6, 14], length[0, 0] = 2.0, 1.0, 3.0
    mom[5, 8] = [NAN, 1.0]                                      # a tap whose moments are not finite is not taken
    v = vm.estimate(_rows(np.zeros((h, w, 3), F32), length), mom, key, 4.0)

    def spatial(y, x):
        ys, xs = slice(max(y - 3, 0), y + 4), slice(max(x - 3, 0), x + 4)
        ok = (key[ys, xs] == key[y, x]) & np.isfinite(mom[ys, xs]).all(axis=-1)
        a, b = mom[ys, xs, 0][ok].astype(np.float64), mom[ys, xs, 1][ok].astype(np.float64)
        return max(0.0, b.mean() - a.mean() ** 2) * (4.0 / float(length[y, x])), int(ok.sum())

    # (6, 9): the 49 taps reach column 12, all of key 0, less the NaN tap; (6, 14): the columns 13 .. 17 of key 3, 7 rows;
    # (0, 0): the 4 x 4 taps inside the frame
    for (y, x), n in (((6, 9), 48), ((6, 14), 35), ((0, 0), 16)):
        want, taken = spatial(y, x)
        assert taken == n, taken
        # sums of <= 49 values near 1: about 50 roundings of 2^-24 on a difference of two numbers near 1.5
        assert abs(float(v[y, x]) - want) <= 100 * 2.0 ** -24 * 2.0 * (4.0 / float(length[y, x])), (y, x)
        assert want > 0
    long_ = length >= 4
    own = np.fmax(F32(0), (mom[..., 1] - (mom[..., 0] * mom[..., 0]).astype(F32)).astype(F32))
    assert np.array_equal(_bits(v[long_]), _bits(own[long_]))    # (5, 8): fmaxf(0, NaN) = 0
    assert v[5, 8] == 0 and not np.isnan(v).any()
    # the long branch ignores the neighbours: change them all, the pixel's v stays
    other = mom.copy()
    other[7:10, 2:5] += 1
    other[8, 3] = mom[8, 3]
    assert vm.estimate(_rows(np.zeros((h, w, 3), F32), length), other, key, 4.0)[8, 3] == v[8, 3]
    # n == 0: a short pixel whose own moments are not finite and which is alone with its key
    key2, len2 = key.copy(), length.copy()
    key2[5, 8], len2[5, 8] = 9, 1.0
    assert vm.estimate(_rows(np.zeros((h, w, 3), F32), len2), mom, key2, 4.0)[5, 8] == 0


def test_model_a_nan_colour_stays_alone():
    w, h = 40, 30
    rng = np.random.default_rng(2)
    c = (rng.random((h, w, 3)) * 2).astype(F32)
    for bad in (NAN, INF, -INF):
        cb = c.copy()
        cb[14, 20, 1] = bad
        mom = vm.frame_moments(cb)
        assert not np.isfinite(mom[14, 20]).any()
        length = np.full((h, w), 8.0, F32)
        length[10:20, 15:25] = 2.0                               # short histories round it, the long branch elsewhere
        steps, v0 = vm.denoise_variance_steps(_rows(cb, length), mom, _flat_guides(w, h), 4.0, INF, INF, 4.0,
                                              (1, 2, 3, 4, 5))
        assert np.isfinite(v0).all()
        others = np.ones((h, w), bool)
        others[14, 20] = False
        for n, out in steps.items():
            assert np.isfinite(out[others]).all(), (bad, n)
            assert not np.isfinite(out[14, 20, 1]), (bad, n)


def test_model_an_infinite_variance_switches_the_luminance_term_off_around_it():
    w, h = 20, 16
    rng = np.random.default_rng(9)
    c = (rng.random((h, w, 3)) + 0.5).astype(F32)
    v = np.full((h, w), 0.01, F32)
    v[8, 10] = INF
    g = _flat_guides(w, h)
    on = vm.filter_steps(c, v, g, 4.0, INF, INF, (1, 3))
    off = vm.filter_steps(c, v, g, INF, INF, INF, (1,))
    ring = np.zeros((h, w), bool)
    ring[7:10, 9:12] = True
    # g = +inf within +-1 of it: inv_den = 0, xc = 0 for every tap, the pixel is filtered as with the term off
    assert np.array_equal(_bits(on[1][0][ring]), _bits(off[1][0][ring]))
    assert not np.array_equal(_bits(on[1][0][~ring]), _bits(off[1][0][~ring]))
    for n in (1, 3):
        assert np.isfinite(on[n][0]).all()                       # no colour becomes non-finite
    assert np.isinf(on[1][1][8, 10]) and np.isinf(on[1][1][8, 12])           # the +inf travels in v: every tap that takes it
    assert np.isfinite(on[1][1][8, 13])
    # from the moments: an m2 that overflowed gives v = +inf through the long branch
    mom = np.broadcast_to(np.array([1.0, 2.0], F32), (h, w, 2)).copy()
    mom[8, 10, 1] = INF
    v0 = vm.estimate(_rows(c, 8.0), mom, np.zeros((h, w), np.int32), 4.0)
    assert np.isinf(v0[8, 10]) and np.isfinite(np.delete(v0.reshape(-1), 8 * w + 10)).all()


def test_model_validity_rules():
    cam = _cam()
    g = _wall(cam)
    rng = np.random.default_rng(4)
    frames = [(rng.random((H, W, 3)) + 0.5).astype(F32) for _ in range(6)]
    s = vm.HistoryState()
    assert not s.reproject_moments(frames[0], g, cam, TOL, -INF, CAP).any() and s.moments_valid
    assert s.reproject_moments(frames[1], g, cam, TOL, -INF, CAP).all() and (s.history[..., 3] == 2).all()
    # the history rows are the plain entry's from the same state
    plain = vm.HistoryState()
    plain.reproject(frames[0], g, cam, TOL, -INF, CAP)
    plain.reproject(frames[1], g, cam, TOL, -INF, CAP)
    assert np.array_equal(_bits(plain.history), _bits(s.history)) and not plain.moments_valid
    # a plain reprojection keeps the history going and ends the moments
    assert s.reproject(frames[2], g, cam, TOL, -INF, CAP).all() and (s.history[..., 3] == 3).all() and not s.moments_valid
    # the next reproject_moments starts the whole history over: (c, 1), (l, l * l)
    taken = s.reproject_moments(frames[3], g, cam, TOL, -INF, CAP)
    assert not taken.any() and (s.history[..., 3] == 1).all() and np.array_equal(_bits(s.history[..., 0:3]), _bits(frames[3]))
    assert np.array_equal(_bits(s.moments), _bits(vm.frame_moments(frames[3]))) and s.moments_valid
    assert s.reproject_moments(frames[4], g, cam, TOL, -INF, CAP).all() and (s.history[..., 3] == 2).all()
    # reset_history ends both
    s.reset()
    assert not s.valid and not s.moments_valid
    assert not s.reproject_moments(frames[5], g, cam, TOL, -INF, CAP).any() and (s.history[..., 3] == 1).all()
