"""Adaptive sampling, the host-only half (no GPU needed): header / exports / optional bindings of the
entries, the argument checks of the C entry and of the Python front-end, which all come before any device use, and the
numpy model of the plan step (helpers/adaptive_model.py) on cases worked out by hand."""
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
import adaptive_model as am  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
NEW = ("crt_renderer_render_adaptive", "crt_renderer_resolve_adaptive", "crt_renderer_read_tile_spp",
       "crt_renderer_read_tile_error", "crt_renderer_read_adaptive_prev", "crt_selftest_adaptive_plan")
F32 = np.float32
INVALID, UNSUPPORTED = -1, -5
INF = float("inf")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


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
    assert re.search(r"typedef struct crt_adaptive_options \{ int32_t spp_min, spp_max; float tolerance; int32_t reserved; \}", header)
    assert re.search(r"typedef struct crt_adaptive_stats \{ uint64_t samples; uint32_t passes, tiles_refined, tiles_at_max; float ms; \}", header)
    assert C.sizeof(_lib.AdaptiveOptions) == 16 and C.sizeof(_lib.AdaptiveStats) == 24
    assert L.crt_abi_version() == 3 and _lib.ABI_VERSION == 3 and re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", header)
    for name in ("render_adaptive", "resolve_adaptive", "tile_spp", "tile_error", "adaptive_prev", "selftest_adaptive_plan"):
        assert callable(getattr(crt_amd.Renderer, name)), name


class _OlderLibrary:
    """A library of the same ABI version from before the adaptive entries: everything but them."""

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
    assert not any(hasattr(old, n) for n in NEW) and hasattr(old, "crt_renderer_render_wavefront_finish")
    for name in NEW:
        with pytest.raises(crt_amd.CrtError, match=name):
            _lib.require(name)
    scene = crt_amd.Scene(None, 0)
    r = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_render_adaptive"):
        r.render_adaptive(scene, 4, 32, 0.1)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_resolve_adaptive"):
        r.resolve_adaptive()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_read_tile_spp"):
        r.tile_spp()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_read_tile_error"):
        r.tile_error()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_read_adaptive_prev"):
        r.adaptive_prev()
    with pytest.raises(crt_amd.CrtError, match="crt_selftest_adaptive_plan"):
        r.selftest_adaptive_plan(np.zeros((4, 8, 3), F32), np.zeros((4, 8, 3), F32), np.zeros((1, 1), np.int32), 2, 4, 0.0)
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


def test_render_adaptive_rejects_bad_arguments_before_any_device_use():
    fn = _lib.hip().crt_renderer_render_adaptive
    sc, rn = _fake(), _fake()
    stats = _lib.AdaptiveStats()

    def call(r=rn, scene=sc, spp_min=4, spp_max=32, tol=0.1, reserved=0, mb=20, flags=0, opts=True):
        o = _lib.AdaptiveOptions(spp_min, spp_max, tol, reserved)
        return fn(None if r is None else _p(r), None if scene is None else _p(scene), C.byref(o) if opts else None, mb,
                  flags, C.byref(stats), None)

    assert call(r=None) == INVALID and "null" in _msg()
    assert call(scene=None) == INVALID and "null" in _msg()
    assert call(opts=False) == INVALID and "null" in _msg()
    for lo in (0, 1, 3, 5, -2, -4):
        assert call(spp_min=lo) == INVALID and "spp_min" in _msg(), lo
    for lo, hi in ((4, 2), (8, 6), (2, 0), (2, -1)):
        assert call(spp_min=lo, spp_max=hi) == INVALID and "spp_max" in _msg()
    assert call(tol=float("nan")) == INVALID and "NaN" in _msg()
    for mb in (0, -1):
        assert call(mb=mb) == INVALID and "max_bounces" in _msg()
    for reserved in (4, 8, -1):
        assert call(reserved=reserved) == INVALID and "reserved" in _msg()
    for flags in (1, 2, 3, 4):                       # ACCUMULATE, COUNT_WORK, both, an unknown one
        assert call(flags=flags) == UNSUPPORTED and "flag" in _msg()
    assert call(scene=_fake(1)) == INVALID and "different devices" in _msg()
    # good values: the camera is the complaint
    for kw in ({}, {"tol": INF}, {"tol": -1.0}, {"tol": 0.0}, {"spp_min": 2, "spp_max": 2}, {"spp_max": 24}, {"reserved": 1},
               {"reserved": 3}):
        assert call(**kw) == INVALID and "camera" in _msg(), kw
    assert stats.samples == 0 and stats.passes == 0 and not rn[4:].any() and not sc[4:].any()
    # the readers and the resolve before any adaptive call on the handle
    out = np.zeros(64, F32)
    L = _lib.hip()
    for name in ("crt_renderer_read_tile_spp", "crt_renderer_read_tile_error", "crt_renderer_read_adaptive_prev"):
        assert getattr(L, name)(_p(rn), _p(out)) == INVALID and "no adaptive render" in _msg()
        assert getattr(L, name)(None, _p(out)) == INVALID
    assert L.crt_renderer_resolve_adaptive(_p(rn), None) == INVALID and "no adaptive render" in _msg()
    assert L.crt_renderer_resolve_adaptive(None, None) == INVALID
    lst, cnt = np.zeros(4, np.uint32), C.c_uint32(0)
    plan = L.crt_selftest_adaptive_plan
    assert plan(None, _p(out), _p(out), _p(out), 2, 4, 0.0, _p(lst), C.byref(cnt)) == INVALID and "null" in _msg()
    assert plan(_p(rn), None, _p(out), _p(out), 2, 4, 0.0, _p(lst), C.byref(cnt)) == INVALID and "null" in _msg()
    for n, nxt in ((3, 4), (0, 4), (4, 2)):
        assert plan(_p(rn), _p(out), _p(out), _p(out), n, nxt, 0.0, _p(lst), C.byref(cnt)) == INVALID and "even" in _msg()
    assert plan(_p(rn), _p(out), _p(out), _p(out), 2, 4, float("nan"), _p(lst), C.byref(cnt)) == INVALID and "NaN" in _msg()


# ------------------------------------------------------------------------------------------ Python argument checks
@pytest.fixture
def no_library(monkeypatch):
    """Any look-up of an entry fails the test: the checks below must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "require", boom)
    monkeypatch.setattr(_lib, "hip", boom)


def test_python_front_end_rejects(no_library):
    scene, r = crt_amd.Scene(None, 0), crt_amd.Renderer._borrow(None, 16, 8, 0, None)
    for lo in (0, 1, 3, -2, 2.0, True, None):
        with pytest.raises(ValueError, match="spp_min"):
            r.render_adaptive(scene, lo, 32, 0.1)
    for hi in (2, 3, 1 << 31, 8.0, None):
        with pytest.raises(ValueError, match="spp_max"):
            r.render_adaptive(scene, 4, hi, 0.1)
    for tol in (float("nan"), None, "x"):
        with pytest.raises(ValueError, match="tolerance"):
            r.render_adaptive(scene, 4, 32, tol)
    with pytest.raises(TypeError):
        r.render_adaptive(scene, 4, 32)                     # no default tolerance
    for mb in (0, -1, 1.5):
        with pytest.raises(ValueError, match="max_bounces"):
            r.render_adaptive(scene, 4, 32, 0.1, max_bounces=mb)
    with pytest.raises(ValueError, match="Scene"):
        r.render_adaptive(None, 4, 32, 0.1)
    with pytest.raises(ValueError, match="different devices"):
        r.render_adaptive(crt_amd.Scene(None, 1), 4, 32, 0.1)
    z, t = np.zeros((8, 16, 3), F32), np.zeros((1, 2), np.int32)
    with pytest.raises(ValueError, match="sum and prev"):
        r.selftest_adaptive_plan(z[:4], z, t, 2, 4, 0.0)
    with pytest.raises(ValueError, match="sum and prev"):
        r.selftest_adaptive_plan(z, z[:, :8], t, 2, 4, 0.0)
    with pytest.raises(ValueError, match="tile_spp"):
        r.selftest_adaptive_plan(z, z, np.zeros(3, np.int32), 2, 4, 0.0)
    for n, nxt in ((3, 4), (0, 2), (4, 2)):
        with pytest.raises(ValueError, match="even"):
            r.selftest_adaptive_plan(z, z, t, n, nxt, 0.0)
    with pytest.raises(ValueError, match="NaN"):
        r.selftest_adaptive_plan(z, z, t, 2, 4, float("nan"))


# ------------------------------------------------------------------------------------------ the model, by hand
def test_model_tiles_and_lanes():
    assert am.tiles(64, 36) == (5, 8) and am.tiles(7, 5) == (1, 1) and am.tiles(136, 136) == (17, 17)
    assert am.tiles(2560, 1440) == (180, 320)
    c = am.in_frame(64, 36)
    assert c.shape == (40,) and (c[:32] == 64).all() and (c[32:] == 32).all() and c.sum() == 64 * 36
    assert am.in_frame(7, 5).tolist() == [35]
    c = am.in_frame(37, 19)
    assert c.reshape(3, 5).tolist() == [[64] * 4 + [40], [64] * 4 + [40], [24] * 4 + [15]]
    x, y, valid = am.lane_pixels(37, 19)
    assert (x[7, 9], y[7, 9]) == (2 * 8 + 1, 1 * 8 + 1) and valid[7, 9]       # tile 7 = (tx 2, ty 1), lane 9 = (1, 1)
    assert valid.sum() == 37 * 19 and valid[14].sum() == 15
    a = np.arange(19 * 37 * 3, dtype=F32).reshape(19, 37, 3)
    pl = am.per_lane(a, 37, 19)
    assert (pl[7, 9] == a[9, 17]).all() and not pl[14][~valid[14]].any()


def test_model_butterfly_adds_pairs_not_a_running_sum():
    v = np.zeros((1, 64), F32)
    v[0, :4] = [2.0 ** 24, 1, 1, 1]
    # pairs: (2^24 + 1) -> 2^24 (a tie, to even), (1 + 1) = 2, then 2^24 + 2; a running sum would stay at 2^24
    out = am.butterfly(v)
    assert (out == F32(2.0 ** 24 + 2)).all()
    seq = F32(0)
    for e in v[0]:
        seq = F32(seq + e)
    assert seq == F32(2.0 ** 24)
    r = np.random.default_rng(3).random((5, 64)).astype(F32)
    out = am.butterfly(r)
    assert (out == out[:, :1]).all()                                         # every lane holds the same sum
    k1 = (r[:, 0::2] + r[:, 1::2]).astype(F32)
    k2 = (k1[:, 0::2] + k1[:, 1::2]).astype(F32)
    k4 = (k2[:, 0::2] + k2[:, 1::2]).astype(F32)
    k8 = (k4[:, 0::2] + k4[:, 1::2]).astype(F32)
    k16 = (k8[:, 0::2] + k8[:, 1::2]).astype(F32)
    assert (out[:, 0] == (k16[:, 0] + k16[:, 1]).astype(F32)).all()


def test_model_pixel_term_by_hand():
    # S = (8, 4, 4) after n = 4 samples, P = (6, 2, 2) after the first two: Q = (2, 2, 2), d = 4, I = 16 / 4 = 4,
    # e = (4 / 2) / sqrt(4) = 1
    assert am.pixel_terms(np.array([8, 4, 4], F32), np.array([6, 2, 2], F32), 4) == F32(1)
    # n = 8: I = 2, e = (4 / 4) / sqrt(2)
    assert am.pixel_terms(np.array([8, 4, 4], F32), np.array([6, 2, 2], F32), 8) == F32(1) / np.sqrt(F32(2))
    # I <= 0 (zero and negative sums) and a NaN sum give 0; an infinite sum gives NaN (inf / inf)
    assert am.pixel_terms(np.zeros(3, F32), np.zeros(3, F32), 4) == 0
    assert am.pixel_terms(np.array([-8, 1, 1], F32), np.array([6, 2, 2], F32), 4) == 0
    assert am.pixel_terms(np.array([np.nan, 1, 1], F32), np.array([6, 2, 2], F32), 4) == 0
    assert np.isnan(am.pixel_terms(np.array([np.inf, 1, 1], F32), np.array([6, 2, 2], F32), 4))
    # the three differences are added as (x + y) + z: 2^24 + 1 + 1 stays at 2^24 that way round, and becomes 2^24 + 2
    # as x + (y + z); I = (2^24 + 2) / 2, so the term is exactly 2^24 / sqrt(I)
    s, p = np.array([2.0 ** 24, 1, 1], F32), np.zeros(3, F32)
    i = F32(F32(F32(s[0] + s[1]) + s[2]) / F32(2))
    assert i == F32(2.0 ** 23) and am.pixel_terms(s, p, 2) == F32(2.0 ** 24) / np.sqrt(i)


def test_model_plan_by_hand():
    w, h = 16, 5                               # two tiles of 40 pixels
    s = np.tile(np.array([8, 4, 4], F32), (h, w, 1))
    p = np.tile(np.array([6, 2, 2], F32), (h, w, 1))
    p[:, 8:] = [4, 2, 2]                       # tile 1: Q = (4, 2, 2) = P, d = 0
    spp = np.array([4, 4], np.int32)
    old = np.array([7, 7], F32)
    assert am.tile_errors(s, p, 4).tolist() == [1.0, 0.0]          # 40 x 1 / 40: exact
    err, spp1, prev1, listed = am.plan(s, p, spp, old, 4, 8, 1.0)  # E == tolerance converges
    assert err.tolist() == [1.0, 0.0] and spp1.tolist() == [4, 4] and listed.size == 0 and (prev1 == p).all()
    err, spp1, prev1, listed = am.plan(s, p, spp, old, 4, 8, 0.5)
    assert spp1.tolist() == [8, 4] and listed.tolist() == [0]
    assert (prev1[:, :8] == s[:, :8]).all() and (prev1[:, 8:] == p[:, 8:]).all()
    err, spp1, prev1, listed = am.plan(s, p, spp, old, 4, 6, -1.0)  # a negative tolerance converges nothing
    assert spp1.tolist() == [6, 6] and listed.tolist() == [0, 1] and (prev1 == s).all()
    err, spp1, prev1, listed = am.plan(s, p, spp, old, 4, 8, INF)
    assert spp1.tolist() == [4, 4] and listed.size == 0 and err.tolist() == [1.0, 0.0]
    err, spp1, prev1, listed = am.plan(s, p, np.array([4, 8], np.int32), old, 8, 16, -1.0)   # only tiles at n
    assert err.tolist() == [7.0, 0.0] and spp1.tolist() == [4, 16] and listed.tolist() == [1]
    assert (prev1[:, :8] == p[:, :8]).all()
    s2 = s.copy()
    s2[2, 3] = [np.inf, 1, 1]                  # one infinite pixel: the tile's error is NaN, and a NaN is unconverged
    err, spp1, _, listed = am.plan(s2, p, spp, old, 4, 8, INF)
    assert np.isnan(err[0]) and err[1] == 0 and spp1.tolist() == [8, 4] and listed.tolist() == [0]
    assert am.canon(err).tolist() == [0x7fc00000, 0]


def test_model_predicts_a_loop_by_hand():
    w, h = 16, 8
    px = {2: (6, 2, 2), 4: (8, 4, 4), 8: (16, 8, 8), 16: (32, 16, 16)}
    frames = {k: np.tile(np.array(v, F32), (h, w, 1)) for k, v in px.items()}
    frames[2][:, 8:] = [4, 2, 2]               # tile 1 has equal halves at n = 4: it converges at once
    # tile 0: n = 4: E = 1; n = 8: P = (8, 4, 4), Q = (8, 4, 4): E = 0
    spp, err, stats = am.predict(frames, 4, 16, 0.5)
    assert spp.tolist() == [8, 4] and err.tolist() == [0.0, 0.0]
    assert stats == {"samples": 64 * 8 + 64 * 4, "passes": 1, "tiles_refined": 1, "tiles_at_max": 0}
    spp, err, stats = am.predict(frames, 4, 16, -1.0)
    assert spp.tolist() == [16, 16] and stats["passes"] == 2 and stats["tiles_at_max"] == 2
    spp, err, stats = am.predict(frames, 4, 16, INF)
    assert spp.tolist() == [4, 4] and err.tolist() == [1.0, 0.0] and stats["passes"] == 0 and stats["samples"] == 128 * 4
    spp, err, stats = am.predict(frames, 4, 12, -1.0)       # a maximum that is no power of two: 4 -> 8 -> 12
    assert spp.tolist() == [12, 12] and stats["passes"] == 2 and stats["tiles_at_max"] == 2
    spp, err, stats = am.predict(frames, 4, 4, -1.0)        # nothing to refine: no plan
    assert spp.tolist() == [4, 4] and stats["passes"] == 0 and stats["tiles_at_max"] == 2 and not err.any()
    assert am.expand(np.array([8, 4]), w, h)[3].tolist() == [8] * 8 + [4] * 8
