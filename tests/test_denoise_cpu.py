"""The denoiser, the host-only half (no GPU needed): header / exports / optional bindings of the entries,
the argument checks of the C entries and of the Python front-end, which all come before any device use, the numpy model
of the filter (helpers/denoise_model.py) on cases worked out by hand, and the filter's effect on an oracle frame."""
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

REPO = Path(__file__).resolve().parents[1]
NEW = ("crt_renderer_compute_guides", "crt_renderer_denoise", "crt_renderer_resolve_denoised", "crt_renderer_read_denoised",
       "crt_renderer_read_guides", "crt_renderer_denoised_device_ptr", "crt_selftest_denoise",
       "crt_renderer_denoise_iteration_ms")
F32 = np.float32
INVALID, UNSUPPORTED = -1, -5
INF = float("inf")
NAN = float("nan")


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
    flat = re.sub(r"\s+", " ", header)
    assert re.search(r"typedef struct crt_denoise_options \{ int32_t iterations; float sigma_color, sigma_normal, "
                     r"sigma_position; uint32_t flags; int32_t reserved; \} crt_denoise_options;", flat)
    assert re.search(r"typedef struct crt_denoise_stats \{ float guides_ms, filter_ms; uint32_t iterations, pixels_hit; \}", flat)
    assert re.search(r"#define\s+CRT_DENOISE_TILE_SCALE\s+1u", header)
    assert C.sizeof(_lib.DenoiseOptions) == 24 and C.sizeof(_lib.DenoiseStats) == 16
    assert [f[0] for f in _lib.DenoiseOptions._fields_] == ["iterations", "sigma_color", "sigma_normal", "sigma_position",
                                                           "flags", "reserved"]
    assert L.crt_abi_version() == 3 and _lib.ABI_VERSION == 3 and re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", header)
    for name in ("compute_guides", "guides", "denoise", "denoised", "resolve_denoised", "denoised_device_ptr",
                 "selftest_denoise", "denoise_iteration_ms"):
        assert callable(getattr(crt_amd.Renderer, name)), name


class _OlderLibrary:
    """A library of the same ABI version from before the denoiser's entries: everything but them."""

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
    assert not any(hasattr(old, n) for n in NEW) and hasattr(old, "crt_renderer_render_adaptive")
    for name in NEW:
        with pytest.raises(crt_amd.CrtError, match=name):
            _lib.require(name)
    scene = crt_amd.Scene(None, 0)
    r = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_compute_guides"):
        r.compute_guides(scene)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_read_guides"):
        r.guides()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_denoise"):
        r.denoise(1.0, 1.0, 1.0, scale=1.0)
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_read_denoised"):
        r.denoised()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_resolve_denoised"):
        r.resolve_denoised()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_denoised_device_ptr"):
        r.denoised_device_ptr()
    with pytest.raises(crt_amd.CrtError, match="crt_renderer_denoise_iteration_ms"):
        r.denoise_iteration_ms()
    with pytest.raises(crt_amd.CrtError, match="crt_selftest_denoise"):
        r.selftest_denoise(np.zeros((4, 8, 3), F32), np.zeros((4, 8, 8), F32), 1.0, 1.0, 1.0)
    monkeypatch.setattr(_lib, "_hip", real)
    assert _lib.require(NEW[0]) is getattr(real, NEW[0])


# ------------------------------------------------------------------------------------------ C argument checks
def _fake(device=0):
    """Stands in for a handle: a zeroed block whose first int, the handle's device in both structs, is `device`.  Each
    call below is refused by a check that comes before anything else of the handle is read, except has_camera, the
    adaptive state and the denoiser state, which the zeroed block answers with "none"."""
    a = np.zeros(1 << 16, np.uint8)
    a[:4].view(np.int32)[0] = device
    return a


BAD_SIGMAS = (NAN, 0.0, -1.0, -INF, 2.0 ** -51, float(np.nextafter(F32(2.0 ** -50), F32(0))), 2.0 ** 51,
              float(np.nextafter(F32(2.0 ** 50), F32(INF))))
GOOD_SIGMAS = (INF, 2.0 ** -50, 2.0 ** 50, 1.0, 0.05)


def test_denoise_rejects_bad_arguments_before_any_device_use():
    fn = _lib.hip().crt_renderer_denoise
    rn = _fake()
    stats = _lib.DenoiseStats()

    def call(r=rn, iters=5, sc=4.0, sn=INF, sx=0.05, flags=0, reserved=0, scale=1.0, opts=True):
        o = _lib.DenoiseOptions(iters, sc, sn, sx, flags, reserved)
        return fn(None if r is None else _p(r), C.byref(o) if opts else None, C.c_float(scale), C.byref(stats), None)

    assert call(r=None) == INVALID and "null" in _msg()
    assert call(opts=False) == INVALID and "null" in _msg()
    for iters in (-1, 9, 100, -(1 << 31)):
        assert call(iters=iters) == INVALID and "iterations" in _msg(), iters
    for name in ("sc", "sn", "sx"):
        for bad in BAD_SIGMAS:
            assert call(**{name: bad}) == INVALID and "sigma_" in _msg(), (name, bad)
    assert call(sc=NAN) == INVALID and "sigma_color" in _msg()
    assert call(sn=0.0) == INVALID and "sigma_normal" in _msg()
    assert call(sx=-1.0) == INVALID and "sigma_position" in _msg()
    for flags in (2, 4, 1 << 30, 3, 0x7ffffffe):
        assert call(flags=flags) == INVALID and "flag" in _msg(), flags
    for reserved in (1, -1, 1 << 20):
        assert call(reserved=reserved) == INVALID and "reserved" in _msg()
    for scale in (NAN, 0.0, -0.0, -1.0, -INF):
        assert call(scale=scale) == INVALID and "scale" in _msg(), scale
    # the tile scale without adaptive state; with it the scale is not looked at, so a bad one is not the complaint
    assert call(flags=1) == INVALID and "adaptive" in _msg()
    assert call(flags=1, scale=NAN) == INVALID and "adaptive" in _msg()
    assert call(flags=1 | (1 << 31)) == INVALID and "adaptive" in _msg()
    # good values: the missing guides are the complaint
    for kw in ({}, {"iters": 0}, {"iters": 1}, {"iters": 8}, {"flags": 1 << 31}, {"scale": 1 / 16}, {"scale": INF},
               *({"sc": s, "sn": s, "sx": s} for s in GOOD_SIGMAS)):
        assert call(**kw) == INVALID and "no guides" in _msg(), kw
    assert stats.iterations == 0 and stats.filter_ms == 0 and not rn[4:].any()


def test_guides_readers_and_selftest_reject_before_any_device_use():
    L = _lib.hip()
    sc, rn = _fake(), _fake()
    fn = L.crt_renderer_compute_guides
    assert fn(None, _p(sc), None, None) == INVALID and "null" in _msg()
    assert fn(_p(rn), None, None, None) == INVALID and "null" in _msg()
    assert fn(_p(rn), _p(_fake(1)), None, None) == INVALID and "different devices" in _msg()
    assert fn(_p(rn), _p(sc), None, None) == INVALID and "camera" in _msg()
    o = _lib.TraceOptions()
    assert fn(_p(rn), _p(sc), C.byref(o), None) == INVALID and "camera" in _msg()
    out = np.zeros(64, F32)
    assert L.crt_renderer_read_guides(_p(rn), _p(out)) == INVALID and "no guides" in _msg()
    assert L.crt_renderer_read_guides(None, _p(out)) == INVALID
    assert L.crt_renderer_read_guides(_p(rn), None) == INVALID
    assert L.crt_renderer_read_denoised(_p(rn), _p(out)) == INVALID and "no denoised" in _msg()
    assert L.crt_renderer_read_denoised(None, _p(out)) == INVALID
    assert L.crt_renderer_resolve_denoised(_p(rn), None) == INVALID and "no denoised" in _msg()
    assert L.crt_renderer_resolve_denoised(None, None) == INVALID
    assert L.crt_renderer_denoise_iteration_ms(_p(rn), _p(out)) == INVALID and "stats pointer" in _msg()
    assert L.crt_renderer_denoise_iteration_ms(None, _p(out)) == INVALID
    assert L.crt_renderer_denoise_iteration_ms(_p(rn), None) == INVALID
    assert L.crt_renderer_denoised_device_ptr(None) is None and L.crt_renderer_denoised_device_ptr(_p(rn)) is None
    st = L.crt_selftest_denoise
    good = _lib.DenoiseOptions(5, 4.0, INF, 0.05, 0, 0)
    for args in ((None, _p(out), _p(out), C.byref(good), _p(out)), (_p(rn), None, _p(out), C.byref(good), _p(out)),
                 (_p(rn), _p(out), None, C.byref(good), _p(out)), (_p(rn), _p(out), _p(out), None, _p(out)),
                 (_p(rn), _p(out), _p(out), C.byref(good), None)):
        assert st(*args) == INVALID and "null" in _msg()
    for bad, word in ((_lib.DenoiseOptions(9, 4.0, INF, 0.05, 0, 0), "iterations"),
                      (_lib.DenoiseOptions(5, 0.0, INF, 0.05, 0, 0), "sigma_color"),
                      (_lib.DenoiseOptions(5, 4.0, INF, 0.05, 2, 0), "flag"),
                      (_lib.DenoiseOptions(5, 4.0, INF, 0.05, 0, 7), "reserved"),
                      (_lib.DenoiseOptions(5, 4.0, INF, 0.05, 1, 0), "tile scale")):
        assert st(_p(rn), _p(out), _p(out), C.byref(bad), _p(out)) == INVALID and word in _msg(), word
    assert not rn[4:].any() and not sc[4:].any()


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
    with pytest.raises(ValueError, match="Scene"):
        r.compute_guides(None)
    with pytest.raises(ValueError, match="different devices"):
        r.compute_guides(crt_amd.Scene(None, 1))
    with pytest.raises(ValueError, match="unknown trace option"):
        r.compute_guides(scene, count_work=True)
    for name in ("sigma_color", "sigma_normal", "sigma_position"):
        for bad in BAD_SIGMAS + (None, "x"):
            kw = dict(sigma_color=4.0, sigma_normal=INF, sigma_position=0.05)
            kw[name] = bad
            with pytest.raises(ValueError, match=name):
                r.denoise(scale=1.0, **kw)
            with pytest.raises(ValueError, match=name):
                r.selftest_denoise(np.zeros((8, 16, 3), F32), np.zeros((8, 16, 8), F32), **kw)
    with pytest.raises(TypeError):
        r.denoise(scale=1.0)                                  # no default sigmas
    for it in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="iterations"):
            r.denoise(4.0, INF, 0.05, iterations=it, scale=1.0)
    for scale in (None, NAN, 0.0, -1.0, "x"):
        with pytest.raises(ValueError, match="scale"):
            r.denoise(4.0, INF, 0.05, scale=scale)
    with pytest.raises(ValueError, match="exclude"):
        r.denoise(4.0, INF, 0.05, scale=1.0, tile_scale=True)
    with pytest.raises(ValueError, match="color"):
        r.selftest_denoise(np.zeros((8, 8, 3), F32), np.zeros((8, 16, 8), F32), 4.0, INF, 0.05)
    with pytest.raises(ValueError, match="guides"):
        r.selftest_denoise(np.zeros((8, 16, 3), F32), np.zeros((8, 16, 7), F32), 4.0, INF, 0.05)


# ------------------------------------------------------------------------------------------ the model, by hand
def _flat_guides(h, w, key=0):
    return dm.pack_guides(np.zeros((h, w, 3), F32), np.ones((h, w), F32), np.zeros((h, w, 3), F32),
                          np.full((h, w), key, np.int32))


H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])


def test_model_kernel_constants_are_exact():
    assert [float(v) for v in dm.H5] == H5.tolist() and float(sum(dm.H5)) == 1.0
    for a in H5:
        for b in H5:
            assert float(F32(a) * F32(b)) == a * b            # all 25 products are exact in float32


def test_model_impulse_with_all_sigmas_off():
    c = np.zeros((9, 9, 3), F32)
    c[4, 4] = 256
    g = _flat_guides(9, 9)
    out = dm.denoise(c, g, INF, INF, INF, 1)
    # the impulse's own 5x5 neighbourhood lies wholly inside, and every pixel of it has full weight or renormalises;
    # inside the 5x5 block round the centre pixel every tap set is complete: sw = 1
    want = np.zeros((9, 9), np.float64)
    want[2:7, 2:7] = 256 * np.outer(H5, H5)
    inner = (slice(2, 7), slice(2, 7))
    for ch in range(3):
        assert np.array_equal(out[inner][..., ch].astype(np.float64), want[inner])
    assert not out[0].any() and not out[:, 0].any() and not out[8].any() and not out[:, 8].any()
    # two iterations: the second has stride 2, so the centre row of the result is the stride-2 pattern of the first
    out2 = dm.denoise(c, g, INF, INF, INF, 2)
    first = dm.denoise(c, g, INF, INF, INF, 1)
    # pixel (4, 4): taps at offsets -4, -2, 0, 2, 4 all inside; sum of k * first at those places
    acc = F32(0)
    sw = F32(0)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            k = F32(dm.H5[dy + 2] * dm.H5[dx + 2])
            acc = F32(acc + F32(k * first[4 + 2 * dy, 4 + 2 * dx, 0]))
            sw = F32(sw + k)
    assert sw == 1 and out2[4, 4, 0] == F32(acc / sw)
    # by hand: first at even offsets from the centre is 256 * (1/16, 3/8, 1/16) x (1/16, 3/8, 1/16) on the taps -2, 0, 2
    # and 0 on -4, 4; weights there (1/4, 3/8, 1/4): (1/4 * 1/16 + 3/8 * 3/8 + 1/4 * 1/16)^2 * 256 = (11/64)^2 * 256
    assert float(out2[4, 4, 0]) == 256 * (11 / 64) ** 2
    # an odd offset from the centre sees only the odd taps of the first pass: (1/4 * 1/4 + 1/4 * 1/4) = 1/8 ... at
    # (4, 5): x taps 1, 3, 5, 7, 9 -> offsets -3, -1, 1, 3, (9 is outside): first = 256 h_y h_x with h_x = (0, 1/4, 1/4, 0)
    # weights (1/16, 1/4, 3/8, 1/4): x part = 1/4 * 1/4 + 3/8 * 1/4 = 5/32, renormalised by 15/16 (one tap outside)
    assert float(out2[4, 5, 0]) == float(F32(F32(256 * (11 / 64) * (5 / 32)) / F32(15 / 16)))


def test_model_corner_renormalises():
    c = np.full((9, 9, 3), 3.0, F32)
    c[0, 0] = 19.0
    g = _flat_guides(9, 9)
    out = dm.denoise(c, g, INF, INF, INF, 1)
    # the corner has the taps dy, dx in 0..2: weight (3/8 + 1/4 + 1/16)^2 = (11/16)^2
    sw = (11 / 16) ** 2
    acc = 3.0 * sw + (19.0 - 3.0) * (3 / 8) ** 2
    assert abs(float(out[0, 0, 0]) - acc / sw) < 1e-6
    ones = dm.denoise(np.ones((9, 9, 3), F32), g, INF, INF, INF, 1)
    assert (ones == 1).all()
    # the corner's sw in the model's own order of additions
    s = F32(0)
    for dy in range(0, 3):
        for dx in range(0, 3):
            s = F32(s + F32(dm.H5[dy + 2] * dm.H5[dx + 2]))
    assert float(s) == sw


@pytest.mark.parametrize("sig", [(INF, INF, INF), (4.0, INF, INF), (1.0, 0.5, 0.05)])
def test_model_constant_power_of_two_image_is_unchanged(sig):
    g = _flat_guides(19, 37)
    for v in (0.5, 2.0, 1024.0, -8.0, 0.0):
        c = np.full((19, 37, 3), v, F32)
        out = dm.denoise(c, g, *sig, 5)
        assert np.array_equal(out.view(np.uint32), c.view(np.uint32)) or (v == 0.0 and not out.any()), (v, sig)


def test_model_key_regions_do_not_leak():
    h, w = 12, 16
    c = np.zeros((h, w, 3), F32)
    c[:, 8:] = 64.0
    key = np.zeros((h, w), np.int32)
    key[:, 8:] = 1
    g = dm.pack_guides(np.zeros((h, w, 3), F32), np.ones((h, w), F32), np.zeros((h, w, 3), F32), key)
    out = dm.denoise(c, g, INF, INF, INF, 4)
    assert not out[:, :8].any() and (out[:, 8:] == 64).all()
    # one region: the edge smears
    g1 = _flat_guides(h, w)
    out = dm.denoise(c, g1, INF, INF, INF, 1)
    assert 0 < out[5, 7, 0] < 64 and 0 < out[5, 8, 0] < 64
    # miss pixels form a region of their own (key 0x7fffffff) and a negative key is a key like any other
    key[:, :8] = dm.MISS_KEY
    key[:, 8:] = -2
    g = dm.pack_guides(np.zeros((h, w, 3), F32), np.ones((h, w), F32), np.zeros((h, w, 3), F32), key)
    out = dm.denoise(c, g, INF, INF, INF, 3)
    assert not out[:, :8].any() and (out[:, 8:] == 64).all()


def test_model_a_term_that_is_off_ignores_an_infinite_difference():
    h, w = 7, 7
    c = np.full((h, w, 3), 2.0, F32)
    n = np.zeros((h, w, 3), F32)
    pos = np.zeros((h, w, 3), F32)
    n[3, 4] = [INF, 0, 0]                      # an infinite normal: dn = inf wherever it takes part
    pos[2, 2] = [0, -INF, 0]
    g = dm.pack_guides(n, np.ones((h, w), F32), pos, np.zeros((h, w), np.int32))
    off = dm.denoise(c, g, 4.0, INF, INF, 2)
    assert (off == 2).all()                    # both off: the guides never enter, 0 * inf is never formed
    c2 = c.copy()
    c2[3, 3] = 6.0
    base = dm.denoise(c2, _flat_guides(h, w), 4.0, INF, INF, 1)
    assert np.array_equal(dm.denoise(c2, g, 4.0, INF, INF, 1).view(np.uint32), base.view(np.uint32))
    # the normal term on: the tap (3, 4) is skipped by its neighbours (X = inf), and (3, 4) itself keeps only its centre
    on = dm.denoise(c2, g, 4.0, 1.0, INF, 1)
    assert np.isfinite(on).all() and on[3, 4, 0] == 2.0
    assert on[3, 3, 0] != base[3, 3, 0]


def test_model_nan_and_inf_neighbours_are_skipped_and_a_nan_centre_stays_alone():
    h, w = 9, 9
    g = _flat_guides(h, w)
    for bad in (NAN, INF, -INF):
        c = np.full((h, w, 3), 4.0, F32)
        c[4, 4, 1] = bad
        out = dm.denoise(c, g, 4.0, INF, INF, 1)
        others = np.ones((h, w), bool)
        others[4, 4] = False
        assert (out[others] == 4).all(), bad                 # the neighbour never spreads
        if bad != bad:
            assert np.isnan(out[4, 4, 1]) and out[4, 4, 0] == 4 and out[4, 4, 2] == 4
        else:
            assert out[4, 4, 1] == bad and out[4, 4, 0] == 4     # only its own centre tap is left: acc / sw = itself
        out5 = dm.denoise(c, g, 4.0, INF, INF, 5)
        assert (out5[others] == 4).all()


def test_exp_neg_edges():
    assert dm.exp_neg(F32(0)) == F32(1) and dm.exp_neg(F32(0)).view(np.uint32) == 0x3f800000
    below = np.nextafter(F32(80), F32(0))
    v = dm.exp_neg(below)
    assert np.isfinite(v) and v > 0 and abs(float(v) / np.exp(-float(below)) - 1) <= 2.0 ** -21
    # 80, +inf and NaN never reach exp_neg: the tap is skipped.  Two pixels whose colours differ by 1 (dc = 1), one
    # iteration with inv_c = X directly
    g = _flat_guides(1, 2)
    cc = np.zeros((1, 2, 3), F32)
    cc[0, 1, 0] = 1
    for d2, skipped in ((float(below), False), (80.0, True), (INF, True), (NAN, True)):
        out = dm.iteration(cc, g[..., 0:3], g[..., 4:7], g.view(np.int32)[..., 7], 1, F32(d2), None, None)
        if skipped:
            assert out[0, 0, 0] == 0 and out[0, 1, 0] == 1, d2
        else:
            assert 0 < out[0, 0, 0] < 1e-30 and out[0, 1, 0] == 1, d2


def test_exp_neg_relative_error():
    x = (np.arange(1_000_000, dtype=np.float64) * (80.0 / 1_000_000)).astype(F32)
    assert x[0] == 0 and x[-1] < 80
    got = dm.exp_neg(x).astype(np.float64)
    want = np.exp(-x.astype(np.float64))
    rel = np.abs(got / want - 1)
    assert rel.max() <= 2.0 ** -21, (rel.max(), x[rel.argmax()])


# ------------------------------------------------------------------------------------------ quality against the oracle
def test_the_filter_lowers_the_error_of_an_oracle_frame(oracle_scenes):
    import pyoracle
    w, h, spp = 64, 36, 16
    o = oracle_scenes["cornell_bunny"]
    cam = pyoracle.camera()
    gold = np.load(REPO / "tests" / "golden" / "cornell_bunny_64x36_16spp.npz")["sum"]
    raw = (gold * F32(1 / spp)).astype(F32)
    ro, rd = dm.centre_rays(cam, w, h)
    t, prim = o.trace(ro, rd)
    hit = t >= 0
    key = np.where(hit, prim[:, 0], dm.MISS_KEY).astype(np.int32)           # the mesh index, or -1 - sphere
    pos = (ro + (t[:, None] * rd).astype(F32)).astype(F32)
    pos[~hit] = 0
    guides = dm.pack_guides(np.zeros((h, w, 3), F32), t.reshape(h, w), pos.reshape(h, w, 3), key.reshape(h, w))
    ref, _, _ = o.render(cam, w, h, 512, 20, seed=1234)
    ref = ref.astype(np.float64) / 512
    out = dm.denoise(raw, guides, 4.0, INF, 0.05, 5)

    def rms(a):
        return float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))

    print(f"raw RMS {rms(raw):.4f}, filtered RMS {rms(out):.4f}")
    assert np.isfinite(out).all() and rms(out) < rms(raw)
