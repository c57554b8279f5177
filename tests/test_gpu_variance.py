"""The variance-guided filtering of the history on the GPU: Renderer.reproject_moments, moments,
denoise_history_variance, variance and the two self-tests.

Every comparison is bit for bit, on uint32 views (NaNs mapped to one pattern first: helpers/denoise_model.canon), against
helpers/variance_model.py.

1. the estimate and the filter on crafted buffers: tiled against direct, both against the model.
2. reproject_moments on crafted buffers: its history against the plain entry's, its moments against the model.
3. a real sequence through the public calls; what is not touched; the old filter's bits on that history.
4. the refusals that need a real handle, and the validity rules.
5. the live-allocation count.
6. the checked build in a fresh child process.
7. the viewer and the crt_viewer command line.
"""
import ctypes as C
import gc
import json
import os
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
from wavefront_batches import same  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
CHECKED = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
VIEWER = REPO / "raytracer-cuda_amd" / "bin" / "crt_viewer"
F32 = np.float32
INF = float("inf")
INVALID, UNSUPPORTED = -1, -5
TOL, CAP = 0.05, 32.0
SIGMAS, MINH = (4.0, INF, 0.05), 4.0              # the paper's sigma_luminance and history length, §21's position sigma
OLD_SIGMAS = (4.0, INF, 0.05)


def _same(a, b):
    return np.array_equal(dm.canon(a), dm.canon(b))


def _where(a, b):
    diff = dm.canon(a) != dm.canon(b)
    return int(diff.sum()), np.argwhere(diff)[:4].tolist()


# ------------------------------------------------------------------------------------------ 1. estimate and filter, crafted
# one lane; partial waves; an exact block; one past it in x and y; odd sizes; 64x36; a column of blocks; 136 rows: the
# tiled kernel's second row group at stride 16; 260 rows: all five stride-32 taps inside the frame for the direct fallback
FRAMES = [(1, 1), (7, 5), (64, 4), (65, 5), (37, 19), (64, 36), (3, 70), (136, 136), (264, 260)]
# all three terms; each one alone
SIGMA_SETS = [(4.0, 0.5, 0.3), (4.0, INF, INF), (INF, 0.5, INF), (INF, INF, 0.3)]


def _crafted_filter(w, h, seed):
    """History rows, moments and guides: keys in blocks over 3 values with a twentieth of the pixels misses, random unit
    normals, positions on a noisy plane, lengths 1 .. 8 (below and above a min_history of 4) and some that are no
    integers, moments whose variance is positive, zero and (clamped) negative, and a few colours and moments that are
    NaN or infinite."""
    g = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    key = ((xs // 5 + ys // 4) % 3).astype(np.int32)
    n = g.normal(size=(h, w, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    pos = np.stack([xs / 16.0, ys / 16.0, g.random((h, w)) * 0.2], axis=-1).astype(F32)
    guides = dm.pack_guides(n, np.ones((h, w), F32), pos, key)
    guides[g.random((h, w)) < 0.05] = dm.miss_record()
    c = (g.random((h, w, 3)) * 2).astype(F32)
    c[ys > h // 2] *= F32(0.25)                                   # a luminance step inside the keys
    length = (g.integers(1, 9, (h, w)) * g.choice([1.0, 0.75, 1.5], (h, w))).astype(F32)
    length = np.maximum(length, F32(1))
    l = vm.lum(c)
    m1 = (l + (g.random((h, w)) - 0.5) * 0.2).astype(F32)
    m2 = (m1 * m1 + (g.random((h, w)) - 0.2) * 0.3 * g.choice([0.0, 1.0, 0.01], (h, w))).astype(F32)
    mom = np.stack([m1, m2], axis=-1).astype(F32)
    bad = np.array([np.inf, -np.inf, np.nan], F32)
    special = g.random((h, w)) < 0.02
    c[special, g.integers(0, 3, int(special.sum()))] = g.choice(bad, int(special.sum()))
    mom[special] = np.nan                                         # what lum of such a colour gives
    special = g.random((h, w)) < 0.01
    mom[special, 1] = np.inf                                      # an m2 that overflowed: v = +inf
    special = g.random((h, w)) < 0.01
    mom[special, g.integers(0, 2, int(special.sum()))] = g.choice(bad, int(special.sum()))
    hist = np.concatenate([c, length[..., None]], axis=-1).astype(F32)
    return hist, mom, guides


@pytest.mark.parametrize("w,h", FRAMES)
def test_estimate_and_filter_on_crafted_buffers_equal_the_model(w, h):
    r = crt_amd.Renderer(w, h)
    hist, mom, guides = _crafted_filter(w, h, 4000 + 17 * w + h)
    _, _, key = dm.split_guides(guides)
    v0 = vm.estimate(hist, mom, key, MINH)
    if w * h >= 500:                 # the cases have power: both branches, clamped and infinite variances, no NaN
        short = hist[..., 3] < MINH
        assert short.any() and (~short).any() and (v0 == 0).any() and np.isinf(v0).any() and (v0[short] > 0).any()
    assert not np.isnan(v0).any()
    for sig in SIGMA_SETS:
        want = vm.filter_steps(hist[..., 0:3], v0, guides, *sig, steps=(1, 2, 3, 4, 5, 6))
        for it in (1, 2, 3, 4, 5, 6):
            tiled, tv = r.selftest_denoise_variance(hist, mom, guides, *sig, min_history=MINH, iterations=it)
            direct, dv = r.selftest_denoise_variance(hist, mom, guides, *sig, min_history=MINH, iterations=it,
                                                     direct_only=True)
            assert _same(tiled, direct), (w, h, sig, it, _where(tiled, direct))
            assert _same(tiled, want[it][0]), (w, h, sig, it, _where(tiled, want[it][0]))
            assert _same(tv, v0) and _same(dv, v0), (w, h, sig, it, _where(tv, v0))
            assert _same(r.denoised(), tiled) and _same(r.variance(), v0)
        # a colour that is not finite never makes another pixel's so, with the luminance term on
        if sig[0] != INF:
            ok = np.isfinite(hist[..., 0:3]).all(axis=-1)
            assert np.isfinite(want[6][0][ok]).all() and np.isfinite(want[1][0][ok]).all()
    # another min_history moves pixels between the branches
    got, gv = r.selftest_denoise_variance(hist, mom, guides, *SIGMA_SETS[0], min_history=6.5, iterations=2)
    v1 = vm.estimate(hist, mom, key, 6.5)
    assert _same(gv, v1) and _same(got, vm.filter_steps(hist[..., 0:3], v1, guides, *SIGMA_SETS[0], steps=(2,))[2][0])
    with pytest.raises(crt_amd.CrtError, match="moments"):       # an upload is no reprojection: no valid moments to read
        r.moments()


# ------------------------------------------------------------------------------------------ 2. reproject_moments, crafted
REPROJECT_FRAMES = [(1, 1), (7, 5), (64, 4), (65, 5), (37, 19), (64, 36), (3, 70), (264, 260)]
OPTION_SETS = [(0.05, -INF, 32.0), (INF, -INF, 1.0), (0.02, 0.0, 8.5)]
# previous cameras: every tap-rejection reason test_gpu_reproject.py crafts
PREVIOUS = {"equal": {}, "translated": {"pos": (0.04, -0.02, 0.33)}, "rotated": {"yaw": -83.0, "pitch": 3.0},
            "turned_away": {"yaw": 90.0}, "off_frame": {"yaw": -15.0}}


def _wall_guides(cam, w, h, g):
    """Guides of the wall z = -1 seen from `cam`: keys in world-space blocks over 4 values, random unit normals, a
    twentieth of the pixels misses, a twentieth of the positions pushed off the wall."""
    o, d = dm.centre_rays(crt_amd.camera_floats(cam), w, h)
    with np.errstate(all="ignore"):
        t = ((F32(-1) - o[:, 2]) / d[:, 2]).astype(F32)
    t = np.where(np.isfinite(t) & (t > 0), t, F32(-1)).reshape(h, w)
    t = np.where(g.random((h, w)) < 0.05, F32(-1), t)
    t = np.where((g.random((h, w)) < 0.05) & (t > 0), (t * F32(1.3)).astype(F32), t)
    pos = (o + (t.reshape(-1, 1) * d).astype(F32)).astype(F32).reshape(h, w, 3)
    key = ((np.floor(pos[..., 0] * 3) + np.floor(pos[..., 1] * 5)) % 4).astype(np.int32) - 1
    n = g.normal(size=(h, w, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    hit = t >= 0
    guides = dm.pack_guides(n, t, np.where(hit[..., None], pos, F32(0)), np.where(hit, key, 0).astype(np.int32))
    guides[~hit] = dm.miss_record()
    return guides


def _crafted_reproject(w, h, seed, previous):
    g = np.random.default_rng(seed)
    aspect = max(w / h, 0.25)
    cam = crt_amd.camera(1, aspect=aspect)
    prev_cam = crt_amd.camera(1, aspect=aspect, **PREVIOUS[previous])
    c = (g.random((h, w, 3)) * 5 - 1).astype(F32)
    hist = np.concatenate([(g.random((h, w, 3)) * 5 - 1), g.integers(1, 40, (h, w, 1)) * g.choice([1.0, 0.75], (h, w, 1))],
                          axis=-1).astype(F32)
    bad = np.array([np.inf, -np.inf, np.nan], F32)
    for a in (c, hist[..., 0:3]):
        special = g.random((h, w)) < 0.03
        a[special, g.integers(0, 3, int(special.sum()))] = g.choice(bad, int(special.sum()))
    mom = (g.random((h, w, 2)) * 3).astype(F32)
    special = g.random((h, w)) < 0.03                             # moments that are not finite under finite colours
    mom[special, g.integers(0, 2, int(special.sum()))] = g.choice(bad, int(special.sum()))
    return c, _wall_guides(cam, w, h, g), _wall_guides(prev_cam, w, h, g), hist, mom, prev_cam


@pytest.mark.parametrize("w,h", REPROJECT_FRAMES)
def test_reproject_moments_on_crafted_buffers(w, h):
    r = crt_amd.Renderer(w, h)
    taken_by = {}
    for pi, previous in enumerate(PREVIOUS):
        c, guides, prev_guides, hist, mom, prev_cam = _crafted_reproject(w, h, 2000 + 31 * w + h + 7 * pi, previous)
        pf = crt_amd.camera_floats(prev_cam)
        for opts in OPTION_SETS:
            want_h, want_m, taken = vm.reproject_moments(c, guides, prev_guides, hist, mom, pf, *opts)
            plain = r.selftest_reproject(c, guides, prev_guides, hist, prev_cam, opts[0], opts[1], max_history=opts[2])
            got_h, got_m = r.selftest_reproject_moments(c, guides, prev_guides, hist, mom, prev_cam, opts[0], opts[1],
                                                        max_history=opts[2])
            assert _same(got_h, plain), (w, h, previous, opts, _where(got_h, plain))       # the plain entry's rows
            assert _same(got_h, want_h), (w, h, previous, opts, _where(got_h, want_h))
            assert _same(got_m, want_m), (w, h, previous, opts, _where(got_m, want_m))
            assert _same(r.history(), got_h) and _same(r.moments(), got_m)
            taken_by[previous, opts] = int(taken.sum())
        first_h, first_m = r.selftest_reproject_moments(c, guides, prev_guides, None, None, prev_cam, TOL, max_history=CAP)
        assert _same(first_h[..., 0:3], c) and (first_h[..., 3] == 1).all() and _same(first_m, vm.frame_moments(c))
    assert not any(n for (previous, _), n in taken_by.items() if previous == "turned_away"), taken_by
    if w * h >= 500:
        for previous in ("equal", "translated", "rotated"):
            a, b, c3 = (taken_by[previous, o] for o in OPTION_SETS)
            assert b > a > c3 > 0, (previous, taken_by)


@pytest.mark.parametrize("w,h", [(65, 5), (37, 19)])
def test_reproject_moments_history_is_the_plain_entrys_raw_bits(w, h):
    """Both kernels are one body (crt_reproject.h reproject_body): the history rows agree as raw uint32, the payload of
    every NaN included (the test above maps the NaNs to one pattern first)."""
    r = crt_amd.Renderer(w, h)
    nans = 0
    for pi, previous in enumerate(PREVIOUS):
        c, guides, prev_guides, hist, mom, prev_cam = _crafted_reproject(w, h, 2000 + 31 * w + h + 7 * pi, previous)
        for opts in OPTION_SETS:
            plain = r.selftest_reproject(c, guides, prev_guides, hist, prev_cam, opts[0], opts[1], max_history=opts[2])
            got_h = r.selftest_reproject_moments(c, guides, prev_guides, hist, mom, prev_cam, opts[0], opts[1],
                                                 max_history=opts[2])[0]
            diff = got_h.view(np.uint32) != plain.view(np.uint32)
            assert not diff.any(), (w, h, previous, opts, int(diff.sum()), np.argwhere(diff)[:4].tolist())
            nans += int(np.isnan(plain).sum())
    assert nans > 0                                                                    # there were NaNs to compare


# ------------------------------------------------------------------------------------------ 3. a real sequence
@pytest.fixture(scope="module")
def bunny_w4(device_scenes):
    return device_scenes["cornell_bunny"][0].upload(0, bvh="rebuilt", width=4)


YAWS = [-47.0, -46.0, -45.0, -44.0]              # the open front of the box is in view: misses beside hits


def _renderer(w, h, seed=41, cam=None):
    r = crt_amd.Renderer(w, h)
    r.set_camera(cam if cam is not None else crt_amd.camera(1))
    r.init_rand(seed)
    return r


def _state(r):
    r.synchronize()
    return {"sum": r.linear(), "rgba": r.rgba8(), "rng": r.rng_state(), "guides": r.guides()}


def _frame(r, sc, yaw):
    cam = crt_amd.camera(1, yaw=yaw)
    r.set_camera(cam)
    r.render(sc, 1, 20)
    r.resolve(1.0)
    r.compute_guides(sc)
    return cam


@pytest.mark.parametrize("w,h", [(64, 36), (37, 19)])
def test_sequence_through_the_public_calls_equals_the_model(bunny_w4, w, h):
    r = _renderer(w, h)
    model = vm.HistoryState()
    for k, yaw in enumerate(YAWS):
        cam = _frame(r, bunny_w4, yaw)
        before = _state(r)
        g = before["guides"]
        assert 0 < int((g[..., 3] < 0).sum()) < w * h                                  # misses and hits
        stats = r.reproject_moments(TOL, max_history=CAP, scale=1.0)
        taken = model.reproject_moments(rm.scaled(before["sum"], 1.0), g, crt_amd.camera_floats(cam), TOL, -INF, CAP)
        hist, mom = r.history(), r.moments()
        assert _same(hist, model.history), (yaw, _where(hist, model.history))
        assert _same(mom, model.moments), (yaw, _where(mom, model.moments))
        assert stats["pixels_reprojected"] == int(taken.sum()) and (k == 0) == (stats["pixels_reprojected"] == 0)
        assert stats["pixels_hit"] == int((g[..., 3] >= 0).sum()) and stats["reproject_ms"] > 0
        fs = r.denoise_history_variance(*SIGMAS, min_history=MINH)
        want, v0 = vm.denoise_variance(hist, mom, g, *SIGMAS, MINH, 5)
        assert _same(r.variance(), v0), (yaw, _where(r.variance(), v0))
        assert _same(r.denoised(), want), (yaw, _where(r.denoised(), want))
        assert fs["iterations"] == 5 and fs["filter_ms"] > 0 and fs["pixels_hit"] == stats["pixels_hit"]
        ms = r.denoise_iteration_ms()
        assert ms["input_ms"] > 0 and len(ms["iteration_ms"]) == 5                     # slot 0: the estimate kernel
        after = _state(r)
        for name in before:
            assert same(before[name], after[name]), (yaw, name)    # sums, RGBA8, RNG state and guides are not touched
        assert _same(r.history(), hist) and _same(r.moments(), mom)
    assert (v0 > 0).any()
    # the direct kernels and other options give the model's bits as well
    r.denoise_history_variance(2.0, 0.5, INF, min_history=2.0, iterations=3, direct_only=True)
    assert _same(r.denoised(), vm.denoise_variance(hist, mom, g, 2.0, 0.5, INF, 2.0, 3)[0])
    # the old filter still gives its old bits on that history, and resolve_denoised serves the new one
    r.denoise_history(*OLD_SIGMAS)
    assert _same(r.denoised(), dm.denoise(hist[..., 0:3], g, *OLD_SIGMAS, 5))
    r.denoise_history_variance(*SIGMAS, min_history=MINH)
    r.resolve_denoised()
    r.synchronize()
    r2 = crt_amd.Renderer(w, h)
    r2.write_linear(np.ascontiguousarray(want))
    r2.resolve(1.0)
    r2.synchronize()
    assert np.array_equal(r.rgba8(), r2.rgba8()) and r.denoised_device_ptr() != 0
    assert same(r.linear(), before["sum"]) and same(r.rng_state(), before["rng"])


# ------------------------------------------------------------------------------------------ 4. refusals, validity
def live():
    gc.collect()
    buffers, nbytes = C.c_int64(-1), C.c_int64(-1)
    crt_amd.check(_lib.require("crt_debug_live_allocations")(C.byref(buffers), C.byref(nbytes)))
    return buffers.value, nbytes.value


def test_refusals_and_validity_on_a_real_handle(bunny_w4):
    w, h = 64, 36
    r = _renderer(w, h)
    r.render(bunny_w4, 1, 20)
    before = live()
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*no guides"):
        r.reproject_moments(TOL, max_history=CAP, scale=1.0)
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*no history.*crt_renderer_reproject_moments"):
        r.denoise_history_variance(*SIGMAS, min_history=MINH)
    with pytest.raises(crt_amd.CrtError, match="moments"):
        r.moments()
    with pytest.raises(crt_amd.CrtError, match="no variance"):
        r.variance()
    assert live() == before                                  # a refusal allocates nothing
    # a plain reprojection: a history, and no moments
    cam = _frame(r, bunny_w4, YAWS[0])
    r.reproject(TOL, max_history=CAP, scale=1.0)
    plain = live()
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*no valid moments.*crt_renderer_reproject_moments"):
        r.denoise_history_variance(*SIGMAS, min_history=MINH)
    with pytest.raises(crt_amd.CrtError, match="moments"):
        r.moments()
    r.set_pixel_shard(1, 2)
    with pytest.raises(crt_amd.CrtError, match=r"status -5.*pixel shard"):
        r.reproject_moments(TOL, max_history=CAP, scale=1.0)
    with pytest.raises(crt_amd.CrtError, match=r"status -5.*pixel shard"):
        r.denoise_history_variance(*SIGMAS, min_history=MINH)
    r.set_pixel_shard(0, 1)
    fn = _lib.hip().crt_renderer_denoise_history_variance
    for o, word in ((_lib.DenoiseVarianceOptions(9, 4.0, INF, 0.05, 4.0, 0, 0), "iterations"),
                    (_lib.DenoiseVarianceOptions(5, 0.0, INF, 0.05, 4.0, 0, 0), "sigma_luminance"),
                    (_lib.DenoiseVarianceOptions(5, 4.0, INF, 0.05, 0.0, 0, 0), "min_history"),
                    (_lib.DenoiseVarianceOptions(5, 4.0, INF, 0.05, 4.0, 2, 0), "flag"),
                    (_lib.DenoiseVarianceOptions(5, 4.0, INF, 0.05, 4.0, 0, 1), "reserved")):
        assert fn(r.h, C.byref(o), None, None) == INVALID and word in _lib.hip().crt_last_error().decode()
    assert live() == plain                                   # the user of the plain entry has paid nothing
    # the validity rules against the model: moments after a plain call start the whole history over
    model = vm.HistoryState()
    model.reproject(rm.scaled(r.linear(), 1.0), r.guides(), crt_amd.camera_floats(cam), TOL, -INF, CAP)
    assert _same(r.history(), model.history)
    for step, yaw in enumerate(YAWS[1:]):
        cam = _frame(r, bunny_w4, yaw)
        c, g, cf = rm.scaled(r.linear(), 1.0), r.guides(), crt_amd.camera_floats(cam)
        if step == 1:                                        # a plain call in between ends the moments again
            s = r.reproject(TOL, max_history=CAP, scale=1.0)
            model.reproject(c, g, cf, TOL, -INF, CAP)
            assert s["pixels_reprojected"] > 0 and _same(r.history(), model.history)
            with pytest.raises(crt_amd.CrtError, match="no valid moments"):
                r.denoise_history_variance(*SIGMAS, min_history=MINH)
            continue
        s = r.reproject_moments(TOL, max_history=CAP, scale=1.0)
        taken = model.reproject_moments(c, g, cf, TOL, -INF, CAP)
        assert s["pixels_reprojected"] == int(taken.sum()) == 0          # both times the history had no moments
        assert _same(r.history(), model.history) and _same(r.moments(), model.moments)
        assert (r.history()[..., 3] == 1).all()
    # without a stats pointer the filter runs as well
    o = _lib.DenoiseVarianceOptions(0, 4.0, INF, 0.05, 4.0, 0, 0)          # iterations 0 = 5
    assert fn(r.h, C.byref(o), None, None) == 0
    r.synchronize()
    assert _same(r.denoised(), vm.denoise_variance(r.history(), r.moments(), r.guides(), *SIGMAS, MINH, 5)[0])
    # reset_history ends the moments too
    r.reset_history()
    with pytest.raises(crt_amd.CrtError, match="no valid moments"):
        r.denoise_history_variance(*SIGMAS, min_history=MINH)


# ------------------------------------------------------------------------------------------ 5. the allocation count
def test_the_state_is_allocated_once_and_released_with_the_handle(bunny_w4):
    base = live()
    w, h = 37, 19
    r = _renderer(w, h)
    for yaw in YAWS[:2]:
        _frame(r, bunny_w4, yaw)
        r.reproject_moments(TOL, max_history=CAP, scale=1.0)
    with_moments = live()
    r.denoise_history_variance(*SIGMAS, min_history=MINH, iterations=2)
    once = live()
    assert once[0] == with_moments[0] + 1 and once[1] == with_moments[1] + w * h * 4      # the variance buffer
    for yaw in YAWS[2:]:
        _frame(r, bunny_w4, yaw)
        r.reproject_moments(TOL, max_history=CAP, scale=1.0)
        r.denoise_history_variance(*SIGMAS, min_history=MINH)
    hist, mom, guides = _crafted_filter(w, h, 5)
    r.selftest_denoise_variance(hist, mom, guides, *SIGMAS, min_history=MINH)
    assert live() == once
    r.close()
    assert live() == base


# ------------------------------------------------------------------------------------------ 6. the checked build
CHILD = r"""
import sys
from pathlib import Path
import numpy as np
repo = Path(sys.argv[1])
sys.path[:0] = [str(repo / "raytracer-cuda_amd"), str(repo / "oracle")]
import crt_amd
from crt_amd import _lib, assets
hs = crt_amd.HostScene(assets.scene_files("cornell_bunny"))
sc = hs.upload(0, bvh="rebuilt", width=4)
r = crt_amd.Renderer(64, 36)
r.init_rand(41)
for yaw in (-47.0, -46.0, -45.0):
    r.set_camera(crt_amd.camera(1, yaw=yaw))
    r.render(sc, 1, 20)
    r.compute_guides(sc)
    stats = r.reproject_moments(0.05, max_history=32.0, scale=1.0)
r.denoise_history_variance(4.0, float("inf"), 0.05, min_history=4.0)
r.resolve_denoised()
r.synchronize()                                          # a device error of the checked build raises here
np.savez(sys.argv[2], flags=np.array(_lib.hip().crt_build_flags()), history=r.history(), moments=r.moments(),
         variance=r.variance(), denoised=r.denoised(), rgba=r.rgba8(), taken=np.array(stats["pixels_reprojected"]))
"""


def test_checked_build_gives_the_same_bits(bunny_w4, tmp_path):
    assert CHECKED.exists() and _lib.hip().crt_build_flags() == 0
    out = tmp_path / "checked.npz"
    p = subprocess.run([sys.executable, "-c", CHILD, str(REPO), str(out)],
                       env=dict(os.environ, CRT_HIP_LIB=str(CHECKED)), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(out)
    assert int(got["flags"]) == _lib.BUILD_CHECKED
    r = _renderer(64, 36)
    for yaw in (-47.0, -46.0, -45.0):
        _frame(r, bunny_w4, yaw)
        stats = r.reproject_moments(TOL, max_history=CAP, scale=1.0)
    r.denoise_history_variance(*SIGMAS, min_history=MINH)
    r.resolve_denoised()
    r.synchronize()
    for name, mine in (("history", r.history()), ("moments", r.moments()), ("variance", r.variance()),
                       ("denoised", r.denoised())):
        assert _same(got[name], mine), name
    assert np.array_equal(got["rgba"], r.rgba8()) and int(got["taken"]) == stats["pixels_reprojected"]


# ------------------------------------------------------------------------------------------ 7. the viewer
BENCH_POS = (0.0, 0.0, 0.3)
MOVE = [(0.016, {}), (0.016, {}), (0.05, {"keys": crt_amd.KEY_W}),
        (0.016, {"right_mouse": True, "mouse_x": 300.0, "mouse_y": 200.0}),
        (0.016, {"right_mouse": True, "mouse_x": 310.0, "mouse_y": 197.0}), (0.016, {}),
        (0.03, {"keys": crt_amd.KEY_D}), (0.016, {})]


def test_viewer_variance_mode_equals_the_calls_by_hand(scenes, device_scenes):
    w, h = 64, 36
    v = crt_amd.Viewer(scenes["cornell_bunny"], w, h, pos=BENCH_POS, focus=0.3, seed=41)
    with pytest.raises(crt_amd.CrtError, match="needs the reproject mode"):
        v.set_denoise_variance(*SIGMAS, min_history=MINH)
    v.set_reproject(TOL, max_history=CAP, denoise=OLD_SIGMAS)
    with pytest.raises(crt_amd.CrtError, match="exclude each other"):
        v.set_denoise_variance(*SIGMAS, min_history=MINH)
    v.set_reproject(TOL, max_history=CAP)
    v.set_denoise_variance(*SIGMAS, min_history=MINH, iterations=4)
    sc = device_scenes["cornell_bunny"][1]                   # the viewer's default tree is the reference's
    r = crt_amd.Renderer(w, h)
    r.init_rand(41)
    for k, (dt, inp) in enumerate(MOVE):
        info = v.frame(dt, **inp)
        cam = v.camera()
        r.set_camera(cam)
        r.render(sc, info["spp"], 20)
        r.compute_guides(sc)
        stats = r.reproject_moments(TOL, max_history=CAP, scale=cam.pixel_sample_scale)
        r.denoise_history_variance(*SIGMAS, min_history=MINH, iterations=4)
        r.resolve_denoised()
        r.synchronize()
        assert info["spp"] == 1 and same(v.renderer.linear(), r.linear()), k
        assert _same(v.renderer.history(), r.history()) and _same(v.renderer.moments(), r.moments()), k
        assert _same(v.renderer.variance(), r.variance()) and _same(v.renderer.denoised(), r.denoised()), k
        assert np.array_equal(v.renderer.rgba8(), r.rgba8()), k
        assert (k == 0) == (stats["pixels_reprojected"] == 0)
    assert r.history()[..., 3].max() > 3
    # switched off: the reproject mode alone again; its plain call ends the moments
    v.set_denoise_variance(None)
    v.frame(0.016)
    with pytest.raises(crt_amd.CrtError, match="moments"):
        v.renderer.moments()
    v.close()


PLAIN_KEYS = {"width", "height", "script", "bvh", "accumulate", "temporal", "drain", "frames", "fps", "frame_ms_mean",
              "frame_ms_p50", "frame_ms_p99", "kernel_ms_mean", "samples_per_pixel_total", "paths_per_s", "last_accumulated"}
MODE_KEYS = {"reproject", "guides_ms_mean", "reproject_ms_mean", "filter_ms_mean", "pixels_reprojected_last",
             "denoise_variance"}


def test_cli_denoise_variance_writes_the_python_chains_frame(scenes, device_scenes, tmp_path):
    w, h, frames = 64, 36, 4
    files = [str(f) for f in scenes["cornell_bunny"]]
    out = tmp_path / "variance.ppm"
    p = subprocess.run([str(VIEWER), "-w", str(w), "-h", str(h), "-frames", str(frames), "-script", "still", "-seed", "41",
                        "-reproject", "0.05:-inf:32", "-denoise-variance", "4:inf:0.05:4", "-denoise-iters", "4",
                        "-o", str(out)] + files, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(info) == PLAIN_KEYS | MODE_KEYS and info["denoise_variance"] == "4:inf:0.05:4"
    assert info["filter_ms_mean"] > 0 and info["reproject_ms_mean"] > 0 and 0 < info["pixels_reprojected_last"] <= w * h
    # the same frames by hand: the camera of a viewer at the same pose, standing still
    v = crt_amd.Viewer(scenes["cornell_bunny"], w, h, pos=BENCH_POS, focus=0.3, seed=41)
    v.frame(1.0 / 60.0)
    cam = v.camera()
    v.close()
    sc = device_scenes["cornell_bunny"][1]
    r = crt_amd.Renderer(w, h)
    r.init_rand(41)
    r.set_camera(cam)
    for _ in range(frames):
        r.render(sc, 1, 20)
        r.compute_guides(sc)
        r.reproject_moments(TOL, max_history=CAP, scale=cam.pixel_sample_scale)
        r.denoise_history_variance(*SIGMAS, min_history=MINH, iterations=4)
        r.resolve_denoised()
    r.synchronize()
    assert out.read_bytes() == crt_amd.encode_image(r.rgba8(), "ppm", flip=True)
