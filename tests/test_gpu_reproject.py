"""The reprojection on the GPU: Renderer.reproject, history, denoise_history, resolve_history and the
self-test.

Every comparison is bit for bit, on uint32 views (NaNs mapped to one pattern first: helpers/denoise_model.canon), against
helpers/reproject_model.py.

1. the kernel on crafted buffers against the numpy model.
2. sequences: render, compute_guides, reproject over a yaw sweep, each frame against the model fed the GPU's own sums and
   guides; what is not touched; reset; the filter and the resolve of the history; the error against a 512-spp frame.
3. the refusals that need a real handle.
4. the live-allocation count.
5. the checked build in a fresh child process.
6. the viewer: crth_viewer_set_reproject against the same calls by hand, and the crt_viewer command line.
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
from wavefront_batches import bits, same  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
CHECKED = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
VIEWER = REPO / "raytracer-cuda_amd" / "bin" / "crt_viewer"
F32 = np.float32
INF = float("inf")
INVALID, UNSUPPORTED = -1, -5
TOL, CAP = 0.05, 32.0
SIGMAS = (4.0, INF, 0.05)


# ------------------------------------------------------------------------------------------ 1. the kernel, crafted
# one lane; partial waves in x and y; an exact block; one past it in x and y; odd sizes; 64x36; a column of blocks; more
# than one block both ways with ragged edges
FRAMES = [(1, 1), (7, 5), (64, 4), (65, 5), (37, 19), (64, 36), (3, 70), (264, 260)]
# (position_tolerance, normal_min, max_history): the position term alone; both terms off and a cap of 1 (the history is
# replaced by the frame wherever it is found); both terms on and a cap that is no integer
OPTION_SETS = [(0.05, -INF, 32.0), (INF, -INF, 1.0), (0.02, 0.0, 8.5)]
# previous cameras: the same, moved sideways and forward, turned by 7 degrees, turned away (every point behind it), and
# turned by 75 degrees (in front, most of them off the frame)
PREVIOUS = {"equal": {}, "translated": {"pos": (0.04, -0.02, 0.33)}, "rotated": {"yaw": -83.0, "pitch": 3.0},
            "turned_away": {"yaw": 90.0}, "off_frame": {"yaw": -15.0}}


def _wall_guides(cam, w, h, g):
    """Guides of the wall z = -1 seen from `cam`: t solved per pixel-centre ray (so two cameras' positions describe the
    same surface; a ray that does not reach it is a miss), keys in world-space blocks over 4 values (one negative),
    random unit normals, a twentieth of the pixels misses, a twentieth of the positions pushed off the wall."""
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


def _crafted(w, h, seed, previous):
    g = np.random.default_rng(seed)
    aspect = max(w / h, 0.25)
    cam = crt_amd.camera(1, aspect=aspect)
    prev_cam = crt_amd.camera(1, aspect=aspect, **PREVIOUS[previous])
    c = (g.random((h, w, 3)) * 5 - 1).astype(F32)
    hist = np.concatenate([(g.random((h, w, 3)) * 5 - 1), g.integers(1, 40, (h, w, 1)) * g.choice([1.0, 0.75], (h, w, 1))],
                          axis=-1).astype(F32)
    for a in (c, hist[..., 0:3]):
        special = g.random((h, w)) < 0.03
        a[special, g.integers(0, 3, int(special.sum()))] = g.choice(np.array([np.inf, -np.inf, np.nan], F32), int(special.sum()))
    return c, _wall_guides(cam, w, h, g), _wall_guides(prev_cam, w, h, g), hist, prev_cam


@pytest.mark.parametrize("w,h", FRAMES)
def test_kernel_on_crafted_buffers_equals_the_model(w, h):
    r = crt_amd.Renderer(w, h)
    taken_by = {}
    for pi, previous in enumerate(PREVIOUS):
        c, guides, prev_guides, hist, prev_cam = _crafted(w, h, 2000 + 31 * w + h + 7 * pi, previous)
        pf = crt_amd.camera_floats(prev_cam)
        for opts in OPTION_SETS:
            want, taken = rm.reproject(c, guides, prev_guides, hist, pf, *opts)
            got = r.selftest_reproject(c, guides, prev_guides, hist, prev_cam, opts[0], opts[1], max_history=opts[2])
            diff = dm.canon(got) != dm.canon(want)
            assert not diff.any(), (w, h, previous, opts, int(diff.sum()), np.argwhere(diff)[:4].tolist())
            assert same(r.guides(), guides) and np.array_equal(dm.canon(r.linear()), dm.canon(c))
            assert np.array_equal(dm.canon(r.history()), dm.canon(got))
            assert (got[..., 3] <= F32(opts[2])).all() and (got[..., 3] >= 1).all()
            taken_by[previous, opts] = int(taken.sum())
        first = r.selftest_reproject(c, guides, prev_guides, None, prev_cam, TOL, max_history=CAP)
        assert np.array_equal(dm.canon(first[..., 0:3]), dm.canon(c)) and (bits(first[..., 3]) == 0x3f800000).all()
    assert not any(n for (previous, _), n in taken_by.items() if previous == "turned_away"), taken_by
    if w * h >= 500:                 # the cases have power: history is found, and each term rejects some of it
        for previous in ("equal", "translated", "rotated"):
            a, b, c3 = (taken_by[previous, o] for o in OPTION_SETS)
            assert b > a > c3 > 0, (previous, taken_by)
        assert taken_by["off_frame", OPTION_SETS[1]] < taken_by["rotated", OPTION_SETS[1]]


def test_a_second_call_on_the_first_calls_history():
    w, h = 37, 19
    r = crt_amd.Renderer(w, h)
    c, guides, prev_guides, hist, prev_cam = _crafted(w, h, 99, "translated")
    pf = crt_amd.camera_floats(prev_cam)
    first = r.selftest_reproject(c, guides, prev_guides, hist, prev_cam, TOL, max_history=CAP)
    second = r.selftest_reproject(c, prev_guides, guides, first, prev_cam, TOL, max_history=CAP)
    w1, _ = rm.reproject(c, guides, prev_guides, hist, pf, TOL, -INF, CAP)
    w2, _ = rm.reproject(c, prev_guides, guides, w1, pf, TOL, -INF, CAP)
    assert np.array_equal(dm.canon(first), dm.canon(w1)) and np.array_equal(dm.canon(second), dm.canon(w2))
    assert r.history_device_ptr() != 0


# ------------------------------------------------------------------------------------------ 2. sequences
@pytest.fixture(scope="module")
def bunny_w4(device_scenes):
    return device_scenes["cornell_bunny"][0].upload(0, bvh="rebuilt", width=4)


@pytest.fixture(scope="module")
def scene_of(device_scenes, bunny_w4):
    """The rebuilt 4-wide bunny scene and the reference-tree Cornell box."""
    return {"bunny_w4": bunny_w4, "cornell": device_scenes["cornell"][1]}


YAWS = [-92.5 + 0.5 * k for k in range(6)]


def _renderer(w, h, seed=41, cam=None):
    r = crt_amd.Renderer(w, h)
    r.set_camera(cam if cam is not None else crt_amd.camera(1))
    r.init_rand(seed)
    return r


def _state(r):
    r.synchronize()
    return {"sum": r.linear(), "rgba": r.rgba8(), "rng": r.rng_state(), "guides": r.guides()}


def _sweep(r, sc, yaws, model_history=None, prev=None, check=True, seeds=None):
    """render(1), compute_guides, reproject per camera; each frame's history against the model fed the GPU's own sums and
    guides.  Returns (the model's last history, (guides, camera floats) of the last frame, the last call's stats)."""
    stats = None
    for k, yaw in enumerate(yaws):
        cam = crt_amd.camera(1, yaw=yaw)
        r.set_camera(cam)
        if seeds is not None:
            r.init_rand(seeds[k])
        r.render(sc, 1, 20)
        r.resolve(1.0)
        r.compute_guides(sc)
        before = _state(r)
        stats = r.reproject(TOL, max_history=CAP, scale=1.0)
        after = _state(r)
        for k in before:
            assert same(before[k], after[k]), (yaw, k)       # sums, RGBA8, RNG state and guides are not touched
        g = before["guides"]
        want, taken = rm.reproject(rm.scaled(before["sum"], 1.0), g, None if prev is None else prev[0], model_history,
                                   None if prev is None else prev[1], TOL, -INF, CAP)
        if check:
            got = r.history()
            diff = dm.canon(got) != dm.canon(want)
            assert not diff.any(), (yaw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
            assert stats["pixels_reprojected"] == int(taken.sum())
            assert stats["pixels_hit"] == int((g[..., 3] >= 0).sum()) and stats["reproject_ms"] > 0
        model_history, prev = want, (g, crt_amd.camera_floats(cam))
    return model_history, prev, stats


@pytest.mark.parametrize("w,h", [(64, 36), (37, 19)])
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_yaw_sweep_equals_the_model_frame_by_frame(scene_of, name, w, h):
    sc = scene_of[name]
    r = _renderer(w, h)
    hist, prev, stats = _sweep(r, sc, YAWS)
    assert stats["pixels_reprojected"] >= 0.99 * stats["pixels_hit"] > 0
    assert len(YAWS) - 1 < hist[..., 3].max() <= len(YAWS) * (1 + 2.0 ** -20)
    # reset_history: the next frame starts over, and the sweep goes on from there
    r.reset_history()
    hist, prev, stats = _sweep(r, sc, YAWS[:1])
    assert stats["pixels_reprojected"] == 0 and (bits(r.history()[..., 3]) == 0x3f800000).all()
    _sweep(r, sc, YAWS[1:3], hist, prev)
    # a second renderer of another size starts over as well
    r2 = _renderer(w + 3, h + 2)
    _, _, stats = _sweep(r2, sc, YAWS[:2])
    assert stats["pixels_reprojected"] > 0


def test_uploaded_guides_have_no_camera_and_give_no_history(bunny_w4):
    """crt_selftest_denoise's upload becomes the current guides without a guide camera: the reprojection that takes them
    as its previous frame starts over instead of projecting into a camera they were not made from."""
    w, h = 37, 19
    r = _renderer(w, h)
    _sweep(r, bunny_w4, YAWS[:2], check=False)
    r.selftest_denoise(r.linear(), r.guides(), *SIGMAS, iterations=1)
    assert r.reproject(TOL, max_history=CAP, scale=1.0)["pixels_reprojected"] > 0      # previous: a real frame
    r.compute_guides(bunny_w4)
    s = r.reproject(TOL, max_history=CAP, scale=1.0)                                     # previous: the upload
    assert s["pixels_reprojected"] == 0 and (bits(r.history()[..., 3]) == 0x3f800000).all()
    r.compute_guides(bunny_w4)
    assert r.reproject(TOL, max_history=CAP, scale=1.0)["pixels_reprojected"] > 0


def test_filter_and_resolve_of_the_history(bunny_w4):
    w, h = 64, 36
    r = _renderer(w, h)
    _sweep(r, bunny_w4, YAWS[:4])
    before = _state(r)
    hist = r.history()
    stats = r.denoise_history(*SIGMAS)
    want = dm.denoise(hist[..., 0:3], before["guides"], *SIGMAS, 5)
    assert np.array_equal(dm.canon(r.denoised()), dm.canon(want)) and stats["iterations"] == 5 and stats["filter_ms"] > 0
    r.denoise_history(1.0, 0.5, 0.1, iterations=3, direct_only=True)
    assert np.array_equal(dm.canon(r.denoised()), dm.canon(dm.denoise(hist[..., 0:3], before["guides"], 1.0, 0.5, 0.1, 3)))
    assert np.array_equal(dm.canon(r.history()), dm.canon(hist))
    after = _state(r)
    for k in before:
        assert same(before[k], after[k]), k
    # the plain filter still takes the sums
    r.denoise(*SIGMAS, scale=1.0)
    assert np.array_equal(dm.canon(r.denoised()), dm.canon(dm.denoise(before["sum"], before["guides"], *SIGMAS, 5)))
    r.resolve_history()
    r.synchronize()
    r2 = crt_amd.Renderer(w, h)
    r2.write_linear(np.ascontiguousarray(hist[..., 0:3]))
    r2.resolve(1.0)
    r2.synchronize()
    assert np.array_equal(r.rgba8(), r2.rgba8()) and not np.array_equal(r.rgba8(), before["rgba"])
    assert same(r.linear(), before["sum"]) and same(r.rng_state(), before["rng"])


def _rms(a, ref):
    return float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))


@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_history_lowers_the_error_and_the_filter_lowers_it_again(scene_of, name):
    """The issue's set-up: 8 frames of 1 spp, seeds 41 .. 48, yaw -93.5 .. -90, against a 512-spp frame (seed 1234) of
    the last camera."""
    w, h = 64, 36
    sc = scene_of[name]
    ref = _renderer(w, h, seed=1234, cam=crt_amd.camera(1, yaw=-90.0))
    ref.render(sc, 512, 20)
    ref.synchronize()
    ref = ref.linear().astype(np.float64) / 512
    r = _renderer(w, h)
    _, _, stats = _sweep(r, sc, [-93.5 + 0.5 * k for k in range(8)], check=False, seeds=range(41, 49))
    raw, hist = r.linear(), r.history()[..., 0:3]
    r.denoise_history(4.0, INF, 0.05, iterations=4)          # the issue's a-trous (4, off, 0.05)
    filtered = r.denoised()
    figures = (_rms(raw, ref), _rms(hist, ref), _rms(filtered, ref))
    print(f"{name}: raw RMS {figures[0]:.4f}, history {figures[1]:.4f}, filtered history {figures[2]:.4f}, "
          f"reprojected {stats['pixels_reprojected']} / hit {stats['pixels_hit']}")
    assert figures[1] < figures[0] and figures[2] < figures[1]
    assert stats["pixels_reprojected"] >= 0.99 * stats["pixels_hit"]


# ------------------------------------------------------------------------------------------ 3. refusals on a real handle
def _no_history(r):
    assert r.history_device_ptr() == 0
    with pytest.raises(crt_amd.CrtError, match="no history"):
        r.history()
    with pytest.raises(crt_amd.CrtError, match="no history"):
        r.resolve_history()
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*no history"):
        r.denoise_history(*SIGMAS)


def live():
    gc.collect()
    buffers, nbytes = C.c_int64(-1), C.c_int64(-1)
    crt_amd.check(_lib.require("crt_debug_live_allocations")(C.byref(buffers), C.byref(nbytes)))
    return buffers.value, nbytes.value


def test_refusals_on_a_real_handle(bunny_w4):
    r = _renderer(64, 36)
    r.render(bunny_w4, 1, 20)
    before = live()
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*no guides"):
        r.reproject(TOL, max_history=CAP, scale=1.0)
    _no_history(r)
    r.reset_history()                                        # nothing to reset is no error
    assert live() == before
    r.compute_guides(bunny_w4)
    with_guides = live()
    r.set_pixel_shard(1, 2)
    with pytest.raises(crt_amd.CrtError, match=r"status -5.*pixel shard"):
        r.reproject(TOL, max_history=CAP, scale=1.0)
    r.set_pixel_shard(0, 1)
    fn = _lib.hip().crt_renderer_reproject
    for o, scale, word in ((_lib.ReprojectOptions(0.0, -INF, 32.0, 0, 0), 1.0, "position_tolerance"),
                           (_lib.ReprojectOptions(TOL, -2.0, 32.0, 0, 0), 1.0, "normal_min"),
                           (_lib.ReprojectOptions(TOL, -INF, 0.5, 0, 0), 1.0, "max_history"),
                           (_lib.ReprojectOptions(TOL, -INF, float("nan"), 0, 0), 1.0, "max_history"),
                           (_lib.ReprojectOptions(TOL, -INF, 32.0, 1, 0), 1.0, "flag"),
                           (_lib.ReprojectOptions(TOL, -INF, 32.0, 0, 3), 1.0, "reserved"),
                           (_lib.ReprojectOptions(TOL, -INF, 32.0, 0, 0), 0.0, "scale")):
        assert fn(r.h, C.byref(o), C.c_float(scale), None, None) == INVALID
        assert word in _lib.hip().crt_last_error().decode()
    _no_history(r)
    assert live() == with_guides                             # after a refusal nothing is allocated
    # the same handle then works, without a stats pointer too
    o = _lib.ReprojectOptions(TOL, -INF, 32.0, 0, 0)
    assert fn(r.h, C.byref(o), C.c_float(1.0), None, None) == 0
    r.synchronize()
    h = r.history()
    assert np.array_equal(dm.canon(h[..., 0:3]), dm.canon(r.linear())) and (h[..., 3] == 1).all()
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*tile scale"):
        o = _lib.DenoiseOptions(5, 4.0, INF, 0.05, 1, 0)
        crt_amd.check(_lib.hip().crt_renderer_denoise_history(r.h, C.byref(o), None, None), "denoise_history")


# ------------------------------------------------------------------------------------------ 4. the allocation count
def test_the_state_is_allocated_once_and_released_with_the_handle(bunny_w4):
    base = live()
    r = _renderer(37, 19)
    _sweep(r, bunny_w4, YAWS[:3], check=False)
    r.denoise_history(*SIGMAS, iterations=2)
    r.resolve_history()
    once = live()
    assert once[0] > base[0]
    r.reset_history()
    _sweep(r, bunny_w4, YAWS[:3], check=False)
    r.denoise_history(*SIGMAS, iterations=2)
    r.resolve_history()
    c, guides, prev_guides, hist, prev_cam = _crafted(37, 19, 5, "equal")
    r.selftest_reproject(c, guides, prev_guides, hist, prev_cam, TOL, max_history=CAP)
    assert live() == once
    r.close()
    assert live() == base


# ------------------------------------------------------------------------------------------ 5. the checked build
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
for yaw in (-92.0, -91.0, -90.0):
    r.set_camera(crt_amd.camera(1, yaw=yaw))
    r.render(sc, 1, 20)
    r.compute_guides(sc)
    stats = r.reproject(0.05, max_history=32.0, scale=1.0)
r.denoise_history(4.0, float("inf"), 0.05)
r.resolve_history()
r.synchronize()                                          # a device error of the checked build raises here
np.savez(sys.argv[2], flags=np.array(_lib.hip().crt_build_flags()), history=r.history(), denoised=r.denoised(),
         rgba=r.rgba8(), taken=np.array(stats["pixels_reprojected"]))
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
    _, _, stats = _sweep(r, bunny_w4, (-92.0, -91.0, -90.0), check=False)
    r.denoise_history(*SIGMAS)
    r.resolve_history()
    r.synchronize()
    assert np.array_equal(dm.canon(got["history"]), dm.canon(r.history()))
    assert np.array_equal(dm.canon(got["denoised"]), dm.canon(r.denoised()))
    assert np.array_equal(got["rgba"], r.rgba8()) and int(got["taken"]) == stats["pixels_reprojected"]


# ------------------------------------------------------------------------------------------ 6. the viewer
BENCH_POS = (0.0, 0.0, 0.3)
MOVE = [(0.016, {}), (0.016, {}), (0.05, {"keys": crt_amd.KEY_W}),
        (0.016, {"right_mouse": True, "mouse_x": 300.0, "mouse_y": 200.0}),
        (0.016, {"right_mouse": True, "mouse_x": 310.0, "mouse_y": 197.0}),
        (0.016, {"right_mouse": True, "mouse_x": 322.0, "mouse_y": 195.0}), (0.016, {}),
        (0.03, {"keys": crt_amd.KEY_D}), (0.016, {})]


@pytest.mark.parametrize("filtered", [False, True])
def test_viewer_reproject_mode_equals_the_calls_by_hand(scenes, device_scenes, filtered):
    w, h = 64, 36
    v = crt_amd.Viewer(scenes["cornell_bunny"], w, h, pos=BENCH_POS, focus=0.3, seed=41)
    v.set_reproject(TOL, max_history=CAP, denoise=SIGMAS if filtered else None, denoise_iterations=4)
    sc = device_scenes["cornell_bunny"][1]                   # the viewer's default tree is the reference's
    r = crt_amd.Renderer(w, h)
    r.init_rand(41)
    cams = []
    for k, (dt, inp) in enumerate(MOVE):
        info = v.frame(dt, **inp)
        cam = v.camera()
        cams.append(crt_amd.camera_floats(cam).tobytes())
        r.set_camera(cam)
        r.render(sc, info["spp"], 20)
        r.compute_guides(sc)
        stats = r.reproject(TOL, max_history=CAP, scale=cam.pixel_sample_scale)
        if filtered:
            r.denoise_history(*SIGMAS, iterations=4)
            r.resolve_denoised()
        else:
            r.resolve_history()
        r.synchronize()
        assert info["spp"] == 1 and same(v.renderer.linear(), r.linear()), k
        assert np.array_equal(dm.canon(v.renderer.history()), dm.canon(r.history())), k
        assert np.array_equal(v.renderer.rgba8(), r.rgba8()), k
        if filtered:
            assert np.array_equal(dm.canon(v.renderer.denoised()), dm.canon(r.denoised())), k
        assert (k == 0) == (stats["pixels_reprojected"] == 0)
    assert len(set(cams)) >= 5                               # the camera moved
    assert r.history()[..., 3].max() > 3
    # switched off: the frame is the plain one again, and the next time the mode starts over
    v.set_reproject(None)
    info = v.frame(0.016)
    r.set_camera(v.camera())
    r.render(sc, 1, 20)
    r.resolve(v.camera().pixel_sample_scale)
    r.synchronize()
    assert np.array_equal(v.renderer.rgba8(), r.rgba8())
    v.set_reproject(TOL, max_history=CAP)
    v.frame(0.016)
    assert (bits(v.renderer.history()[..., 3]) == 0x3f800000).all()
    v.close()
    acc = crt_amd.Viewer(scenes["cornell_bunny"], w, h, pos=BENCH_POS, focus=0.3, seed=41, accumulate=True)
    with pytest.raises(crt_amd.CrtError, match="exclude"):
        acc.set_reproject(TOL, max_history=CAP)
    acc.close()


PLAIN_KEYS = {"width", "height", "script", "bvh", "accumulate", "temporal", "drain", "frames", "fps", "frame_ms_mean",
              "frame_ms_p50", "frame_ms_p99", "kernel_ms_mean", "samples_per_pixel_total", "paths_per_s", "last_accumulated"}
MODE_KEYS = {"reproject", "guides_ms_mean", "reproject_ms_mean", "filter_ms_mean", "pixels_reprojected_last"}


def test_cli_reproject(scenes, tmp_path):
    base = [str(VIEWER), "-w", "64", "-h", "36", "-frames", "6", "-script", "orbit"]
    files = [str(f) for f in scenes["cornell_bunny"]]
    for extra, filtered in ((["-reproject", "0.05:-inf:32"], False),
                            (["-reproject", "0.05:-inf:32", "-denoise", "4:inf:0.05", "-denoise-iters", "4"], True)):
        out = tmp_path / ("filtered.ppm" if filtered else "history.ppm")
        p = subprocess.run(base + extra + ["-o", str(out)] + files, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        info = json.loads(p.stdout.strip().splitlines()[-1])
        assert set(info) == PLAIN_KEYS | MODE_KEYS
        assert info["reproject"] == "0.05:-inf:32" and info["guides_ms_mean"] > 0 and info["reproject_ms_mean"] > 0
        assert (info["filter_ms_mean"] > 0) == filtered and 0 < info["pixels_reprojected_last"] <= 64 * 36
        assert out.stat().st_size > 64 * 36 * 3
    p = subprocess.run(base + files, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert set(json.loads(p.stdout.strip().splitlines()[-1])) == PLAIN_KEYS
    for bad in (["-reproject", "0.05:32"], ["-denoise", "4:inf:0.05"], ["-reproject", "0.05:-inf:32", "-accumulate"],
                ["-reproject", "0.05:-inf:32", "-denoise-iters", "4"], ["-denoise-iters", "4"]):
        p = subprocess.run(base + bad + files, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and ("-reproject" in p.stderr or "-denoise" in p.stderr)
