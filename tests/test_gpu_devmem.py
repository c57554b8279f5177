"""The library releases what it allocates, counted by crt_debug_live_allocations: the buffers and bytes
csrc/crt_devmem.h's types hold in this process.  Other processes on the device do not move the count, and handles that
other tests of this process keep alive are part of every reading, so each test compares readings, never absolute values.

1. a handle's life: every feature that allocates on first use, once and then once more, then the handles destroyed.
2. every self-test entry leaves the count where it was.
3. a refused creation leaves nothing behind.

No test provokes a HIP failure: the error paths are leak-free by the types, and tests/test_devmem_cpu.py keeps the
allocating calls inside them.
"""
import ctypes as C
import gc
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import synth_scenes as synth  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 24, 16
SIGMAS = (4.0, 0.7, 0.5)
STACK_CAP = 16              # above CRT_STACK6 (12): the stream kernel's deeper entries go to the overflow region
INVALID = -1


def live():
    gc.collect()            # handles a finished test dropped are destroyed now, not in the middle of a comparison
    buffers, nbytes = C.c_int64(-1), C.c_int64(-1)
    crt_amd.check(_lib.require("crt_debug_live_allocations")(C.byref(buffers), C.byref(nbytes)))
    return buffers.value, nbytes.value


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def planar(tmp_path_factory):
    """The smallest synthetic family (125 triangles in two meshes) with the loader's standard sphere pair."""
    hs = crt_amd.HostScene(synth.planar(str(tmp_path_factory.mktemp("devmem"))))
    e = hs.export("rebuilt", width=4)
    assert e["width"] == 4 and e["n_ray_spheres"] == 2 and e["stack_bound"] < STACK_CAP
    return hs


def _rays(n):
    g = np.random.default_rng(5)
    d = g.normal(size=(n, 3)).astype(np.float32)
    d[:, 2] = -np.abs(d[:, 2]) - 0.5
    return crt_amd.pack_rays(np.tile(np.float32([0.0, 0.0, 0.3]), (n, 1)), d)


def test_a_handles_life_allocates_once_and_releases_everything(planar):
    import torch
    base = live()
    scene = planar.upload(0, bvh="rebuilt", width=4)
    deep = planar.upload(0, bvh="rebuilt", width=4, stack_cap=STACK_CAP)
    threaded = planar.upload(0)                      # the reference tree: variant 10's kind of scene
    r = crt_amd.Renderer(W, H)
    r.set_camera(crt_amd.camera(4))
    assert live()[0] > base[0]
    device_rays = torch.from_numpy(_rays(4096)).to("cuda:0")

    def every_step():
        after_trace = []
        r.init_rand(41)
        r.init_rand(41)                              # the same seed: the copy from the cache
        r.set_schedule(probe_spp=-1, min_spp=64)
        r.set_temporal_order(False)
        r.set_kernel_variant(4)
        r.render(scene, 4)
        r.set_kernel_variant(8)
        r.set_schedule(probe_spp=2, min_spp=0)       # with the cost probe
        r.render(scene, 4)
        r.set_schedule(probe_spp=0)
        r.set_kernel_variant(7)
        r.set_temporal_order(True)
        r.render(scene, 2)
        r.set_kernel_variant(10)
        r.render(threaded, 2)
        r.synchronize()
        assert r.last_kernel_name().startswith("crt_render_kernel<false, 10,")
        for n in (10, 3000):                         # the second query outgrows the first one's staging buffers
            assert len(scene.trace(_rays(n))["t"]) == n
            after_trace.append(live())
        deep.trace(device_rays, mode=2)              # the stream kernel, whose stack spills to the overflow region
        assert deep.trace_stats()["kernel_ms"] > 0
        r.set_kernel_variant(-1)
        r.set_temporal_order(False)
        assert r.render_wavefront(scene, 2)["rays"] >= W * H * 2
        assert r.render_adaptive(scene, 2, 8, 0.05)["samples"] >= W * H * 2
        r.compute_guides(scene)
        assert r.denoise(*SIGMAS, iterations=2, scale=0.5)["iterations"] == 2
        return after_trace

    small, large = every_step()
    assert large[0] == small[0] and large[1] > small[1], (small, large)
    once = live()
    again = every_step()
    assert again == [once, once] and live() == once, (once, again, live())
    r.close()
    for s in (scene, deep, threaded):
        s.close()
    assert live() == base


def _selftests(r):
    """name -> a call of that entry with its smallest valid input."""
    L = _lib.hip()
    one = np.ones(4, np.float32)
    out16, out64 = np.zeros(4, np.float32), np.zeros(2, np.float64)
    bad, first = C.c_ulonglong(0), C.c_uint32(0)
    lo = 0x3f800000
    cam = crt_amd.camera(1)
    rng = np.zeros(6, np.uint32)
    geometry_in = {0: 17, 1: 14, 2: 12, 3: 2, 4: 12}
    subs = np.zeros(1, np.uint64)
    n_pix, n_tiles = W * H, ((W + 7) // 8) * ((H + 7) // 8)
    calls = {
        "math": lambda: L.crt_selftest_math(_p(one), _p(one), 1, _p(out16), _p(out64)),
        "rcp": lambda: L.crt_selftest_rcp(lo, lo, C.byref(bad), C.byref(first)),
        "sqrt": lambda: L.crt_selftest_sqrt(lo, lo + (1 << 16) - 1, C.byref(bad), C.byref(first)),
        "unit": lambda: L.crt_selftest_unit(_p(np.ones(3, np.float32)), 1, _p(np.zeros(3, np.float32))),
        "scan": lambda: L.crt_selftest_scan(_p(np.ones(64, np.int32)), 1, _p(np.zeros(192, np.int32))),
        "rng": lambda: L.crt_selftest_rng(41, _p(subs), 1, 0, _p(np.zeros(6, np.uint32)), _p(np.zeros(1, np.float32))),
        "uv_div": lambda: L.crt_selftest_uv_div(1, C.byref(bad)),
        "tile_schedule": lambda: _lib.require("crt_selftest_tile_schedule")(
            r.h, _p(np.ones(n_pix, np.uint32)), 1, 2, 0, 1, 0, None),
        "pixel_order": lambda: _lib.require("crt_selftest_pixel_order")(r.h, 0, _p(np.ones(n_pix, np.uint32)), 0, 1),
        "adaptive_plan": lambda: _lib.require("crt_selftest_adaptive_plan")(
            r.h, _p(np.ones(n_pix * 3, np.float32)), _p(np.ones(n_pix * 3, np.float32)),
            _p(np.full(n_tiles, 2, np.int32)), 2, 4, C.c_float(0.0), _p(np.zeros(n_tiles, np.uint32)),
            C.byref(C.c_uint32(0))),
        "denoise": lambda: _lib.require("crt_selftest_denoise")(
            r.h, _p(np.ones(n_pix * 3, np.float32)), _p(np.ones(n_pix * 8, np.float32)),
            C.byref(crt_amd.Renderer._denoise_options("selftest denoise", *SIGMAS, 1, False, False)),
            _p(np.zeros(n_pix * 3, np.float32))),
        "shade": lambda: _lib.require("crt_selftest_shade")(_p(np.ones(32, np.float32)), 1, _p(np.zeros(20, np.float32))),
    }
    for kind, words in geometry_in.items():
        # kind 3 reads its two words as the pixel's integer coordinates: (0, 0)
        calls[f"geometry{kind}"] = lambda kind=kind, words=words: L.crt_selftest_geometry(
            kind, _p(np.full(words, 0.0 if kind == 3 else 1.0, np.float32)), 1, C.byref(cam), W, H, _p(rng),
            _p(np.zeros(6, np.float32)))
    return calls


SELFTESTS = ("math", "rcp", "sqrt", "unit", "scan", "geometry0", "geometry1", "geometry2", "geometry3", "geometry4", "rng",
             "uv_div", "tile_schedule", "pixel_order", "adaptive_plan", "denoise", "shade")


@pytest.fixture(scope="module")
def selftest_renderer():
    """A renderer whose on-first-use states exist already, so a self-test on it allocates nothing it keeps."""
    r = crt_amd.Renderer(W, H)
    calls = _selftests(r)
    for name in ("tile_schedule", "pixel_order", "adaptive_plan", "denoise"):
        crt_amd.check(calls[name](), name)
    yield r
    r.close()


@pytest.mark.parametrize("name", SELFTESTS)
def test_a_selftest_entry_leaves_the_count_where_it_was(selftest_renderer, name):
    call = _selftests(selftest_renderer)[name]
    before = live()
    crt_amd.check(call(), name)
    assert live() == before


def test_a_refused_creation_leaves_nothing_behind(planar):
    base = live()
    h = C.c_void_p()
    for w, hgt in ((0, H), (W, -1), (1 << 16, 1 << 16)):
        assert _lib.hip().crt_renderer_create(w, hgt, 0, C.byref(h)) == INVALID and not h.value
        assert b"bad renderer size" in _lib.hip().crt_last_error()
    assert live() == base
    d = planar.desc()
    for opts in (crt_amd.scene_options("rebuilt", width=3), crt_amd.scene_options("rebuilt", leaf_size=17)):
        assert _lib.hip().crt_scene_create_ex(C.byref(d), 0, C.byref(opts), C.byref(h)) == INVALID and not h.value
    assert live() == base
