"""The regeneration pass after its blocks were merged: one Camera::getRay per next_ray call (bounce limit and roulette
ahead of it) and one unit() for every material of shade_rec.  Frames, RGBA8, RNG state and ray counts must stay what the
CPU oracle computes.

Scene: cornell_bunny_metal (Cornell box, glass bunny, the fuzzy-metal blocks, the light, the ground and metal spheres
and the sky), so an 8x8 frame is ONE wave that holds Lambert, glass, metal, light and sky lanes in the same pass.
Frames: that single 8x8 tile, and 20x12 (2x3 tiles of 8x8, the last column and row ragged).  Bounces: 20, and 1 and 3,
where the bounce limit and the first roulette bounce (bounce >= 3) end paths inside next_ray; 0, where a new sample
ends on the spot and only the retained outer loop of next_ray gets the lane out.

Bars: the reference-BVH kernel (variant 3) is bit-exact against the oracle in fp32 sums, RGBA8 bytes, the per-pixel
XORWOW state and the ray count.  The 4-wide kernels (variants 4, 7, 8 on the rebuilt tree) are bit-identical to each
other and meet the rebuilt-tree bar of tests/test_gpu_edge_paths.py against the oracle: per-channel RMS <= 1e-4 and
>= 99.9 % of the pixels bit-identical (at 64 and 240 pixels: every pixel).

crt_selftest_unit: the shared unit() in waves that mix ordinary vectors with vectors whose squared length lies outside
the fast square root's and the fast reciprocal's ranges; every lane must give the host's correctly rounded
(1 / sqrt(x*x + y*y + z*z)) * v, operation for operation in f32.
"""
import ctypes as C

import numpy as np
import pytest

import crt_amd
import objload
import pyoracle
from crt_amd import _lib, assets

pytestmark = pytest.mark.gpu
RMS_TOL = 1e-4
MIN_EQUAL = 0.999
SPP = 8
FRAMES = [(8, 8), (20, 12)]
BOUNCES = [20, 1, 3, 0]


@pytest.fixture(scope="module")
def mixed():
    files = assets.scene_files("cornell_bunny_metal")
    hs = crt_amd.HostScene(files)
    return {"ref": hs.upload(0), "fast": hs.upload(0, bvh="rebuilt", width=4), "hs": hs,
            "oracle": pyoracle.OracleScene(objload.load_scene(files)), "expected": {}}


def _oracle(mixed, w, h, bounces):
    """(sums, rgba8, final RNG state, rays) of the oracle for one frame; computed once per frame and bounce limit."""
    key = (w, h, bounces)
    if key not in mixed["expected"]:
        rng = np.stack([pyoracle.rng_init(41, i) for i in range(w * h)]).astype(np.uint32).reshape(h, w, 6)
        rng = np.ascontiguousarray(rng)
        cam = crt_amd.camera_floats(crt_amd.camera(SPP))
        s, rgba, cnt = mixed["oracle"].render_rng(cam, w, h, SPP, rng, bounces)
        mixed["expected"][key] = (s, rgba, rng, cnt["rays"])
    return mixed["expected"][key]


def _render(dev, w, h, bounces, variant, chunks=(SPP,)):
    r = crt_amd.Renderer(w, h)
    r.set_kernel_variant(variant)
    r.set_camera(crt_amd.camera(SPP))
    r.init_rand(41)
    rays = 0
    for k, spp in enumerate(chunks):
        r.render(dev, spp, bounces, accumulate=k > 0)
        r.synchronize()
        rays += r.counters()["rays"]
    r.resolve(crt_amd.pixel_sample_scale(SPP))
    r.synchronize()
    return r.linear(), r.rgba8(), r.rng_state(), rays


def _exact(got, exp):
    lin, rgba, rng, rays = got
    e_lin, e_rgba, e_rng, e_rays = exp
    diff = np.argwhere(lin.view(np.uint32) != e_lin.view(np.uint32))
    assert len(diff) == 0, f"{len(diff)} fp32 words differ, first at {diff[:5].tolist()}"
    assert np.array_equal(rgba, e_rgba)
    assert np.array_equal(rng, e_rng), "per-pixel RNG state differs"
    assert rays == e_rays, (rays, e_rays)


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("w,h", FRAMES)
def test_reference_bvh_bit_exact(mixed, w, h, bounces):
    _exact(_render(mixed["ref"], w, h, bounces, 3), _oracle(mixed, w, h, bounces))


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("w,h", FRAMES)
def test_wide_variants_identical_and_within_bar(mixed, w, h, bounces):
    e_lin, _, _, e_rays = _oracle(mixed, w, h, bounces)
    base = _render(mixed["fast"], w, h, bounces, 4)
    for variant in (7, 8):
        _exact(_render(mixed["fast"], w, h, bounces, variant), base)
    lin, rays = base[0], base[3]
    rms = np.sqrt(np.mean(((lin - e_lin) / SPP).astype(np.float64) ** 2, axis=(0, 1)))
    eq = float(np.mean(np.all(lin.view(np.uint32) == e_lin.view(np.uint32), axis=-1)))
    print(f"{w}x{h} {bounces} bounces: rms {rms}, bit-identical pixels {eq:.6f}, rays {rays} (oracle {e_rays})")
    assert (rms <= RMS_TOL).all(), f"per-channel RMS {rms}"
    assert eq >= MIN_EQUAL, f"only {eq:.6f} of pixels bit-identical"


@pytest.mark.parametrize("variant,tree", [(3, "ref"), (8, "fast")])
def test_chunked_accumulate_equals_single(mixed, variant, tree):
    """3 + 5 spp accumulated == 8 spp in one render (sums, RGBA8, RNG state, rays): a lane that comes back for the
    second chunk starts with a fresh sample, whatever ended its last path of the first."""
    w, h = FRAMES[1]
    one = _render(mixed[tree], w, h, 20, variant)
    _exact(_render(mixed[tree], w, h, 20, variant, chunks=(3, 5)), one)
    if variant == 3:
        _exact(one, _oracle(mixed, w, h, 20))


def _host_unit(v):
    """(1 / sqrt((x*x + y*y) + z*z)) * v in f32, every operation rounded once (numpy float32 arithmetic)."""
    v = v.astype(np.float32)
    with np.errstate(all="ignore"):
        l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        r = np.float32(1.0) / np.sqrt(l2)
        return (r[:, None] * v).astype(np.float32), l2


def test_shared_unit_known_answers():
    rng = np.random.default_rng(11)
    ordinary = rng.uniform(-1.0, 1.0, size=(64, 3))
    tiny = rng.uniform(0.5, 1.0, size=(64, 3)) * 1e-17    # len2 ~ 1e-34 < 2^-100; length < 1e-8
    huge = rng.uniform(2.5, 3.0, size=(64, 3)) * 1e19     # len2 overflows to +inf: 1 / inf = 0
    big = rng.uniform(0.5, 1.0, size=(64, 3)) * 1e19      # len2 ~ 1e38, finite: both fast ranges still hold
    lane = np.arange(64)[:, None]
    waves = [ordinary,                                      # every lane fast
             np.where(lane % 7 == 3, tiny, ordinary),       # a few tiny lanes: the whole wave takes the IEEE sequences
             np.where(lane % 5 == 1, huge, ordinary),       # a few overflowing lanes
             np.where(lane % 3 == 0, tiny, np.where(lane % 3 == 1, huge, ordinary)),
             np.where(lane == 63, tiny, big),
             tiny, huge]
    v = np.ascontiguousarray(np.concatenate(waves), np.float32)
    exp, l2 = _host_unit(v)
    assert (l2[64:128][np.arange(64) % 7 == 3] < 2.0 ** -100).all() and np.isinf(l2[128:192][np.arange(64) % 5 == 1]).all()
    assert np.isfinite(l2[256:319]).all() and (l2[256:319] > 1e37).all()
    out = np.zeros_like(v)
    crt_amd.check(_lib.hip().crt_selftest_unit(v.ctypes.data_as(C.c_void_p), len(v), out.ctypes.data_as(C.c_void_p)))
    bad = np.argwhere(out.view(np.uint32) != exp.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} words differ, first at {bad[:5].tolist()}: {out[bad[0][0]]} vs {exp[bad[0][0]]}"
