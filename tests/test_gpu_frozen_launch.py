"""The two twins of the plain variant-8 render kernels: the frozen one, in which the knobs of a default launch are
compile-time constants, and the open one, which reads them from the launch's arguments.

The library picks per launch (crt_renderer_last_launch_frozen says which ran); whichever runs, fp32 sums, RGBA8, the
per-pixel XORWOW state and the ray count must be the same bits.

Scene: cornell_bunny_metal on the rebuilt 4-wide tree, as tests/test_gpu_regen_pass.py: an 8x8 frame is ONE wave that
holds Lambert, glass, metal, light and sky lanes; 20x12 has a ragged last row and column.  8 spp; bounces 20, 1 and 0.
Its stack bound (13) exceeds the LDS entries of the occupancy-6 and -7 kernels (12, 8), so those launches use the
overflow region, and lies within the 16 of the occupancy-4 kernel.

Scenes outside the frozen shape come from tests/helpers/custom_scene.py: 1 and 3 spheres (the generic per-ray sphere
loop) and 9 spheres (spheres in the tree's leaves).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd
import objload
from crt_amd import assets

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import synth_scenes as synth  # noqa: E402
from custom_scene import CustomScene  # noqa: E402

pytestmark = pytest.mark.gpu
SPP = 8
FRAMES = [(8, 8), (20, 12)]
BOUNCES = [20, 1, 0]
STACK_ENTRIES = {4: 16, 6: 12, 7: 8}     # LDS stack entries of the kernels built for each occupancy target


@pytest.fixture(scope="module")
def fast():
    return crt_amd.HostScene(assets.scene_files("cornell_bunny_metal")).upload(0, bvh="rebuilt", width=4)


def _render(scene, w, h, bounces, variant=8, setup=None, chunks=(SPP,), count_work=False):
    """(sums, RGBA8, RNG state, rays), the kernel's name and whether each launch was frozen."""
    r = crt_amd.Renderer(w, h)
    r.set_kernel_variant(variant)
    if setup:
        setup(r)
    r.set_camera(crt_amd.camera(SPP))
    r.init_rand(41)
    rays, frozen = 0, []
    for k, spp in enumerate(chunks):
        r.render(scene, spp, bounces, accumulate=k > 0, count_work=count_work)
        r.synchronize()
        rays += r.counters()["rays"]
        frozen.append(r.last_launch_frozen())
    r.resolve(crt_amd.pixel_sample_scale(SPP))
    r.synchronize()
    return (r.linear(), r.rgba8(), r.rng_state(), rays), r.last_kernel_name(), frozen


def _exact(got, exp):
    lin, rgba, rng, rays = got
    e_lin, e_rgba, e_rng, e_rays = exp
    diff = np.argwhere(lin.view(np.uint32) != e_lin.view(np.uint32))
    assert len(diff) == 0, f"{len(diff)} fp32 words differ, first at {diff[:5].tolist()}"
    assert np.array_equal(rgba, e_rgba)
    assert np.array_equal(rng, e_rng), "per-pixel RNG state differs"
    assert rays == e_rays, (rays, e_rays)


# a knob set to its default value: still the frozen twin
DEFAULTS = {"regen_threshold_44": lambda r: r.set_regen_threshold(44), "wave_drain_48": lambda r: r.set_wave_drain(48),
            "top_levels_default": lambda r: r.set_top_levels(-1), "top_levels_1": lambda r: r.set_top_levels(1),
            "stack_lds_16": lambda r: r.set_stack_lds(16)}
# a knob moved off its default: the open twin (small frames run at occupancy 6: 12 LDS stack entries)
MOVED = {"regen_threshold_40": lambda r: r.set_regen_threshold(40), "wave_drain_64": lambda r: r.set_wave_drain(64),
         "top_levels_0": lambda r: r.set_top_levels(0), "stack_lds_8": lambda r: r.set_stack_lds(8)}


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("w,h", FRAMES)
def test_default_launch_is_frozen_and_every_knob_gives_the_same_bits(fast, w, h, bounces):
    base, name, frozen = _render(fast, w, h, bounces)
    assert name == "crt_render_kernel<false, 8, 6>" and frozen == [1]
    for key, setup in DEFAULTS.items():
        got, n, f = _render(fast, w, h, bounces, setup=setup)
        assert (n, f) == (name, [1]), key
        _exact(got, base)
    for key, setup in MOVED.items():
        got, n, f = _render(fast, w, h, bounces, setup=setup)
        assert (n, f) == (name, [0]), key
        # the thresholds change when a wave passes, never what a lane computes: one lane per pixel, samples in order
        _exact(got, base)


@pytest.mark.parametrize("occ", [4, 6, 7])
@pytest.mark.parametrize("w,h", FRAMES)
def test_occupancy_targets_keep_their_names_and_match_the_open_twin(fast, w, h, occ):
    for bounces in BOUNCES:
        frozen, name, f = _render(fast, w, h, bounces, setup=lambda r: r.set_occupancy_target(occ))
        assert name == f"crt_render_kernel<false, 8, {occ}>" and f == [1]

        def open_twin(r):
            r.set_occupancy_target(occ)
            r.set_stack_lds(STACK_ENTRIES[occ] - 4)     # fewer LDS entries than the kernel's: the open twin
        got, n, f = _render(fast, w, h, bounces, setup=open_twin)
        assert (n, f) == (name, [0])
        _exact(got, frozen)


@pytest.fixture(scope="module")
def sphere_worlds():
    one = assets.scene_files("cornell")
    floor = float(objload.load_scene(one).positions[:, 1].min())
    worlds = synth.sphere_worlds(floor)
    out = {}
    for key in ("s1", "s3", "s9_ground"):
        spheres, order, _ = worlds[key]
        cs = CustomScene(one, spheres, synth.SPHERE_MATS, order)
        out[key] = (cs, cs.upload(0, bvh="rebuilt", width=4), len(spheres))
    return out


@pytest.mark.parametrize("world", ["s1", "s3", "s9_ground"])
def test_scenes_outside_the_frozen_shape_run_the_open_twin(sphere_worlds, world):
    cs, scene, n = sphere_worlds[world]
    info = cs.export("rebuilt", width=4)
    assert info["n_ray_spheres"] != 2
    # up to eight spheres are all tested per ray; of the nine only the ground is, the others sit in the tree's leaves
    assert info["n_ray_spheres"] == (1 if world == "s9_ground" else n)
    for w, h in FRAMES:
        for bounces in BOUNCES:
            got, name, f = _render(scene, w, h, bounces)
            assert name == "crt_render_kernel<false, 8, 6>" and f == [0]
            _exact(got, _render(scene, w, h, bounces, variant=4)[0])


def test_chunked_accumulate_on_the_frozen_twin_equals_one_render(fast):
    w, h = FRAMES[1]
    one, _, f1 = _render(fast, w, h, 20)
    two, _, f2 = _render(fast, w, h, 20, chunks=(3, 5))
    assert f1 == [1] and f2 == [1, 1]
    _exact(two, one)


def test_counting_launch_is_not_frozen_and_counts_the_same_rays(fast):
    for w, h in FRAMES:
        plain, _, f = _render(fast, w, h, 20)
        counted, name, fc = _render(fast, w, h, 20, count_work=True)
        assert f == [1] and fc == [0] and name == "crt_render_kernel<true, 8, 6>"
        assert counted[3] == plain[3]
