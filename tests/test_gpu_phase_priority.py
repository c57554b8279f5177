"""Phase priority of the frozen variant-8 kernels (profiles/phase_priority): a wave of
crt_render_kernel<false, 8, W> may traverse at one s_setprio level and run its regeneration passes at another.  Issue
priority decides when a wave's instructions run, never what a lane computes, so the frozen twin's frame must be the
bits of the open twin's (crt_render_open_kernel, which has no priority changes): fp32 sums, per-pixel RNG state, ray
and path counts.

Scene: cornell_bunny on the rebuilt 4-wide tree, 104x45 (13 x 6 = 78 tiles, the last row partial), 64 spp, 20 bounces,
seed 41.  The open twin renders when one schedule knob is off its default (wave_drain 32 instead of 64); the knob
changes when a draining wave passes, not its results (tests/test_gpu_tail_fill.py::test_the_open_twin).
"""
import numpy as np
import pytest

import crt_amd
from crt_amd import assets

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES, SEED = 104, 45, 64, 20, 41
N_TILES = 13 * 6


@pytest.fixture(scope="module")
def scene():
    return crt_amd.HostScene(assets.scene_files("cornell_bunny")).upload(0, bvh="rebuilt", width=4)


def _render(scene, setup=None, open_twin=False):
    """(sums, RNG state, counters, kernel name, frozen) of one frame; setup(r) moves knobs both twins honour."""
    r = crt_amd.Renderer(W, H)
    r.set_kernel_variant(8)
    if setup:
        setup(r)
    if open_twin:
        r.set_wave_drain(32)
    r.set_camera(crt_amd.camera(SPP))
    r.init_rand(SEED)
    r.render(scene, SPP, BOUNCES)
    r.synchronize()
    cnt = r.counters()
    name, frozen = r.last_kernel_name(), r.last_launch_frozen()
    r.resolve(crt_amd.pixel_sample_scale(SPP))
    r.synchronize()
    return r.linear(), r.rng_state(), cnt, name, frozen


def _same_bits(got, exp):
    lin, rng, cnt = got[:3]
    e_lin, e_rng, e_cnt = exp[:3]
    diff = np.argwhere(lin.view(np.uint32) != e_lin.view(np.uint32))
    assert len(diff) == 0, f"{len(diff)} fp32 words differ, first at {diff[:5].tolist()}"
    assert np.array_equal(rng, e_rng), "per-pixel RNG state differs"
    for key in ("rays", "paths"):
        assert cnt[key] == e_cnt[key], (key, cnt[key], e_cnt[key])
    assert cnt["rays"] > 0      # (a plain render counts rays only; paths are the counting kernel's, 0 == 0 here)


def _twins(scene, setup=None, kernel=None):
    frozen = _render(scene, setup)
    opened = _render(scene, setup, open_twin=True)
    assert frozen[4] == 1 and opened[4] == 0, (frozen[3:], opened[3:])
    assert frozen[3].startswith("crt_render_kernel<false, 8, "), frozen[3]
    if kernel:
        assert frozen[3] == kernel, frozen[3]
    _same_bits(frozen, opened)
    return frozen


def test_default_launch_equals_the_open_twin(scene):
    _twins(scene)


@pytest.mark.parametrize("occ", [4, 5, 6, 7])
def test_every_occupancy_target(scene, occ):
    _twins(scene, lambda r: r.set_occupancy_target(occ), kernel=f"crt_render_kernel<false, 8, {occ}>")


def test_tail_fill_forced_on(scene):
    """Heads and tail parts are frozen-twin blocks too: half the tiles hold back half their samples."""
    fills = []

    def setup(r):
        r.set_tail_fill(N_TILES // 2, SPP // 2)
        fills.append(r)

    _twins(scene, setup)
    for r in fills:      # both twins rendered with the fill on
        f = r.last_tail_fill()
        assert (f["tiles"], f["spp"]) == (N_TILES // 2, SPP // 2) and f["in_launch"] + f["swept"] == N_TILES // 2, f


@pytest.mark.parametrize("occ", [0, 6], ids=["automatic_occupancy", "occupancy_6"])
@pytest.mark.parametrize("tiles", [1000000, 0], ids=["every_tile_critical", "no_tile_critical"])
def test_critical_tiles(scene, tiles, occ):
    """Every tile regenerating at 5 parked lanes (each wave also drains below 5 live lanes), and none critical (a wave
    drains below the default threshold): the tests by which a wave may keep its traversal priority through a pass
    both run, in waves that also pass the ordinary way.  At the automatic occupancy, and at 6, whose kernel is one
    that holds those tests whatever the probe makes of this frame."""
    def setup(r):
        r.set_critical_tiles(tiles, 5)
        if occ:
            r.set_occupancy_target(occ)

    _twins(scene, setup, kernel=f"crt_render_kernel<false, 8, {occ}>" if occ else None)
