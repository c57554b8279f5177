"""Tail fill of a variant-8 launch (crt_renderer_set_tail_fill): the heads of the first K tiles of the
cost order hold back their last delta samples, which follow the launch's tiles as small items (tail parts) and, where a
tail part finds its head unfinished, are rendered by a short sweep launch.

Every pixel stays on one lane and its samples stay in order on its one RNG stream, so fp32 sums, RGBA8, the per-pixel
XORWOW state and the ray and path counts must be the bits of the same render with the fill off, and
crt_renderer_last_tail_fill must account for every part: parts in the launch + parts swept == K.

Scene: cornell_bunny on the rebuilt 4-wide tree.  100x37 (13 x 5 = 65 tiles, ragged last row and column) at 64 spp:
all 130 blocks are resident at once, so the tail parts find their heads running and the sweep renders them.  1024x768
(12,288 tiles, more than the 7,168 wave slots) at 8 spp with K = 2,048: the tail parts are dispatched after most of
the launch's tiles ended, so parts also run inside the launch, a head and its tail part on different compute units.
"""
import numpy as np
import pytest

import crt_amd
from crt_amd import assets

pytestmark = pytest.mark.gpu
W, H, SPP = 100, 37, 64
N_TILES = 13 * 5
KS = {"one": 1, "half": N_TILES // 2, "all": N_TILES}
DELTAS = [1, 32, 63]


@pytest.fixture(scope="module")
def fast():
    return crt_amd.HostScene(assets.scene_files("cornell_bunny")).upload(0, bvh="rebuilt", width=4)


def _render(scene, fill, w=W, h=H, chunks=(SPP,), setup=None, count_work=False):
    """((sums, RGBA8, RNG state, counters summed over the chunks), last_tail_fill per chunk, frozen per chunk).
    fill: (tiles, spp) of set_tail_fill."""
    r = crt_amd.Renderer(w, h)
    r.set_kernel_variant(8)
    if setup:
        setup(r)
    r.set_tail_fill(*fill)
    r.set_camera(crt_amd.camera(sum(chunks)))
    r.init_rand(41)
    total, fills, frozen = {}, [], []
    for k, spp in enumerate(chunks):
        r.render(scene, spp, 20, accumulate=k > 0, count_work=count_work)
        r.synchronize()
        for key, v in r.counters().items():
            total[key] = total.get(key, 0) + v
        fills.append(r.last_tail_fill())
        frozen.append(r.last_launch_frozen())
    r.resolve(crt_amd.pixel_sample_scale(sum(chunks)))
    r.synchronize()
    return (r.linear(), r.rgba8(), r.rng_state(), total), fills, frozen


def _exact(got, exp, keys=("rays", "paths")):
    lin, rgba, rng, cnt = got
    e_lin, e_rgba, e_rng, e_cnt = exp
    diff = np.argwhere(lin.view(np.uint32) != e_lin.view(np.uint32))
    assert len(diff) == 0, f"{len(diff)} fp32 words differ, first at {diff[:5].tolist()}"
    assert np.array_equal(rgba, e_rgba)
    assert np.array_equal(rng, e_rng), "per-pixel RNG state differs"
    for key in keys:
        assert cnt[key] == e_cnt[key], (key, cnt[key], e_cnt[key])
    assert cnt["rays"] > 0


def _accounted(fill, k, delta):
    assert (fill["tiles"], fill["spp"]) == (k, delta), fill
    assert fill["in_launch"] >= 0 and fill["swept"] >= 0 and fill["in_launch"] + fill["swept"] == k, fill


OFF = {"tiles": 0, "spp": 0, "in_launch": 0, "swept": 0}


@pytest.fixture(scope="module")
def plain(fast):
    """The frame with the fill off (the default schedule: the probe on)."""
    got, fills, frozen = _render(fast, (0, 0))
    assert fills == [OFF] and frozen == [1]
    return got


def _no_probe(r):
    r.set_schedule(probe_spp=0)


@pytest.mark.parametrize("probe", [True, False])
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("k", list(KS))
def test_every_k_and_delta_gives_the_bits_of_the_plain_launch(fast, plain, k, delta, probe):
    got, fills, frozen = _render(fast, (KS[k], delta), setup=None if probe else _no_probe)
    assert frozen == [1]
    _accounted(fills[0], KS[k], delta)
    _exact(got, plain)          # the tile order changes when a tile runs, never what a lane computes


def test_k_beyond_the_tile_count_is_clamped(fast, plain):
    got, fills, _ = _render(fast, (10 * N_TILES, 32))
    _accounted(fills[0], N_TILES, 32)
    _exact(got, plain)


@pytest.mark.parametrize("delta", DELTAS)
def test_accumulate_over_two_renders(fast, delta):
    exp, fills, _ = _render(fast, (0, 0), chunks=(SPP, SPP))
    assert fills == [OFF, OFF]
    got, fills, _ = _render(fast, (KS["half"], delta), chunks=(SPP, SPP))
    for f in fills:             # the second render's heads continue the first render's sums, its tail parts the heads'
        _accounted(f, KS["half"], delta)
    _exact(got, exp)


@pytest.mark.parametrize("delta", DELTAS)
def test_the_open_twin(fast, plain, delta):
    got, fills, frozen = _render(fast, (KS["all"], delta), setup=lambda r: r.set_wave_drain(32))
    assert frozen == [0]
    _accounted(fills[0], KS["all"], delta)
    _exact(got, plain)


@pytest.mark.parametrize("occ", [4, 6, 7])
def test_forced_occupancies(fast, plain, occ):
    for delta in DELTAS:
        got, fills, frozen = _render(fast, (KS["half"], delta), setup=lambda r: r.set_occupancy_target(occ))
        assert frozen == [1]
        _accounted(fills[0], KS["half"], delta)
        _exact(got, plain)


@pytest.mark.parametrize("delta", [0, SPP, SPP + 1, -3])
def test_a_delta_outside_the_render_turns_the_fill_off(fast, plain, delta):
    got, fills, _ = _render(fast, (KS["half"], delta))
    assert fills == [OFF]
    _exact(got, plain)


def test_automatic_rule_leaves_a_small_frame_alone(fast, plain):
    got, fills, _ = _render(fast, (-1, 0))     # fewer than 4 tiles per wave slot: today's launch
    assert fills == [OFF]
    _exact(got, plain)


def test_a_counting_render_is_not_split(fast):
    keys = ("rays", "paths", "box_tests", "tri_tests", "sphere_tests")
    exp, fills, _ = _render(fast, (0, 0), count_work=True)
    assert fills == [OFF]
    assert all(k in exp[3] for k in keys), sorted(exp[3])
    got, fills, _ = _render(fast, (KS["all"], 32), count_work=True)
    assert fills == [OFF]
    _exact(got, exp, keys)
    assert got[3]["paths"] > 0


def test_parts_inside_the_launch_1024x768(fast):
    w, h, spp, k, delta = 1024, 768, 8, 2048, 4
    exp, fills, _ = _render(fast, (0, 0), w, h, chunks=(spp,))
    assert fills == [OFF]
    got, fills, _ = _render(fast, (k, delta), w, h, chunks=(spp,))
    _accounted(fills[0], k, delta)
    print(f"1024x768: {fills[0]['in_launch']} parts in the launch, {fills[0]['swept']} swept")
    # 12,288 + 2,048 one-wave blocks over at most 7,168 wave slots: a tail part is dispatched only after thousands of
    # blocks ended, so parts do run inside the launch (the release / acquire path between compute units)
    assert fills[0]["in_launch"] > 0
    _exact(got, exp)
