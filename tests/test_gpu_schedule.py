"""The tile and pixel schedules of variants 7, 8 and 10, stage by stage, against tests/helpers/schedule_model.py.

The renders' own tests only show that no order loses or repeats a pixel ("results never depend on the order").  Here
the stages between the cost probe and the main kernel run on crafted costs through the library's schedule self-tests
(crt_selftest_tile_schedule, crt_selftest_pixel_order: the host functions the renders call, in the renderer's own
buffers) and are held against the model, which states what is determined -- keys, statistics, a descending
permutation, the (strip, key) pair of every XCD slot, the slot expansion -- and what is free (the order of equal
clamped keys: the sort's ranks come from atomics).  Nothing here compares the library with itself.

The order buffer is filled with 0xffffffff before every stage, so an entry written past a stage's range shows.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import schedule_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu
EMPTY = sm.EMPTY
_renderers = {}


def _renderer(w, h):
    """One renderer per frame size for the whole module (no camera, no scene: the stages need neither)."""
    if (w, h) not in _renderers:
        _renderers[w, h] = crt_amd.Renderer(w, h)
    return _renderers[w, h]


def _rng(*key):
    return np.random.default_rng([41, *key])


def _layouts(w, h, *key):
    """The cost layouts every size gets: many ties, wide (keys above 1023 meet the clamp), all zero -- and "tiles",
    whose scale changes from tile to tile.  The maximum of 64 pixels drawn alike is nearly the same in every tile (4
    for "ties", clamped for "wide"), so those layouts alone leave every tile-level order free; "tiles" draws each
    tile's pixels below a level of its own, half of the levels in 0..6 (ties between tiles) and half in 0..1500."""
    g = _rng(w, h, *key)
    n = w * h
    tiles_x, tiles_y = sm.tile_grid(w, h)
    level = np.where(g.random(tiles_x * tiles_y) < 0.5, g.integers(0, 7, tiles_x * tiles_y),
                     g.integers(0, 1501, tiles_x * tiles_y))
    p = np.arange(n)
    tile = (p // w // 8) * tiles_x + (p % w) // 8
    return {"ties": g.integers(0, 5, n), "wide": g.integers(0, 3001, n), "zero": np.zeros(n, np.int64),
            "tiles": g.integers(0, level[tile] + 1)}


def _untouched(rest, what):
    assert (rest == EMPTY).all(), f"{what}: {int((rest != EMPTY).sum())} order entries written past the stage's range"


# ------------------------------------------------------------------ the counting sort over pixels (variant 7's probe order)
@pytest.mark.parametrize("w,h", ((1, 1), (33, 31), (32, 32), (41, 25), (683, 3)))   # n = 1, 1023, 1024, 1025, 2049
def test_pixel_sort(w, h):
    n = w * h
    r = _renderer(w, h)
    layouts = _layouts(w, h, 0)
    layouts["equal"] = np.full(n, 17)
    layouts["distinct"] = np.arange(n)
    layouts["last"] = np.where(np.arange(n) == n - 1, 900, 1)     # one expensive pixel at index n - 1
    for name, cost in layouts.items():
        buf = r.selftest_pixel_order("probe", cost)
        bad = sm.sort_violation(buf[:n], cost)
        assert bad is None, f"{w}x{h} {name}: {bad}"
        _untouched(buf[n:], f"{w}x{h} {name}")
        if name == "last":
            assert buf[0] == n - 1
        if name == "distinct" and n <= 1024:      # no two keys share a bucket: the order is fully determined
            assert np.array_equal(buf[:n], np.arange(n)[::-1])


# ------------------------------------------------------------------ tile keys and the probe statistics
def _probe_costs(cost, w, h, stride):
    """What a probe of `stride` leaves: its pixels hold the costs, every other pixel was never written."""
    c = np.asarray(cost, np.int64).reshape(h, w).copy()
    probed = np.zeros((h, w), bool)
    probed[::stride, ::stride] = True
    c[~probed] = EMPTY
    return c


@pytest.mark.parametrize("w,h", ((8, 8), (9, 1), (1, 17), (100, 37), (264, 264)))
def test_tile_keys_and_stats(w, h):
    r = _renderer(w, h)
    layouts = _layouts(w, h, 1)
    corner = np.ones((h, w), np.int64)        # the maximum in the last row and the last column of the frame
    corner[h - 1, :] = 2000
    corner[:, w - 1] = 2500
    layouts["edge"] = corner.reshape(-1)
    for name, cost in layouts.items():
        for stride in (1, 2, 4):
            for mode in (0, 1, 2):
                what = f"{w}x{h} {name} stride {stride} mode {mode}"
                c = _probe_costs(cost, w, h, stride)
                want, want_stats = sm.tile_keys(c, w, h, stride, mode)     # the model looks at probed pixels only
                keys, order, rest, stats = r.selftest_tile_schedule(c, stride, mode, stats=True)
                assert np.array_equal(keys, want), f"{what}: keys {keys[:8]} != {want[:8]}"
                assert stats == want_stats, f"{what}: stats {stats} != {want_stats}"
                bad = sm.sort_violation(order, want)
                assert bad is None, f"{what}: {bad}"
                _untouched(rest, what)
    # without the statistics the keys are the same
    keys, order, _, stats = r.selftest_tile_schedule(layouts["wide"], 1, 2)
    assert stats is None and np.array_equal(keys, sm.tile_keys(layouts["wide"], w, h, 1, 2)[0])


# ------------------------------------------------------------------ pixel sharding, with and without the probe
@pytest.mark.parametrize("w,h", ((100, 37), (9, 1)))
@pytest.mark.parametrize("shard,shards", ((0, 1), (0, 2), (1, 2), (2, 3), (6, 7)))
def test_shards(w, h, shard, shards):
    r = _renderer(w, h)
    n_tiles = int(np.prod(sm.tile_grid(w, h)))
    mine = sm.shard_tiles(n_tiles, shard, shards)
    count = sm.shard_tile_count(n_tiles, shard, shards)
    assert len(mine) == count
    for name, cost in _layouts(w, h, 2).items():
        for xcd in (False, True):           # XCD regions are ignored with pixel sharding: the global order stands
            if xcd and shards == 1:
                continue                    # one shard with XCD regions is test_xcd_regions' subject
            what = f"{w}x{h} shard {shard}/{shards} {name} xcd {xcd}"
            want = sm.tile_keys(cost, w, h, 1, 2)[0]
            if shards > 1:
                want = sm.shard_mask(want, shard, shards)
            keys, order, rest, _ = r.selftest_tile_schedule(cost, 1, 2, shard, shards, xcd_regions=xcd)
            assert np.array_equal(keys, want), what
            bad = sm.sort_violation(order, want)
            assert bad is None, f"{what}: {bad}"
            assert np.array_equal(np.sort(order[:count]), mine), f"{what}: the first {count} tiles are not the shard's"
            _untouched(rest, what)
    # without the probe: the shard's tiles in row order, nothing else written
    buf = r.selftest_pixel_order("shard", shard=shard, shards=shards)
    assert np.array_equal(buf[:count], mine)
    _untouched(buf[count:], f"{w}x{h} shard {shard}/{shards} without the probe")


# ------------------------------------------------------------------ XCD regions
XCD_FRAMES = ((64, 64), (72, 64), (100, 37), (8, 64), (24, 40), (264, 264), (16392, 8), (1, 17), (9, 1))


@pytest.mark.parametrize("w,h", XCD_FRAMES)
def test_xcd_regions(w, h):
    r = _renderer(w, h)
    tiles_x, tiles_y = sm.tile_grid(w, h)
    n_tiles = tiles_x * tiles_y
    applies = sm.xcd_applies(w, h)
    assert applies == ((w, h) not in ((16392, 8), (1, 17), (9, 1)))    # the three frames the guards divert
    layouts = _layouts(w, h, 3)
    x = np.arange(w * h) % w
    layouts["column"] = np.where(x // 8 == tiles_x // 3, 700, 0)       # all cost in one tile column
    layouts["ramp"] = 1 + (x // 8) * 1000 // tiles_x                   # cost rising linearly across the columns
    for name, cost in layouts.items():
        for mode in (0, 2):
            what = f"{w}x{h} {name} mode {mode}"
            want = sm.tile_keys(cost, w, h, 1, mode)[0]
            keys, order, rest, _ = r.selftest_tile_schedule(cost, 1, mode, xcd_regions=True)
            assert np.array_equal(keys, want), what
            assert np.array_equal(np.sort(order), np.arange(n_tiles)), f"{what}: not a permutation"
            _untouched(rest, what)
            if applies:
                model = sm.xcd_order(sm.a_sorted_order(want), want, tiles_x)
                got, exp = sm.slot_pairs(order, want, tiles_x), sm.slot_pairs(model, want, tiles_x)
                diff = np.nonzero((got != exp).any(axis=1))[0]
                assert diff.size == 0, (f"{what}: {diff.size} slots differ, first {diff[0]}: (strip, key) "
                                        f"{got[diff[0]]} != {exp[diff[0]]}")
            else:       # diverted: the global cost order stands
                bad = sm.sort_violation(order, want)
                assert bad is None, f"{what}: diverted by the guards, but {bad}"
    if applies and tiles_x >= 8:
        # the ramp's XCD order is not the global order (slot 0 is the cheapest strip's first tile, slot 7 the most
        # expensive strip's), so the comparison above is not met by a kernel that never ran or that put every tile in
        # strip 0
        want = sm.tile_keys(layouts["ramp"], w, h, 1, 0)[0]
        assert sm.sort_violation(sm.xcd_order(sm.a_sorted_order(want), want, tiles_x), want) is not None
        order = r.selftest_tile_schedule(layouts["ramp"], 1, 0, xcd_regions=True)[1]
        assert sm.sort_violation(order, want) is not None


# ------------------------------------------------------------------ variant 7's temporal order, row order, sharded rows
@pytest.mark.parametrize("w,h", ((100, 37), (9, 1), (1, 17), (64, 64)))
def test_temporal_and_row_orders(w, h):
    r = _renderer(w, h)
    n_tiles = int(np.prod(sm.tile_grid(w, h)))
    n_slots = n_tiles * 64
    rows = sm.expand_slots(np.arange(n_tiles), w, h)
    assert np.array_equal(np.sort(rows[rows != EMPTY]), np.arange(w * h))      # the model's slots hold every pixel once
    for name, rays in _layouts(w, h, 4).items():
        what = f"{w}x{h} {name}"
        buf = r.selftest_pixel_order("temporal", rays)
        tile_order, keys = r.schedule_buffer("tile_order"), r.schedule_buffer("tile_key")
        want = sm.tile_keys(rays, w, h, 1, 2)[0]          # mode 0 followed by the neighbour rule
        assert np.array_equal(keys, want), what
        if name == "tiles" and n_tiles >= 16:             # this layout does pin the order down
            assert len(np.unique(sm.clamped(want))) >= 8
        bad = sm.sort_violation(tile_order, want)
        assert bad is None, f"{what}: {bad}"
        assert np.array_equal(buf[:n_slots], sm.expand_slots(tile_order, w, h)), what
        _untouched(buf[n_slots:], what)
        assert np.array_equal(r.schedule_buffer("pix_rays"), rays)
        # the row order afterwards does not use the map
        buf = r.selftest_pixel_order("rows")
        assert np.array_equal(buf[:n_slots], rows), what
        _untouched(buf[n_slots:], what)
    for shard, shards in ((0, 1), (1, 2), (2, 3)):
        buf = r.selftest_pixel_order("shard", shard=shard, shards=shards)
        mine = sm.shard_tiles(n_tiles, shard, shards)
        assert np.array_equal(buf[:len(mine)], mine)
        _untouched(buf[len(mine):], f"{w}x{h} shard {shard}/{shards}")


# ------------------------------------------------------------------ the cost maps of real renders
@pytest.fixture(scope="module")
def bunny_w4(device_scenes):
    return device_scenes["cornell_bunny"][0].upload(0, bvh="rebuilt", width=4)


def _render_setup(variant, spp):
    r = crt_amd.Renderer(100, 37)
    r.set_kernel_variant(variant)
    r.set_camera(crt_amd.camera(spp))
    r.init_rand(41)
    return r


def test_probe_cost_map_of_a_render(bunny_w4):
    """Variant 7's probe writes rays per pixel (2 samples from the frame's RNG state, nothing else written); the sort
    only reads the map, so it is read back after the render.  Its sum is the ray count of a variant-4 render of 2
    spp from the same state, and the pixel order of the render is a descending sort of it."""
    w, h = 100, 37
    ref = _render_setup(4, 2)
    ref.render(bunny_w4, 2, 20)
    ref.synchronize()
    rays = ref.counters()["rays"]
    assert rays >= 2 * w * h
    r = _render_setup(7, 2)
    r.set_schedule(2, 0)
    r.render(bunny_w4, 2, 20)
    r.synchronize()
    assert r.last_kernel_name().startswith("crt_render_kernel<false, 7,")
    cost = r.schedule_buffer("pix_cost")
    print(f"probe map: sum {int(cost.sum())}, min {cost.min()}, max {cost.max()}; variant 4 rays {rays}")
    assert cost.shape == (w * h,) and int(cost.sum()) == rays
    assert cost.min() >= 2                        # every pixel traced its 2 camera rays
    assert r.counters()["rays"] == rays           # and the render itself the same 2 samples
    order = r.schedule_buffer("order")
    bad = sm.sort_violation(order[:w * h], cost)
    assert bad is None, bad


def test_temporal_cost_map_of_two_frames(bunny_w4):
    """Two temporal 1-spp frames of variant 7.  Frame 1 (row order) leaves its rays per pixel; frame 2 orders its tiles
    by that map.  Both halves are readable: the map after frame 1, and after frame 2 the tile order, the keys and the
    slots frame 2 ran with (frame 2 overwrites only the map)."""
    w, h = 100, 37
    n_tiles = int(np.prod(sm.tile_grid(w, h)))
    r = _render_setup(7, 1)
    r.set_temporal_order(True)
    r.render(bunny_w4, 1, 20)
    r.synchronize()
    map1 = r.schedule_buffer("pix_rays")
    rays1 = r.counters()["rays"]
    print(f"frame 1: map sum {int(map1.sum())}, rays {rays1}")
    assert map1.shape == (w * h,) and int(map1.sum()) == rays1 and map1.min() >= 1
    rows = r.schedule_buffer("order")
    assert np.array_equal(rows[:n_tiles * 64], sm.expand_slots(np.arange(n_tiles), w, h))    # frame 1 ran in row order
    r.render(bunny_w4, 1, 20, accumulate=True)
    r.synchronize()
    assert r.last_kernel_name().startswith("crt_render_kernel<false, 7,")
    tile_order, keys, slots = r.schedule_buffer("tile_order"), r.schedule_buffer("tile_key"), r.schedule_buffer("order")
    want = sm.tile_keys(map1, w, h, 1, 2)[0]
    assert np.array_equal(keys, want)
    bad = sm.sort_violation(tile_order, want)
    assert bad is None, bad
    assert want.max() > want.min() and not np.array_equal(tile_order, np.arange(n_tiles))   # a real order, not rows
    assert np.array_equal(slots[:n_tiles * 64], sm.expand_slots(tile_order, w, h))
    map2 = r.schedule_buffer("pix_rays")
    assert int(map2.sum()) == r.counters()["rays"]
