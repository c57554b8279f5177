"""Which crt_render_kernel instantiation a render launches, through the public API.

crt_renderer_render picks the row of its launch table by (variant, counting, occupancy target): the largest built
MINW <= the target, else the smallest built.  Every case names the kernel it expects and must give the frame, RNG state
and ray count of the same variant at its automatic occupancy, bit for bit: the occupancy target changes the schedule,
never the samples.  44x20 is 6x3 8x8 tiles with the last column and row partial.
"""
import numpy as np
import pytest

import crt_amd

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES, SEED = 44, 20, 4, 20, 41

# MINW launched at occupancy targets 1..8
MINW = {4: (1, 1, 1, 4, 5, 6, 7, 7), 7: (5, 5, 5, 5, 5, 6, 7, 7), (8, False): (4, 4, 4, 4, 5, 6, 7, 7),
        (8, True): (5, 5, 5, 5, 5, 6, 7, 7), 10: (5, 5, 5, 5, 5, 6, 7, 7), 3: (1, 1, 1, 4, 5, 6, 6, 6),
        2: (1, 1, 1, 1, 5, 6, 6, 8), 0: (1,) * 8, 1: (1,) * 8}


def _name(variant, minw, count=False):
    return f"crt_render_kernel<{'true' if count else 'false'}, {variant}, {minw}>"


def _expected(variant, occ, count=False):
    return _name(variant, MINW.get((variant, count), MINW.get(variant))[occ - 1], count)


@pytest.fixture(scope="module")
def bunny(device_scenes):
    hs, ref = device_scenes["cornell_bunny"]
    return {"w4": hs.upload(0, bvh="rebuilt", width=4), "w2": hs.upload(0, bvh="rebuilt", width=2), "ref": ref}


@pytest.fixture(scope="module")
def renderers():
    """One renderer per scene, reused by every case, so the schedules also meet each other's buffers."""
    out = {}
    for k in ("w4", "w2", "ref"):
        out[k] = crt_amd.Renderer(W, H)
        out[k].set_camera(crt_amd.camera(SPP))
    return out


def _render(r, dev, variant, occ=0, count=False, min_spp=0):
    r.set_kernel_variant(variant)
    r.set_occupancy_target(occ)
    r.set_schedule(2, min_spp)       # the cost probe runs unless min_spp exceeds the render's samples
    r.init_rand(SEED)
    r.render(dev, SPP, BOUNCES, count_work=count)
    r.synchronize()
    return dict(name=r.last_kernel_name(), lin=r.linear().view(np.uint32), rng=r.rng_state(), rays=r.counters()["rays"],
                occupancy=r.last_schedule()["occupancy"])


_BASE = {}


def _baseline(renderers, bunny, scene, variant):
    """The variant at its automatic occupancy, plain kernel (rendered once per scene and variant)."""
    if (scene, variant) not in _BASE:
        _BASE[scene, variant] = _render(renderers[scene], bunny[scene], variant)
    return _BASE[scene, variant]


def _same(a, b):
    assert np.array_equal(a["lin"], b["lin"]), "frame bits differ"
    assert np.array_equal(a["rng"], b["rng"]), "RNG state differs"
    assert a["rays"] == b["rays"] and a["rays"] > 0


WIDE = ([(8, occ, False) for occ in (4, 5, 6, 7)] + [(8, occ, True) for occ in (4, 6, 7)] +
        [(7, occ, False) for occ in (5, 6, 7)] + [(4, occ, False) for occ in (5, 6)])
THREADED = [(10, 5), (10, 6), (10, 7), (3, 5), (3, 6), (2, 5), (2, 6)]


@pytest.mark.parametrize("variant,occ,count", WIDE)
def test_wide_kernel_by_occupancy(renderers, bunny, variant, occ, count):
    base = _baseline(renderers, bunny, "w4", variant)
    got = _render(renderers["w4"], bunny["w4"], variant, occ, count)
    assert got["name"] == _expected(variant, occ, count)
    assert got["occupancy"] == (occ if variant == 8 else 0)     # the schedule report is variant 8's
    _same(got, base)


@pytest.mark.parametrize("scene", ["w2", "ref"])
@pytest.mark.parametrize("variant,occ", THREADED)
def test_threaded_kernel_by_occupancy(renderers, bunny, scene, variant, occ):
    base = _baseline(renderers, bunny, scene, variant)
    got = _render(renderers[scene], bunny[scene], variant, occ)
    assert got["name"] == _expected(variant, occ)
    assert got["occupancy"] == 0
    _same(got, base)


@pytest.mark.parametrize("scene", ["w2", "ref"])
@pytest.mark.parametrize("variant", [0, 1])
def test_single_instantiation_variants(renderers, bunny, scene, variant):
    got = _baseline(renderers, bunny, scene, variant)
    assert got["name"] == _name(variant, 1)
    _same(got, _baseline(renderers, bunny, scene, 3))


def test_automatic_variant_wide(renderers, bunny):
    r, dev = renderers["w4"], bunny["w4"]
    probed = _render(r, dev, -1)
    # 18 tiles are fewer than 4 per wave slot: occupancy 6, or 4 where the probe finds the frame chain-bound
    assert probed["occupancy"] in (4, 6) and probed["name"] == _name(8, probed["occupancy"])
    _same(probed, _baseline(renderers, bunny, "w4", 8))
    short = _render(r, dev, -1, min_spp=64)          # 4 spp < 64: no probe
    assert short["name"] == _name(7, 6) and short["occupancy"] == 0
    _same(short, _baseline(renderers, bunny, "w4", 7))
    for threaded_only in (3, 10):                    # not a 4-wide variant: the automatic choice
        got = _render(r, dev, threaded_only)
        assert got["name"] == probed["name"]
        _same(got, probed)


@pytest.mark.parametrize("scene", ["w2", "ref"])
def test_automatic_variant_threaded(renderers, bunny, scene):
    r, dev = renderers[scene], bunny[scene]
    probed = _render(r, dev, -1)
    assert probed["name"] == _name(10, 6) and probed["occupancy"] == 0
    _same(probed, _baseline(renderers, bunny, scene, 10))
    plain = _render(r, dev, -1, min_spp=64)
    assert plain["name"] == _name(3, 6)
    _same(plain, _baseline(renderers, bunny, scene, 3))
    for wide_only in (4, 7, 8):                      # not a threaded variant: the automatic choice
        got = _render(r, dev, wide_only)
        assert got["name"] == _name(10, 6)
        _same(got, probed)


def test_tile_schedule_after_pixel_queue_on_a_fresh_renderer(renderers, bunny):
    """Variant 7 allocates the order buffers without the tile keys; variant 8 then adds the keys."""
    r = crt_amd.Renderer(W, H)
    r.set_camera(crt_amd.camera(SPP))
    first = _render(r, bunny["w4"], 7, min_spp=64)
    assert first["name"] == _name(7, 6)
    _same(first, _baseline(renderers, bunny, "w4", 7))
    second = _render(r, bunny["w4"], 8, 7)
    assert second["name"] == _name(8, 7)
    _same(second, _baseline(renderers, bunny, "w4", 8))
