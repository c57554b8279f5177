"""Adaptive sampling on the GPU: Renderer.render_adaptive, resolve_adaptive, the per-tile readers and
the plan self-test.

Every comparison is bit for bit, on uint32 views (NaNs, whose sign and payload IEEE 754 leaves open, mapped to one
pattern first: helpers/adaptive_model.canon).

1. the plan step on crafted buffers against the numpy model: tile errors, tile samples, prev, the list as a set, its
   count, and non-increasing error along it.
2. whole frames: every tile equals the uniform frame of its own sample count (sums, RNG state, resolved bytes), and the
   numpy model predicts the sample and error maps and the stats from the uniform frames alone.
3. the refusals that need a real handle: a pixel shard, render flags.
4. the checked build in a fresh child process.
5. crt_render -adaptive.
"""
import ctypes as C
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
import adaptive_model as am  # noqa: E402
from wavefront_batches import bits, same  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
CHECKED = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
CLI = REPO / "raytracer-cuda_amd" / "bin" / "crt_render"
F32 = np.float32
INF = float("inf")
UNSUPPORTED = -5
W, H = 64, 36
SPP_MIN = 4
UNIFORM = (2, 4, 8, 12, 16, 24, 32)


# ------------------------------------------------------------------------------------------ 1. the plan, crafted
# 40 tiles with the last tile row half outside; partial tiles both ways; one tile; one partial tile; 289 tiles (more than
# a 256-lane workgroup of the list kernel); 1,089 tiles (more than one 1,024-key block of it), the last row half outside
PLAN_FRAMES = [(64, 36), (37, 19), (8, 8), (7, 5), (136, 136), (264, 260)]
KINDS = ("exact", "zero", "negative", "inf", "nan", "other_spp_above", "other_spp_below")


def _set_tile(a, w, h, t, value):
    tx = am.tiles(w, h)[1]
    x0, y0 = (t % tx) * 8, (t // tx) * 8
    a[y0:y0 + 8, x0:x0 + 8] = value


def _crafted(w, h, seed, kinds, n):
    """Seeded random sums, and one special tile per kind (spread over the tiles; with one tile only kinds[0])."""
    g = np.random.default_rng(seed)
    prev = (g.random((h, w, 3)) * 4).astype(F32)
    sums = (prev + (g.random((h, w, 3)) * 4).astype(F32)).astype(F32)
    n_tiles = int(np.prod(am.tiles(w, h)))
    spp = np.full(n_tiles, n, np.int32)
    where = {}
    for j, kind in enumerate(kinds[:n_tiles]):
        t = (j * 7 + (n_tiles - 1)) % n_tiles if n_tiles > len(kinds) else j     # the last (partial) tile first
        while t in where.values():
            t = (t + 1) % n_tiles
        where[kind] = t
        tx = am.tiles(w, h)[1]
        x0, y0 = (t % tx) * 8, (t // tx) * 8
        if kind == "exact":            # every pixel's term is 1 for n = 4, and c x 1 / c = 1: E == 1 exactly
            _set_tile(sums, w, h, t, [8, 4, 4])
            _set_tile(prev, w, h, t, [6, 2, 2])
        elif kind == "zero":
            _set_tile(sums, w, h, t, 0)
            _set_tile(prev, w, h, t, 0)
        elif kind == "negative":
            _set_tile(sums, w, h, t, [-3, 1, 1])
        elif kind == "inf":
            sums[y0, x0] = [np.inf, 1, 1]
        elif kind == "nan":
            sums[y0, x0] = [1, np.nan, 1]
        elif kind == "other_spp_above":
            spp[t] = 2 * n
        elif kind == "other_spp_below":
            spp[t] = n // 2
    return sums, prev, spp, where


def _check_plan(r, w, h, sums, prev, spp, n, nxt, tol, what):
    old_err = r.tile_error().reshape(-1) if getattr(r, "_planned", False) else np.zeros(spp.size, F32)
    listed = r.selftest_adaptive_plan(sums, prev, spp, n, nxt, tol)
    r._planned = True
    want_err, want_spp, want_prev, want_listed = am.plan(sums, prev, spp, old_err, n, nxt, tol)
    got_err = r.tile_error().reshape(-1)
    assert np.array_equal(am.canon(got_err), am.canon(want_err)), (what, "tile_error", np.flatnonzero(am.canon(got_err) != am.canon(want_err))[:8])
    assert np.array_equal(r.tile_spp().reshape(-1), want_spp), (what, "tile_spp")
    assert np.array_equal(am.canon(r.adaptive_prev()), am.canon(want_prev)), (what, "prev")
    assert np.array_equal(am.canon(r.linear()), am.canon(sums)), (what, "the sums changed")
    assert listed.size == want_listed.size, (what, "count", listed.size, want_listed.size)
    assert np.array_equal(np.sort(listed), want_listed), (what, "the list as a set")
    e = want_err[listed].astype(np.float64)
    ordered = ~np.isnan(e)
    assert (np.diff(e[ordered]) <= 0).all(), (what, "the list is not in non-increasing error")
    return want_err, want_spp, want_listed


@pytest.mark.parametrize("w,h", PLAN_FRAMES)
def test_plan_on_crafted_buffers_equals_the_model(w, h):
    r = crt_amd.Renderer(w, h)
    n_tiles = int(np.prod(am.tiles(w, h)))
    n, nxt = 4, 8
    kind_sets = [KINDS] if n_tiles >= len(KINDS) else [(k,) for k in KINDS]
    seen_listed = seen_converged = 0
    for ks, kinds in enumerate(kind_sets):
        sums, prev, spp, where = _crafted(w, h, 100 + 7 * ks + w, kinds, n)
        E = am.tile_errors(sums, prev, n)
        finite = E[np.isfinite(E) & (E > 0)]
        tols = [-1.0, 0.0, INF, 1.0, float(np.nextafter(F32(1), F32(0)))]
        if finite.size:
            tols.append(float(np.median(finite)))
        for tol in tols:
            what = f"{w}x{h} {kinds if len(kinds) == 1 else 'all kinds'} tolerance {tol!r}"
            err, new_spp, listed = _check_plan(r, w, h, sums, prev, spp, n, nxt, tol, what)
            seen_listed += listed.size
            seen_converged += int(((spp == n) & (new_spp == n)).sum())
            cand = spp == n
            if tol == INF:            # only a NaN is unconverged
                assert set(listed) == set(np.flatnonzero(cand & np.isnan(err)))
            if tol == -1.0:
                assert np.array_equal(listed_sorted := np.sort(listed), np.flatnonzero(cand)), (what, listed_sorted)
            if "exact" in where and cand[where["exact"]]:
                t = where["exact"]
                assert err[t] == F32(1)
                assert (t in listed) == (tol < 1.0), (what, "E == tolerance must converge, E > tolerance must not")
            for k in ("zero", "negative"):
                if k in where and cand[where[k]]:
                    assert err[where[k]] == 0 and (where[k] in listed) == (tol < 0)
            if "inf" in where:
                assert np.isnan(err[where["inf"]]) and where["inf"] in listed
            if "nan" in where:        # a NaN sum has I > 0 false: its pixel counts 0, the tile's error stays a number
                assert np.isfinite(err[where["nan"]])
            for k in ("other_spp_above", "other_spp_below"):
                if k in where:
                    assert where[k] not in listed and new_spp[where[k]] == spp[where[k]]
    assert seen_listed and seen_converged
    # a second step on what the first left: n = 8 looks only at the tiles the first one refined
    sums, prev, spp, _ = _crafted(w, h, 5 + h, KINDS[:1], n)
    _, spp1, listed = _check_plan(r, w, h, sums, prev, spp, n, nxt, 0.5, f"{w}x{h} first step")
    prev1 = r.adaptive_prev()
    sums2 = (sums + sums).astype(F32)
    _, spp2, listed2 = _check_plan(r, w, h, sums2, prev1, spp1, 8, 16, -1.0, f"{w}x{h} second step")
    assert np.array_equal(listed2_sorted := np.sort(listed2), np.sort(listed)), listed2_sorted
    assert set(np.unique(spp2)) <= {4, 16}


# ------------------------------------------------------------------------------------------ 2. whole frames
@pytest.fixture(scope="module")
def bunny_w4(device_scenes):
    return device_scenes["cornell_bunny"][0].upload(0, bvh="rebuilt", width=4)


@pytest.fixture(scope="module")
def scene_of(device_scenes, bunny_w4):
    """The rebuilt 4-wide bunny scene (variant 8 refines) and a reference-tree scene (variant 10 refines)."""
    return {"bunny_w4": bunny_w4, "cornell": device_scenes["cornell"][1]}


def _renderer(seed=41):
    r = crt_amd.Renderer(W, H)
    r.set_camera(crt_amd.camera(1))
    r.init_rand(seed)
    return r


def _state(r):
    r.synchronize()
    return {"sum": r.linear(), "rgba": r.rgba8(), "rng": r.rng_state()}


@pytest.fixture(scope="module")
def uniform(scene_of):
    """Uniform frames of Renderer.render from seed 41, computed once per scene and left unchanged."""
    out = {}
    for name, sc in scene_of.items():
        out[name] = {}
        for spp in UNIFORM:
            r = _renderer()
            r.render(sc, spp, 20)
            r.resolve(crt_amd.pixel_sample_scale(spp))
            out[name][spp] = _state(r)
            for a in out[name][spp].values():
                a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def median_tolerance(scene_of, uniform):
    """Per scene, the median of the non-zero tile errors of the spp_min frame: the +inf run's tile_error."""
    out = {}
    for name, sc in scene_of.items():
        r = _renderer()
        r.render_adaptive(sc, SPP_MIN, 32, INF)
        e = r.tile_error().reshape(-1)
        out[name] = float(np.median(e[e > 0]))
    return out


def _adaptive(r, sc, spp_max, tol):
    stats = r.render_adaptive(sc, SPP_MIN, spp_max, tol)
    r.resolve_adaptive()
    return dict(_state(r), tile_spp=r.tile_spp().reshape(-1), tile_error=r.tile_error().reshape(-1), stats=stats)


def _assert_adaptive_frame(got, frames, spp_max, tol, what):
    """Per-tile equality with the uniform frames, and the model's prediction from the uniform frames alone."""
    spp_map = am.expand(got["tile_spp"], W, H)
    assert set(np.unique(got["tile_spp"])) <= set(UNIFORM), (what, np.unique(got["tile_spp"]))
    for k in ("sum", "rng", "rgba"):
        want = np.zeros_like(frames[SPP_MIN][k])
        for spp in np.unique(got["tile_spp"]):
            m = spp_map == spp
            want[m] = frames[int(spp)][k][m]
        diff = bits(np.ascontiguousarray(got[k])) != bits(np.ascontiguousarray(want))
        assert not diff.any(), f"{what}: {k} differs from the uniform frames in {int(diff.sum())} words"
    want_spp, want_err, want_stats = am.predict({k: v["sum"] for k, v in frames.items()}, SPP_MIN, spp_max, tol)
    assert np.array_equal(got["tile_spp"], want_spp), (what, "tile_spp", got["tile_spp"], want_spp)
    assert np.array_equal(am.canon(got["tile_error"]), am.canon(want_err)), (what, "tile_error")
    stats = {k: got["stats"][k] for k in want_stats}
    assert stats == want_stats, (what, stats, want_stats)
    assert got["stats"]["mean_spp"] == want_stats["samples"] / (W * H) and got["stats"]["ms"] > 0
    return want_stats


@pytest.mark.parametrize("spp_max", [32, 24])
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_every_tile_equals_the_uniform_frame_of_its_sample_count(scene_of, uniform, median_tolerance, name, spp_max):
    sc, frames = scene_of[name], uniform[name]
    n_tiles = int(np.prod(am.tiles(W, H)))
    # the median error as the tolerance: both outcomes must occur, a condition on the input
    tol = median_tolerance[name]
    got = _adaptive(_renderer(), sc, spp_max, tol)
    stats = _assert_adaptive_frame(got, frames, spp_max, tol, f"{name} {spp_max} median")
    assert 0 < stats["tiles_refined"] < n_tiles and stats["passes"] >= 1, stats
    assert (got["tile_spp"] == SPP_MIN).any() and (got["tile_spp"] > SPP_MIN).any()
    # a negative tolerance: render(spp_max) everywhere
    got = _adaptive(_renderer(), sc, spp_max, -1.0)
    _assert_adaptive_frame(got, frames, spp_max, -1.0, f"{name} {spp_max} -1")
    assert (got["tile_spp"] == spp_max).all() and got["stats"]["tiles_at_max"] == n_tiles
    assert got["stats"]["samples"] == W * H * spp_max and got["stats"]["passes"] == 3
    for k in ("sum", "rng", "rgba"):
        assert same(got[k], frames[spp_max][k]), k
    # +inf: render(spp_min), one plan, tile errors filled
    got = _adaptive(_renderer(), sc, spp_max, INF)
    _assert_adaptive_frame(got, frames, spp_max, INF, f"{name} {spp_max} inf")
    assert (got["tile_spp"] == SPP_MIN).all() and got["stats"]["passes"] == 0 and got["stats"]["tiles_refined"] == 0
    assert (got["tile_error"] > 0).any()
    for k in ("sum", "rng", "rgba"):
        assert same(got[k], frames[SPP_MIN][k]), k


def test_refinement_runs_on_the_tile_kernels(scene_of, median_tolerance):
    for name, kernel in (("bunny_w4", "crt_render_kernel<false, 8, "), ("cornell", "crt_render_kernel<false, 10, ")):
        r = _renderer()
        stats = r.render_adaptive(scene_of[name], SPP_MIN, 32, median_tolerance[name])
        assert stats["passes"] >= 1 and r.last_kernel_name().startswith(kernel), (name, r.last_kernel_name())


@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_list_order_and_critical_tiles_change_nothing(scene_of, uniform, median_tolerance, name):
    for kw in ({"list_by_error": True}, {"critical_tiles": True}, {"list_by_error": True, "critical_tiles": True}):
        r = _renderer()
        stats = r.render_adaptive(scene_of[name], SPP_MIN, 32, median_tolerance[name], **kw)
        r.resolve_adaptive()
        got = dict(_state(r), tile_spp=r.tile_spp().reshape(-1), tile_error=r.tile_error().reshape(-1), stats=stats)
        _assert_adaptive_frame(got, uniform[name], 32, median_tolerance[name], f"{name} {kw}")


def test_a_handle_is_reused_and_plain_renders_interleave(scene_of, uniform, median_tolerance):
    name = "bunny_w4"
    sc, frames, tol = scene_of[name], uniform[name], median_tolerance[name]
    r = _renderer()
    first = _adaptive(r, sc, 32, tol)
    _assert_adaptive_frame(first, frames, 32, tol, "first call")
    # a plain render in between is the uniform frame, and leaves the adaptive state of the handle alone
    r.init_rand(41)
    r.render(sc, 8, 20)
    r.resolve(crt_amd.pixel_sample_scale(8))
    plain = _state(r)
    for k in ("sum", "rng", "rgba"):
        assert same(plain[k], frames[8][k]), k
    assert np.array_equal(r.tile_spp().reshape(-1), first["tile_spp"])
    # another tolerance on the same handle: the state is reset, the buffers are reused
    for other, spp_max in ((-1.0, 24), (INF, 32), (tol * 2, 32), (tol, 32)):
        r.init_rand(41)
        again = _adaptive(r, sc, spp_max, other)
        _assert_adaptive_frame(again, frames, spp_max, other, f"reused handle, tolerance {other}")
    for k in ("sum", "rng", "rgba", "tile_spp"):
        assert same(again[k], first[k]), k
    assert np.array_equal(am.canon(again["tile_error"]), am.canon(first["tile_error"]))


def test_spp_max_equal_to_spp_min_plans_nothing(scene_of, uniform):
    r = _renderer()
    got = _adaptive(r, scene_of["bunny_w4"], SPP_MIN, 0.0)
    assert got["stats"]["passes"] == 0 and got["stats"]["tiles_at_max"] == got["tile_spp"].size
    assert (got["tile_spp"] == SPP_MIN).all() and not got["tile_error"].any()
    for k in ("sum", "rng", "rgba"):
        assert same(got[k], uniform["bunny_w4"][SPP_MIN][k]), k


# ------------------------------------------------------------------------------------------ 3. refusals on a real handle
def test_pixel_shard_and_flags_are_refused(bunny_w4, uniform):
    r = _renderer()
    r.set_pixel_shard(1, 2)
    with pytest.raises(crt_amd.CrtError, match=r"status -5.*pixel shard"):
        r.render_adaptive(bunny_w4, SPP_MIN, 32, 0.1)
    r.set_pixel_shard(0, 1)
    fn = _lib.hip().crt_renderer_render_adaptive
    o = _lib.AdaptiveOptions(SPP_MIN, 32, 0.1, 0)
    for flags in (crt_amd.RENDER_ACCUMULATE, crt_amd.RENDER_COUNT_WORK, 3):
        assert fn(r.h, bunny_w4.h, C.byref(o), 20, flags, None, None) == UNSUPPORTED
        assert "flag" in _lib.hip().crt_last_error().decode()
    # nothing was rendered or allocated by the refused calls
    with pytest.raises(crt_amd.CrtError, match="no adaptive render"):
        r.tile_spp()
    assert same(r.rng_state(), _renderer().rng_state()) and not r.linear().any()
    # and without a stats pointer the call works
    assert fn(r.h, bunny_w4.h, C.byref(o), 20, 0, None, None) == 0
    assert set(np.unique(r.tile_spp())) <= set(UNIFORM)


# ------------------------------------------------------------------------------------------ 4. the checked build
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
r.set_camera(crt_amd.camera(1))
r.init_rand(41)
stats = r.render_adaptive(sc, 4, 32, float(sys.argv[3]))
r.resolve_adaptive()
r.synchronize()                                          # a device error of the checked build raises here
np.savez(sys.argv[2], flags=np.array(_lib.hip().crt_build_flags()), sum=r.linear(), rgba=r.rgba8(), rng=r.rng_state(),
         tile_spp=r.tile_spp(), tile_error=r.tile_error(), samples=np.array(stats["samples"]), passes=np.array(stats["passes"]))
"""


def test_checked_build_gives_the_same_bits(scene_of, median_tolerance, tmp_path):
    assert CHECKED.exists() and _lib.hip().crt_build_flags() == 0
    tol = median_tolerance["bunny_w4"]
    out = tmp_path / "checked.npz"
    p = subprocess.run([sys.executable, "-c", CHILD, str(REPO), str(out), repr(tol)],
                       env=dict(os.environ, CRT_HIP_LIB=str(CHECKED)), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(out)
    assert int(got["flags"]) == _lib.BUILD_CHECKED
    want = _adaptive(_renderer(), scene_of["bunny_w4"], 32, tol)
    for k in ("sum", "rgba", "rng"):
        assert same(got[k], want[k]), k
    assert np.array_equal(got["tile_spp"].reshape(-1), want["tile_spp"])
    assert np.array_equal(am.canon(got["tile_error"].reshape(-1)), am.canon(want["tile_error"]))
    assert int(got["samples"]) == want["stats"]["samples"] and int(got["passes"]) == want["stats"]["passes"] >= 1


# ------------------------------------------------------------------------------------------ 5. the CLI
def _read_ppm(path):
    data = path.read_bytes()
    fields, pos = [], 0
    while len(fields) < 4:
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        fields.append(data[pos:end])
        pos = end + 1
    assert fields[0] == b"P6" and fields[3] == b"255"
    w, h = int(fields[1]), int(fields[2])
    return np.frombuffer(data[pos:pos + w * h * 3], np.uint8).reshape(h, w, 3)


def test_cli_adaptive(device_scenes, scenes, tmp_path):
    sc = device_scenes["cornell_bunny"][1]                 # the CLI's default tree is the reference's
    r = _renderer()
    r.render_adaptive(sc, SPP_MIN, 32, INF)
    e = r.tile_error().reshape(-1)
    tol = float(np.median(e[e > 0]))
    r = _renderer()
    stats = r.render_adaptive(sc, SPP_MIN, 32, tol)
    r.resolve_adaptive()
    want = _state(r)
    out = tmp_path / "adaptive.ppm"
    p = subprocess.run([str(CLI), "-w", str(W), "-h", str(H), "-spp", "32", "-spp-min", str(SPP_MIN), "-adaptive", repr(tol),
                        "-o", str(out), *map(str, scenes["cornell_bunny"])], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert info["samples"] == stats["samples"] and info["passes"] == stats["passes"] >= 1
    assert info["tiles_at_max"] == stats["tiles_at_max"] and info["spp"] == 32 and info["spp_min"] == SPP_MIN
    assert abs(info["mean_spp"] - stats["mean_spp"]) < 1e-3 and SPP_MIN < info["mean_spp"] < 32
    img = _read_ppm(out)
    assert np.array_equal(img, want["rgba"][::-1, :, :3])               # the file holds the top row first
    # without -adaptive the program prints what it printed before
    p = subprocess.run([str(CLI), "-w", str(W), "-h", str(H), "-spp", "2", "-o", str(tmp_path / "plain.ppm"),
                        *map(str, scenes["cornell_bunny"])], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(info) == {"width", "height", "spp", "rays", "setup_s", "frame_s", "kernel_ms", "mrays_per_s", "out"}
