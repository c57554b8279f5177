"""Batch ray queries on the GPU (Scene.trace / Scene.occluded, crt_scene_trace*): DESIGN.md "Ray queries".

Ray sets: R_synth(name) = tests/test_synth_scenes.py::_test_rays (>= 20,000 primary, interior and second-generation
rays) followed by R_axis, the 80 rays of _axis_rays (direction components of +0 and -0; for `planar`, origins snapped
onto its zero-thickness planes); R_bunny = the same recipe over cornell_bunny.

1. reference tree: t bits and (object, primitive) equal OracleScene.trace for every ray; material, normal bits and
   front_face equal the values recomputed in numpy from crt_scene_export.  Tolerance zero.
2. rebuilt trees: modes 1 and 2 bit-identical; against the oracle the same primitive has the same t bits, every other
   ray is the brute-force hit over the export's primitives, at most MAX_DIFFERING_SHARE of the set.
3. the stream kernel's shapes (counts around the wave size, tiny grids with many refills per lane, refill thresholds,
   the HBM stack, all-miss / all-equal / alternating sets, permutation independence) against mode 1, bit for bit.
4. occlusion == hit & (t <= tmax) for tmax around t, both modes, both tree kinds.
5. torch tensors through the device entry on a side stream; work counts.
6. the renderer's primary rays: a pixel whose ray misses carries exactly the sky colour.
7. the checked build serves the same calls with the same results.
8. crt_render -aov normal / depth against the image computed from Scene.trace.
"""
import json
import os
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import custom_scene  # noqa: E402
import stream_gate  # noqa: E402
from bvh_emulation import _best, _is_sphere, _prim_ranks, _prim_t  # noqa: E402
from custom_scene import world_offset  # noqa: E402
from test_image_io import _decode_png  # noqa: E402
from test_ray_query_cpu import tri_normals_f32  # noqa: E402
from test_synth_scenes import MAX_DIFFERING_SHARE, MIN_RAYS, _axis_rays, _test_rays  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
CHECKED = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
CLI = REPO / "raytracer-cuda_amd" / "bin" / "crt_render"
F32 = np.float32
FIELDS = ("t", "object", "primitive", "material", "normal", "front_face")
BUNNY = "cornell_bunny"
REF_WORLDS = ("soup", "ties", "degenerate", "planar", "far", "s0", "s3_ground", "s9_ground", "s40", "only3", BUNNY)
TREES = {"w4": dict(width=4), "w4_leaf16": dict(width=4, leaf_size=16), "w4_sbvh": dict(width=4, spatial_splits=True),
         "w4_gpu": dict(width=4, gpu_build=True), "w2_leaf16": dict(width=2, leaf_size=16)}
REBUILT_WORLDS = ("soup", "ties", "planar", "s9_ground", "s40", BUNNY)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(a, b, what):
    for k in FIELDS:
        assert a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        diff = _bits(a[k]) != _bits(b[k])
        bad = np.nonzero(diff.any(1) if diff.ndim > 1 else diff)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} rays differ in {k}, first {bad[:5].tolist()}"


# ------------------------------------------------------------------------------------------ worlds and ray sets
class World:
    """One scene of the tests: its description and oracle, and its ray set with the oracle's answers, computed once."""

    def __init__(self, name, desc, oracle, ranks_of, reference_scene=None):
        self.name, self.desc, self.oracle, self.ranks_of = name, desc, oracle, ranks_of
        self.off = world_offset(name) if name != BUNNY else np.zeros(3, F32)
        self._scenes = {"reference": reference_scene} if reference_scene is not None else {}
        self._rays = self._exports = None

    def rays(self):
        if self._rays is None:
            o, d = _test_rays(types.SimpleNamespace(oracle=self.oracle), self.off)
            assert len(o) >= MIN_RAYS
            ao, ad = _axis_rays(np.random.default_rng(17), 80, -0.29, 0.29, snap=64 if self.name == "planar" else None)
            assert (np.signbit(ad) & (ad == 0)).sum() >= 40 and (~np.signbit(ad) & (ad == 0)).sum() >= 40
            o, d = np.concatenate([o, (ao + self.off).astype(F32)]), np.concatenate([d, ad])
            t, prim = self.oracle.trace(o, d)
            for a in (o, d, t, prim):
                a.setflags(write=False)
            self._rays = (o, d, t, prim)
        return self._rays

    def scene(self, tree="reference"):
        if tree not in self._scenes:
            self._scenes[tree] = (crt_amd.create_scene(self.desc, 0) if tree == "reference" else
                                  crt_amd.create_scene(self.desc, 0, "rebuilt", **TREES[tree]))
        return self._scenes[tree]

    def export(self, tree="reference"):
        self._exports = self._exports or {}
        if tree not in self._exports:
            self._exports[tree] = (crt_amd.export_desc(self.desc) if tree == "reference" else
                                   crt_amd.export_desc(self.desc, "rebuilt", **TREES[tree]))
        return self._exports[tree]


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, scenes, device_scenes, oracle_scenes):
    out = {}
    for name, cs in custom_scene.synth_worlds(custom_scene.family_files(tmp_path_factory.mktemp("rq"))).items():
        out[name] = World(name, cs.desc, cs.oracle, cs.oracle_ranks)
        out[name].keep = cs
    hs, ref = device_scenes[BUNNY]
    cs = custom_scene.CustomScene(scenes[BUNNY])       # the same world through the helper: primitive id -> rank
    out[BUNNY] = World(BUNNY, hs.desc(), oracle_scenes[BUNNY], cs.oracle_ranks, ref)
    out[BUNNY].keep = (hs, cs)
    return out


def _expected_records(w, o, d, t_ref, prim):
    """The hit records the reference tree must return, from the oracle's (t, primitive id) and the reference export:
    material = the record's material word, normal = unit(cross(e1, e2)) (Mesh.cuh:303-304) or (1 / r) * (P - c) with
    P = o + t * d (Sphere.cuh:44) in float32 operation order, front_face = dot(d, normal) < 0."""
    e = w.export()
    prims = e["prims"].reshape(-1, 3, 4)
    n = len(o)
    hit = t_ref >= 0
    exp = {"t": np.where(hit, t_ref, F32(-1)).astype(F32), "object": np.zeros(n, np.int32),
           "primitive": np.zeros(n, np.int32), "material": np.zeros(n, np.int32), "normal": np.zeros((n, 3), F32),
           "front_face": np.zeros(n, np.int32)}
    if not hit.any():
        return exp
    exp["object"][hit], exp["primitive"][hit] = prim[hit, 0], prim[hit, 1]
    rank = w.ranks_of(prim[hit])
    p = e["rank_code"][rank] & ~(1 << 30)
    rec = prims[p]
    sph = _is_sphere(e["prims"])[p]
    assert np.array_equal(sph, (e["rank_code"][rank] & (1 << 30)) != 0) and np.array_equal(sph, prim[hit, 0] < 0)
    exp["material"][hit] = np.where(sph, rec[:, 1, 1].view(np.int32), rec[:, 2, 1].view(np.int32))
    oh, dh, th = o[hit], d[hit], t_ref[hit]
    with np.errstate(all="ignore"):
        nrm = tri_normals_f32(rec)
        inv_r = F32(1) / rec[:, 0, 3]
        hp = oh + (th[:, None] * dh).astype(F32)
        ns = (inv_r[:, None] * (hp - rec[:, 0, :3]).astype(F32)).astype(F32)
    nrm = np.where(sph[:, None], ns, nrm).astype(F32)
    dot = ((dh[:, 0] * nrm[:, 0]).astype(F32) + (dh[:, 1] * nrm[:, 1]).astype(F32)).astype(F32) + (dh[:, 2] * nrm[:, 2]).astype(F32)
    exp["normal"][hit] = nrm
    exp["front_face"][hit] = (dot < 0).astype(np.int32)
    return exp


# ------------------------------------------------------------------------------------------ 1. reference tree
@pytest.mark.parametrize("name", REF_WORLDS)
def test_reference_tree_exact(worlds, name):
    w = worlds[name]
    o, d, t_ref, prim = w.rays()
    got = w.scene().trace(o, d)
    exp = _expected_records(w, o, d, t_ref, prim)
    print(f"\n{name}: {len(o)} rays, {int((t_ref >= 0).sum())} hit")
    _assert_same(got, exp, name)
    assert name in ("only3",) or (t_ref >= 0).sum() >= 1000
    if name == BUNNY:       # the identity table of the product == the one behind the expected records
        ident = crt_amd.identity_desc(w.desc)
        h = t_ref >= 0
        assert np.array_equal(ident[w.ranks_of(prim[h])], np.stack([got[k][h] for k in ("object", "primitive", "material")], 1))


# ------------------------------------------------------------------------------------------ 2. rebuilt trees
@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("name", REBUILT_WORLDS)
def test_rebuilt_trees(worlds, name, tree):
    w = worlds[name]
    o, d, t_ref, prim = w.rays()
    sc = w.scene(tree)
    got = sc.trace(o, d, mode=1)
    if TREES[tree]["width"] == 4:
        _assert_same(sc.trace(o, d, mode=2), got, f"{name}/{tree} mode 2 vs mode 1")
        _assert_same(sc.trace(o, d), got, f"{name}/{tree} automatic mode vs mode 1")
    else:
        with pytest.raises(crt_amd.CrtError, match="4-wide"):
            sc.trace(o[:64], d[:64], mode=2)
    exp = _expected_records(w, o, d, t_ref, prim)
    same = (got["object"] == exp["object"]) & (got["primitive"] == exp["primitive"]) & ((got["t"] >= 0) == (exp["t"] >= 0))
    for k in FIELDS:        # the same primitive: the same record, t bits included
        assert np.array_equal(_bits(got[k])[same], _bits(exp[k])[same]), k
    differ = np.nonzero(~same)[0]
    share = len(differ) / len(o)
    print(f"\n{name}/{tree}: {len(o)} rays, {len(differ)} on another primitive than the reference, share {share:.2e}")
    assert share <= MAX_DIFFERING_SHARE
    e = w.export(tree)
    prims, ranks = e["prims"].reshape(-1, 3, 4), _prim_ranks(e["prims"])
    ident = crt_amd.identity_desc(w.desc)
    for i in differ:        # ... is the brute-force hit over this export's primitives
        bt, br = _best(_prim_t(prims, o[i], d[i], F32(np.inf)), ranks)
        if br < 0:
            assert got["t"][i] == -1, (i, got["t"][i])
        else:
            assert F32(bt).view(np.uint32) == got["t"][i].view(np.uint32), (i, bt, got["t"][i])
            assert tuple(ident[br]) == (got["object"][i], got["primitive"][i], got["material"][i]), (i, br)


# ------------------------------------------------------------------------------------------ 3. stream-kernel shapes
@pytest.fixture(scope="module")
def bunny(worlds):
    """cornell_bunny w4, its ray set and the lane kernel's (mode 1) records for it."""
    w = worlds[BUNNY]
    o, d, _, _ = w.rays()
    sc = w.scene("w4")
    base = sc.trace(o, d, mode=1)
    for a in base.values():
        a.setflags(write=False)
    return sc, o, d, base


def _sub(h, idx):
    return {k: h[k][idx] for k in FIELDS}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_stream_counts_around_the_wave_size(bunny, n):
    sc, o, d, base = bunny
    got = sc.trace(o[:n], d[:n], mode=2)
    assert len(got["t"]) == n and got["normal"].shape == (n, 3)
    _assert_same(got, _sub(base, slice(0, n)), f"n = {n}")
    assert len(sc.occluded(o[:n], d[:n], mode=2)) == n


@pytest.mark.parametrize("grid_waves", [1, 2])
def test_stream_small_grid_many_refills(bunny, grid_waves):
    sc, o, d, base = bunny
    sel = slice(5000, 6000)                     # 1000 rays over 64 or 128 lanes: >= 7 refills per lane
    _assert_same(sc.trace(o[sel], d[sel], mode=2, grid_waves=grid_waves), _sub(base, sel), f"grid_waves = {grid_waves}")


@pytest.mark.parametrize("threshold", [1, 32, 64])
def test_stream_refill_thresholds(bunny, threshold):
    sc, o, d, base = bunny
    sel = slice(0, 4097)
    got = sc.trace(o[sel], d[sel], mode=2, grid_waves=3, refill_threshold=threshold)
    _assert_same(got, _sub(base, sel), f"refill_threshold = {threshold}")


def test_stream_hbm_stack(bunny):
    sc, o, d, base = bunny
    assert sc.stats()["stack_bound"] > 1, "stack_lds = 1 must send entries to the overflow region"
    _assert_same(sc.trace(o, d, mode=2, stack_lds=1), base, "stack_lds = 1")
    _assert_same(sc.trace(o[:4097], d[:4097], mode=2, stack_lds=1, grid_waves=3), _sub(base, slice(0, 4097)), "stack_lds = 1, 3 waves")


def _miss_set():
    rng = np.random.default_rng(11)
    d = rng.normal(size=(3000, 3)).astype(F32)
    d[:, 1] = np.abs(d[:, 1]) + F32(0.1)        # upwards, from above the box: away from everything
    o = (rng.uniform(-0.3, 0.3, (3000, 3)) + (0, 50, 0)).astype(F32)
    return o, d


def _equal_set(o, d, base):
    i = int(np.argmax(base["t"] >= 0))
    return np.repeat(o[i:i + 1], 2000, 0), np.repeat(d[i:i + 1], 2000, 0), i


def _alternating_set(o, d, base):
    hit = np.nonzero((base["object"] == 1) & (base["t"] >= 0))[0]          # object 1: the bunny mesh
    k = min(1024, len(hit))
    assert k >= 256
    deep = hit[:k]
    oo = np.empty((2 * k, 3), F32)
    dd = np.empty((2 * k, 3), F32)
    oo[0::2], dd[0::2] = (0, 50, 0), np.tile(np.array([[0, 1, 0]], F32), (k, 1))
    oo[1::2], dd[1::2] = o[deep], d[deep]
    return oo, dd


def _permutation(n):
    perm = np.random.default_rng(2).permutation(n)
    back = np.empty_like(perm)
    back[perm] = np.arange(n)
    return perm, back


def test_stream_all_rays_miss(bunny):
    sc, _, _, _ = bunny
    o, d = _miss_set()
    for mode in (1, 2):
        got = sc.trace(o, d, mode=mode)
        assert (got["t"] == -1).all() and not any(_bits(got[k]).any() for k in FIELDS[1:])
        assert not sc.occluded(o, d, mode=mode).any()


def test_stream_all_rays_equal(bunny):
    sc, o, d, base = bunny
    oo, dd, i = _equal_set(o, d, base)
    got = sc.trace(oo, dd, mode=2)
    _assert_same(got, _sub(base, np.full(2000, i)), "2000 copies of one ray")


def test_stream_alternating_miss_and_deep_rays(bunny):
    """The lanes of a wave get alternately a miss (one node step) and a ray that ends on the bunny mesh, the deepest
    subtree of the scene (the longest traversals of the set): lane fill and refill order under the most uneven load."""
    sc, o, d, base = bunny
    oo, dd = _alternating_set(o, d, base)
    want = sc.trace(oo, dd, mode=1)
    assert (want["t"][0::2] == -1).all() and (want["t"][1::2] >= 0).all()
    for kw in (dict(), dict(grid_waves=1), dict(grid_waves=2, refill_threshold=1)):
        _assert_same(sc.trace(oo, dd, mode=2, **kw), want, f"alternating {kw}")


def test_stream_output_depends_only_on_its_ray(bunny):
    sc, o, d, base = bunny
    perm, back = _permutation(len(o))
    got = sc.trace(o[perm], d[perm], mode=2)
    _assert_same(_sub(got, back), base, "permuted")


# ------------------------------------------------------------------------------------------ 4. occlusion
def _occlusion_cases(t):
    hit = t >= 0
    tt = np.where(hit, t, F32(1)).astype(F32)
    return {"t": tt, "below": np.nextafter(tt, F32(0)), "above": np.nextafter(tt, F32(np.inf)),
            "inf": np.full(len(t), np.inf, F32), "zero": np.zeros(len(t), F32), "near": np.full(len(t), 0.001, F32)}


@pytest.mark.parametrize("tree", ["reference", "w4"])
@pytest.mark.parametrize("name", [BUNNY, "soup"])
def test_occlusion(worlds, name, tree):
    w = worlds[name]
    o, d, _, _ = w.rays()
    sc = w.scene(tree)
    modes = (1, 2) if tree == "w4" else (1,)
    closest = sc.trace(o, d, mode=1)
    hit = closest["t"] >= 0
    assert hit.sum() >= 1000
    for case, tmax in _occlusion_cases(closest["t"]).items():
        want = hit & (closest["t"] <= tmax)
        assert case not in ("t", "above", "inf") or np.array_equal(want, hit)
        assert case not in ("below", "zero") or not want.any()
        for mode in modes:
            occ = sc.occluded(o, d, tmax, mode=mode)
            assert occ.dtype == np.uint8 and np.array_equal(occ, want.astype(np.uint8)), (case, mode)
            got = sc.trace(o, d, tmax, mode=mode)
            assert np.array_equal(got["t"] >= 0, want), (case, mode)
            _assert_same(_sub(got, want), _sub(closest, want), f"{case} mode {mode}: reported hits")
            assert (got["t"][~want] == -1).all() and not any(_bits(got[k][~want]).any() for k in FIELDS[1:])


# ------------------------------------------------------------------------------------------ 5. device entry / torch
def test_torch_tensors_on_a_side_stream(bunny):
    import torch
    sc, o, d, base = bunny
    source = torch.from_numpy(crt_amd.pack_rays(o, d)).to("cuda:0")
    rays = torch.zeros_like(source)                            # what a query on another stream would trace
    stream = stream_gate.side_stream()
    torch.cuda.synchronize()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        assert torch.cuda.current_stream() == stream and stream != torch.cuda.default_stream()
        stream_gate.gate(stream)
        rays.copy_(source)                                     # the rays arrive on this stream, behind the gate
        hits = sc.trace(rays, mode=2, count_work=True)         # the stream kernel: the step counts are its own
        stats = sc.trace_stats()
        again = sc.trace(rays, mode=2, count_work=True)
        stats2 = sc.trace_stats()
        rays.zero_()
        stream_gate.gate(stream)                               # trace_stats waited: a gate again, and the rays behind it
        rays.copy_(source)
        auto = sc.trace(rays)                                  # automatic: the lane kernel at this size
        occ = sc.occluded(rays, mode=2)
        occ1 = sc.occluded(rays, mode=1)
        occ0 = sc.occluded(rays)
    stream.synchronize()
    assert hits["f32"].shape == (len(o), 8) and hits["f32"].dtype == torch.float32 and hits["f32"].is_cuda
    assert hits["i32"].dtype == torch.int32 and hits["i32"].data_ptr() == hits["f32"].data_ptr()
    _assert_same({k: hits[k].cpu().numpy() for k in FIELDS}, base, "torch")
    assert occ.dtype == torch.uint8 and occ.shape == (len(o),) and occ.is_cuda
    assert np.array_equal(occ.cpu().numpy(), (base["t"] >= 0).astype(np.uint8))
    assert torch.equal(occ, occ1) and torch.equal(occ, occ0)
    assert torch.equal(hits["i32"], again["i32"]) and torch.equal(hits["i32"], auto["i32"])
    print("\ntrace_stats:", stats)
    assert stats["rays"] == len(o) and stats["kernel_ms"] > 0
    assert 0 < stats["step_active_lanes"] <= stats["step_lane_slots"] and stats["step_lane_slots"] % 64 == 0
    for k in ("rays", "box_tests", "tri_tests", "sphere_tests"):
        assert stats[k] == stats2[k] and stats[k] > 0, k
    # numpy rays with count_work take the device entry too; the lane kernel over 4-wide nodes counts its rays only
    sc.trace(o[:1000], d[:1000], mode=1, count_work=True)
    assert sc.trace_stats()["rays"] == 1000
    with pytest.raises(ValueError):
        sc.trace(rays[:, :7])
    with pytest.raises(ValueError):
        sc.trace(rays.cpu())


def test_reference_tree_counts_the_oracles_work(worlds):
    """The lane kernel over the reference tree is the render kernels' trace<>: its box, triangle and sphere counts for a
    set of rays are the oracle's for the same rays (a 1-bounce render of exactly these primary rays)."""
    cam = crt_amd.camera(1)
    o, d = custom_scene.camera_rays(cam, 64, 36, 1)
    w = worlds[BUNNY]
    w.scene().trace(o, d, count_work=True)
    st = w.scene().trace_stats()
    _, _, cnt = w.oracle.render(crt_amd.camera_floats(cam), 64, 36, 1, 1, nthreads=16)
    assert cnt["rays"] == 64 * 36
    for k in ("rays", "box_tests", "tri_tests", "sphere_tests"):
        assert st[k] == cnt[k], (k, st[k], cnt[k])


def test_host_entries_refuse_bad_rays_before_launching(bunny):
    sc, o, d, _ = bunny
    r = crt_amd.pack_rays(o[:100], d[:100])
    r[37, 4:7] = 0
    with pytest.raises(crt_amd.CrtError, match="ray 37"):
        sc.trace(r)
    with pytest.raises(crt_amd.CrtError, match="ray 37"):
        sc.occluded(r)


# ------------------------------------------------------------------------------------------ 6. the renderer's rays
def _sky_f32(d):
    """sky(d) of CRTUtility.cuh:34-38 in float32 operation order."""
    l2 = ((d[:, 0] * d[:, 0]).astype(F32) + (d[:, 1] * d[:, 1]).astype(F32)).astype(F32) + (d[:, 2] * d[:, 2]).astype(F32)
    uy = ((F32(1) / np.sqrt(l2).astype(F32)).astype(F32) * d[:, 1]).astype(F32)
    t = (F32(0.5) * (uy + F32(1)).astype(F32)).astype(F32)
    white = (F32(1) - t).astype(F32)
    return np.stack([(white + (t * F32(c)).astype(F32)).astype(F32) for c in (0.5, 0.7, 1.0)], 1)


@pytest.mark.parametrize("view", ["bench", "outside"])
def test_consistent_with_the_renderer(worlds, view):
    """bench: the benchmark's pose inside the box (every primary ray hits); outside: from above and in front of the
    box, looking along -z over the ground sphere's horizon (the upper rows see the sky)."""
    w, h = 64, 36
    wd = worlds[BUNNY]
    sc = wd.scene()
    cam = crt_amd.camera(1) if view == "bench" else crt_amd.camera(1, pos=(0.0, 1.5, 2.0))
    r = crt_amd.Renderer(w, h)
    r.set_camera(cam)
    r.init_rand(41)
    r.render(sc, 1, 1, count_work=True)
    r.synchronize()
    lin = r.linear().reshape(-1, 3)
    assert r.counters()["rays"] == w * h
    o, d = custom_scene.camera_rays(cam, w, h, 1)
    got = sc.trace(o, d)
    miss = got["t"] < 0
    print(f"\n{view}: {int(miss.sum())} of {w * h} primary rays miss")
    assert view == "bench" or miss.sum() >= w * h // 8
    assert np.array_equal(_bits(lin[miss]), _bits(_sky_f32(d[miss])))
    # a ray that hits ends at the bounce limit: the pixel holds nothing (or the emission of a light it hit)
    hs = wd.keep[0]
    mats = hs.loader_arrays()[4]
    lights = {i for i, m in enumerate(mats) if int(m[0]) == 3}
    dark = ~miss & ~np.isin(got["material"], list(lights))
    assert dark.sum() > 0 and not lin[dark].any()


# ------------------------------------------------------------------------------------------ 7. checked build
CHILD = r"""
import json, sys
from pathlib import Path
import numpy as np
repo = Path(sys.argv[1])
sys.path[:0] = [str(repo / "raytracer-cuda_amd"), str(repo / "oracle")]
import crt_amd
from crt_amd import _lib, assets
sets = np.load(sys.argv[2])
hs = crt_amd.HostScene(assets.scene_files("cornell_bunny"))
sc = hs.upload(0, bvh="rebuilt", width=4)
out = {"flags": np.array(_lib.hip().crt_build_flags())}
for key, name, lo, hi, kw in json.loads(sys.argv[4]):
    o, d = sets[name + "_o"][lo:hi], sets[name + "_d"][lo:hi]
    if kw.pop("occluded", False):
        out[key] = sc.occluded(o, d, **kw)          # a device error of the checked build raises here
    else:
        h = sc.trace(o, d, **kw)
        out[key] = np.column_stack([np.ascontiguousarray(h[k]).view(np.uint32)
                                    for k in ("t", "object", "primitive", "material", "normal", "front_face")])
np.savez(sys.argv[3], **out)
"""


def _rows(h):
    return np.column_stack([_bits(h[k]) for k in FIELDS])


def test_checked_build_serves_the_same_calls(bunny, tmp_path):
    """Every shape of test 3 through the checked build (lib/checked/), in a child process as tests/test_gpu_synth.py
    loads it (one HIP library per process).  The checked build re-checks every leaf-round (owner, primitive) pair and
    reports a bad one as a device error, which would make the child's call raise.  Expected: the fast library's lane
    kernel (mode 1) on the same rays, bit for bit."""
    sc, o, d, base = bunny
    assert CHECKED.exists() and _lib.hip().crt_build_flags() == 0
    mo, md = _miss_set()
    eo, ed, _ = _equal_set(o, d, base)
    ao, ad = _alternating_set(o, d, base)
    perm, back = _permutation(len(o))
    sets = {"main": (o, d), "miss": (mo, md), "equal": (eo, ed), "alt": (ao, ad), "perm": (o[perm], d[perm])}
    np.savez(tmp_path / "sets.npz", **{f"{k}_{c}": v[j] for k, v in sets.items() for j, c in enumerate("od")})
    plan = [[f"n{n}", "main", 0, n, dict(mode=2)] for n in (0, 1, 63, 64, 65, 129)]
    plan += [[f"gw{g}", "main", 5000, 6000, dict(mode=2, grid_waves=g)] for g in (1, 2)]
    plan += [[f"thr{t}", "main", 0, 4097, dict(mode=2, grid_waves=3, refill_threshold=t)] for t in (1, 32, 64)]
    plan += [["hbm", "main", 0, len(o), dict(mode=2, stack_lds=1)],
             ["hbm3", "main", 0, 4097, dict(mode=2, stack_lds=1, grid_waves=3)],
             ["miss", "miss", 0, len(mo), dict(mode=2)],
             ["equal", "equal", 0, len(eo), dict(mode=2)],
             ["alt", "alt", 0, len(ao), dict(mode=2)],
             ["alt1", "alt", 0, len(ao), dict(mode=2, grid_waves=1)],
             ["alt2", "alt", 0, len(ao), dict(mode=2, grid_waves=2, refill_threshold=1)],
             ["perm", "perm", 0, len(o), dict(mode=2)],
             ["lane", "main", 0, 129, dict(mode=1)],
             ["occ", "main", 0, 4097, dict(mode=2, grid_waves=3, occluded=True)],
             ["occ_miss", "miss", 0, len(mo), dict(mode=2, occluded=True)]]
    res = tmp_path / "checked.npz"
    env = dict(os.environ, CRT_HIP_LIB=str(CHECKED))
    p = subprocess.run([sys.executable, "-c", CHILD, str(REPO), str(tmp_path / "sets.npz"), str(res), json.dumps(plan)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(res)
    assert int(got["flags"]) == _lib.BUILD_CHECKED
    want = {"main": _rows(base), "miss": _rows(sc.trace(mo, md, mode=1)), "equal": _rows(sc.trace(eo, ed, mode=1)),
            "alt": _rows(sc.trace(ao, ad, mode=1)), "perm": _rows(base)[perm]}
    assert (want["miss"][:, 0] == _bits(F32(-1))).all() and not want["miss"][:, 1:].any()
    assert (want["equal"] == want["equal"][0]).all() and want["equal"][0, 0] != _bits(F32(-1))
    for key, name, lo, hi, kw in plan:
        if kw.get("occluded"):
            exp = (want[name][lo:hi, 0] != _bits(F32(-1))).astype(np.uint8)
        else:
            exp = want[name][lo:hi]
        assert got[key].shape == exp.shape and np.array_equal(got[key], exp), key
    assert np.array_equal(got["perm"][back], _rows(base))


# ------------------------------------------------------------------------------------------ 8. crt_render -aov
def _centre_rays(cam, w, h):
    """Camera::getRay (Camera.cuh:32-44) through the pixel centres with lens offset 0, float32 operation order."""
    c = crt_amd.camera_floats(cam)
    pos, llc, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    y, x = np.mgrid[0:h, 0:w]
    u = ((x.reshape(-1).astype(F32) + F32(0.5)) / F32(w)).astype(F32)[:, None]
    v = ((y.reshape(-1).astype(F32) + F32(0.5)) / F32(h)).astype(F32)[:, None]
    d = (((llc + (u * hor).astype(F32)).astype(F32) + (v * ver).astype(F32)).astype(F32) - pos).astype(F32)
    return np.repeat(pos[None], w * h, 0).astype(F32), d


def _byte(c):
    return (F32(255) * c.astype(F32) + F32(0.5)).astype(F32).astype(np.int32).astype(np.uint8)


@pytest.mark.parametrize("aov", ["normal", "depth", "object"])
def test_cli_aov(worlds, scenes, tmp_path, aov):
    w, h = 64, 36
    out = tmp_path / f"{aov}.png"
    p = subprocess.run([str(CLI), "-w", str(w), "-h", str(h), "-aov", aov, "-o", str(out), *map(str, scenes[BUNNY])],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    img = _decode_png(out.read_bytes())
    assert img.shape == (h, w, 3) and info["rays"] == w * h and info["aov"] == aov
    o, d = _centre_rays(crt_amd.camera(1), w, h)
    got = worlds[BUNNY].scene().trace(o, d)
    hit = got["t"] >= 0
    assert info["hits"] == int(hit.sum()) and hit.sum() > w * h // 2
    want = np.zeros((w * h, 3), np.uint8)
    if aov == "depth":
        want[hit] = _byte(F32(1) / (F32(1) + got["t"][hit]).astype(F32))[:, None]
    elif aov == "normal":
        want[hit] = _byte((F32(0.5) * got["normal"][hit]).astype(F32) + F32(0.5))
    else:
        palette = np.array([[230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180],
                            [70, 240, 240], [240, 50, 230]], np.uint8)
        want[hit] = palette[got["object"][hit] & 7]
        assert len(np.unique(got["object"][hit])) >= 2
    assert np.array_equal(img, want.reshape(h, w, 3)[::-1])         # the file holds the top row first
