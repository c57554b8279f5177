"""Synthetic scenes, sphere counts and axis rays on the CPU (no GPU needed).

The asset scenes always hold two spheres, at most three meshes and no coincident, degenerate or far-away geometry.
Here the generated families of tests/helpers/synth_scenes.py and sphere worlds of 0 to 40 spheres (reachable only
through the C ABI, tests/helpers/custom_scene.py) are checked through crt_scene_export:

* both loaders agree on every generated file set, and every scene builds;
* the rebuilt layouts are well formed at leaf sizes 1, 4, 16, width 2 and with spatial splits; spheres are kept
  per ray up to eight and go into the tree above that;
* the restated variant-4 traversal (kernel slab arithmetic: clamped 1/d, one fma per plane, entry row by sign bit)
  returns the brute-force closest hit bit for bit, on random rays and on rays with one or two exactly zero direction
  components of either sign;
* the rebuilt tree against the reference's own traversal (oracle_trace_rays): same primitive -> same t bit for bit;
  rays where they differ are ones where brute force over the reachable primitives confirms the rebuilt answer, and
  they are at most MAX_DIFFERING_SHARE of the rays.  The share per scene is printed.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd
import pyoracle

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import synth_scenes as synth  # noqa: E402
from bvh_emulation import (_best, _box_inv, _check_threaded, _check_wide, _is_sphere, _prim_ranks,  # noqa: E402
                           _prim_t, _trace_wide_rays, _wide_boxes)
import custom_scene  # noqa: E402
from custom_scene import FAMILIES, ONLY, WORLDS, world_offset as _offset  # noqa: E402
from test_host_parity import _compare_scene  # noqa: E402

F32 = np.float32
# the reference's unpadded boxes may round a genuine hit away; more than this share of differing rays is a broken tree
MAX_DIFFERING_SHARE = 1e-3
MIN_RAYS = 20000


@pytest.fixture(scope="module")
def family_files(tmp_path_factory):
    return custom_scene.family_files(tmp_path_factory.mktemp("synth"))


@pytest.fixture(scope="module")
def scenes(family_files):
    return custom_scene.synth_worlds(family_files)


def _tri_records(cs):
    prims = cs.ref_export()["prims"].reshape(-1, 3, 4)
    return prims[~_is_sphere(cs.ref_export()["prims"])]


# ------------------------------------------------------------------------------------------ loaders, content
@pytest.mark.parametrize("name", FAMILIES)
def test_loaders_agree_and_scene_builds(family_files, scenes, name):
    _compare_scene(family_files[name])             # positions, indices, face materials, mesh info, materials, BVHs
    cs = scenes[name]
    assert cs.ref_export()["ranks"] == len(cs.loaded.indices) // 3 + 2
    assert (cs.loaded.mesh_info[:, 3] // 3 <= 2000).all()


def test_families_hold_what_they_are_for(scenes):
    tri = _tri_records(scenes["ties"])
    geo = tri.copy()
    geo[:, 2, 1:] = 0                                # geometry words only: v0, e1, e2
    _, inv, cnt = np.unique(geo.reshape(len(geo), -1).view(np.uint32), axis=0, return_inverse=True, return_counts=True)
    assert 0.08 * len(tri) <= (cnt[inv] > 1).sum() - (cnt > 1).sum() <= 0.12 * len(tri)    # the duplicates
    assert (cnt == 2).sum() >= 10 and (cnt == 3).sum() >= 10 and cnt.max() == 3
    for g in np.nonzero(cnt > 1)[0]:                 # every copy under another material
        mats = tri[inv.ravel() == g][:, 2, 1].view(np.int32)
        assert len(set(mats.tolist())) == len(mats)

    tri = _tri_records(scenes["degenerate"]).astype(np.float64)
    e1 = np.stack([tri[:, 0, 3], tri[:, 1, 0], tri[:, 1, 1]], 1)
    e2 = np.stack([tri[:, 1, 2], tri[:, 1, 3], tri[:, 2, 0]], 1)
    l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
    area = np.linalg.norm(np.cross(e1, e2), axis=1)
    assert ((l1 == 0) | (l2 == 0)).sum() == 20                                   # two equal vertices
    needle = (l1 > 0) & (l2 > 0) & (np.minimum(l1, l2) < 2e-6 * np.maximum(l1, l2))
    collinear = (l1 > 0) & (l2 > 0) & ~needle & (area < 1e-5 * l1 * l2)
    assert needle.sum() == 20 and collinear.sum() == 20                          # edge ratio 1e6; collinear

    cs = scenes["planar"]
    assert (cs.loaded.mesh_info[:, 3] // 3).tolist()[1] == 1                     # a mesh of one triangle
    pos = cs.loaded.positions[4:]                                                # all but the floor's corners
    assert np.array_equal(pos * 64, np.round(pos * 64)), "vertices lie on the 1/64 grid exactly"
    assert cs.export("rebuilt", width=4)["excluded"] > 0                         # zero-thickness reference leaves

    cs = scenes["many_meshes"]
    assert len(cs.loaded.mesh_info) == 12 and (cs.loaded.mesh_info[:, 3] // 3 >= 8).all()
    assert (cs.loaded.mesh_info[1:, 5] > 0).all()                                # materialIDOffset on every file
    _, ints = cs.scene_nodes
    depth = {0: 0}
    for i, (left, right, _, _, leaf) in enumerate(ints):
        if not leaf:
            depth[int(left)] = depth[int(right)] = depth[i] + 1
    assert max(depth.values()) >= 4

    assert np.abs(scenes["far"].loaded.positions).min() > 999


# ------------------------------------------------------------------------------------------ export structure
OPTS = {"w4": dict(width=4), "w4_leaf1": dict(width=4, leaf_size=1), "w4_leaf16": dict(width=4, leaf_size=16),
        "w2_leaf16": dict(width=2, leaf_size=16), "w4_sbvh": dict(width=4, spatial_splits=True)}


@pytest.mark.parametrize("opts", list(OPTS))
@pytest.mark.parametrize("name", FAMILIES + WORLDS + ONLY)
def test_export_structure(scenes, name, opts):
    cs = scenes[name]
    o = OPTS[opts]
    e = cs.export("rebuilt", **o)
    n_ref = cs.ref_export()["ranks"]
    assert e["ranks"] == n_ref and e["width"] == o["width"]
    prims = e["prims"].reshape(-1, 3, 4)
    ranks = _prim_ranks(e["prims"])
    if o["width"] == 4:
        # up to eight spheres: all per ray; above: the small ones in the tree, spheres of radius >= 1 still per ray
        per_ray = cs.n_spheres if cs.n_spheres <= 8 else (1 if name == "s9_ground" else 0)
        assert e["n_ray_spheres"] == per_ray
        in_tree = int(_is_sphere(e["prims"])[:e["sphere_first"]].sum()) if len(prims) else 0
        assert in_tree == cs.n_spheres - per_ray
    else:
        assert e["n_ray_spheres"] == 0
    uniq, cnt = np.unique(ranks, return_counts=True)
    if o.get("spatial_splits"):
        assert len(uniq) + e["excluded"] == n_ref
    else:
        assert len(ranks) == len(uniq) and len(ranks) + e["excluded"] == n_ref
    if len(prims) == 0:                               # no mesh and no sphere in the tree: the empty 4-wide root
        assert name == "only3" and o["width"] == 4
    if o["width"] == 4:
        _check_wide(e, prims, split_ranks=uniq[cnt > 1])
    else:
        _check_threaded(e, prims)


# ------------------------------------------------------------------------------------------ traversal
def _axis_rays(rng, n, lo, hi, snap=None):
    """n rays with one or two direction components exactly zero, +0 and -0 alike."""
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    if snap is not None:                               # origins on grid planes: rays inside zero-thickness boxes
        o[::2] = (np.round(o[::2] * snap) / snap).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    for i in range(n):
        zero = [(i // 2) % 3] if i % 4 < 2 else [(i // 2) % 3, (i // 2 + 1 + (i // 12) % 2) % 3]
        d[i, zero] = -0.0 if i % 2 else 0.0
    return o, d


def _slab_f64(q, o, d):
    """The four child boxes of node rows q (8, 4) against ray (o, d) over [0.001, inf) in float64, from the
    definition: a zero direction component never leaves its slab, so the box is entered only if lo <= o < hi there
    (the clamped reciprocal keeps the sign of plane - o, and a ray on the lo plane enters at t = 0).  Returns
    (hit, decisive): decisive = the entry and exit differ by far more than float32 rounding."""
    t0, t1, ok = np.full(4, 0.001), np.full(4, np.inf), np.ones(4, bool)
    for k in range(3):
        lo, hi = q[2 * k].astype(np.float64), q[2 * k + 1].astype(np.float64)
        ok &= lo < hi                                   # an unused slot (lo = hi = 1e30) is never entered
        if d[k] == 0:
            ok &= (lo <= o[k]) & (o[k] < hi)
        else:
            a, b = (lo - o[k]) / np.float64(d[k]), (hi - o[k]) / np.float64(d[k])
            t0, t1 = np.maximum(t0, np.minimum(a, b)), np.minimum(t1, np.maximum(a, b))
    return ok & (t0 < t1), ~ok | (np.abs(t1 - t0) > 1e-3 * (1 + np.abs(t0)))


@pytest.mark.parametrize("name", ("soup", "planar", "far", "s9_ground", "s40"))
def test_axis_ray_box_decisions(scenes, name):
    """_wide_boxes (the kernel's clamped-reciprocal fma slab test) against the float64 definition, for every node of
    the default export and rays with exactly zero direction components: a box whose slab on a zero axis the origin is
    outside of is never entered, one the ray runs inside of never culled."""
    cs = scenes[name]
    off = _offset(name)
    e = cs.export("rebuilt", width=4)
    nodes = e["nodes"].reshape(-1, 8, 4)
    rng = np.random.default_rng(23)
    o, d = _axis_rays(rng, 48, -0.29, 0.29, snap=64 if name == "planar" else None)
    o = (o + off).astype(np.float32)
    binv = _box_inv(d)
    assert (d == 0).sum() >= 48 and np.isfinite(o).all()
    n_dec = n_all = n_hit = 0
    for i in range(len(o)):
        t0, hit = _wide_boxes(nodes, np.repeat(o[i:i + 1], len(nodes), 0), np.repeat(binv[i:i + 1], len(nodes), 0),
                              np.full(len(nodes), np.inf, np.float32))
        for j, q in enumerate(nodes):
            want, decisive = _slab_f64(q, o[i], d[i])
            assert np.array_equal(hit[j][decisive], want[decisive]), (i, j, o[i], d[i], hit[j], want)
            n_dec += int(decisive.sum())
            n_all += 4
            n_hit += int(want.sum())
    # indecisive: boxes thinner than the margin that the ray crosses (the padded boxes of wall triangles)
    assert n_dec >= 0.95 * n_all and n_hit > 0


def _brute(prims, ranks, o, d):
    t, r = np.full(len(o), np.inf, np.float32), np.full(len(o), -1, np.int64)
    for i in range(len(o)):
        t[i], r[i] = _best(_prim_t(prims, o[i], d[i], np.float32(np.inf)), ranks)
    return t, r


@pytest.mark.parametrize("name", FAMILIES + WORLDS + ONLY)
def test_traversal_equals_brute_force(scenes, name):
    """200 rays per export: 120 interior rays (every other one aimed near a primitive's anchor point), 80 axis
    rays."""
    cs = scenes[name]
    off = _offset(name)
    rng = np.random.default_rng(17)
    o = (rng.uniform(-0.29, 0.29, (120, 3)) + off).astype(np.float32)
    d = rng.normal(size=(120, 3)).astype(np.float32)
    anchor = cs.ref_export()["prims"].reshape(-1, 3, 4)[:, 0, :3]
    anchor = anchor[np.abs(anchor - off).max(1) < 1]                 # not the ground sphere's centre
    d[::2] = (anchor[rng.integers(0, len(anchor), 60)] + rng.normal(0, 0.02, (60, 3)) - o[::2]).astype(np.float32)
    ao, ad = _axis_rays(rng, 80, -0.29, 0.29, snap=64 if name == "planar" else None)
    o, d = np.concatenate([o, (ao + off).astype(np.float32)]), np.concatenate([d, ad])
    assert (np.signbit(ad) & (ad == 0)).sum() >= 40 and (~np.signbit(ad) & (ad == 0)).sum() >= 40
    exports = [OPTS["w4"]] + ([OPTS["w4_leaf16"], OPTS["w4_sbvh"], OPTS["w4_leaf1"]] if name in FAMILIES else [])
    n_hit = 0
    for opts in exports:
        e = cs.export("rebuilt", **opts)
        prims, ranks = e["prims"].reshape(-1, 3, 4), _prim_ranks(e["prims"])
        bt, br = _brute(prims, ranks, o, d)
        gt, gr = _trace_wide_rays(e, prims, ranks, o, d)
        bad = np.nonzero((gr != br) | (gt.view(np.uint32) != bt.view(np.uint32)))[0]
        assert len(bad) == 0, (opts, bad[:5].tolist(), gt[bad[:5]], bt[bad[:5]], gr[bad[:5]], br[bad[:5]])
        n_hit += int((gr >= 0).sum())
    assert n_hit >= 60 * len(exports), "the rays must exercise the leaves"


def _test_rays(cs, off, seed=3, n_interior=9000):
    """Primary rays of the bench camera (96x54, one sample, Camera::getRay), random interior rays, and a second
    generation leaving the first one's hit points in random directions (origins on surfaces, as bounces have)."""
    rng = np.random.default_rng(seed)
    cam = crt_amd.camera_floats(crt_amd.camera(1))
    cam[0:3] += off
    cam[3:6] += off
    w, h = 96, 54
    xy = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.int32)
    state = np.stack([pyoracle.rng_init(41, i) for i in range(len(xy))])
    prim = pyoracle.kat_get_ray(cam, w, h, xy, state)
    o = np.concatenate([prim[:, :3], (rng.uniform(-0.3, 0.3, (n_interior, 3)) + off).astype(np.float32)])
    d = np.concatenate([prim[:, 3:], rng.normal(size=(n_interior, 3)).astype(np.float32)])
    t, _ = cs.oracle.trace(o, d)
    hit = t >= 0
    o2 = (o[hit] + (t[hit, None] * d[hit]).astype(np.float32)).astype(np.float32)      # Ray::at
    d2 = rng.normal(size=o2.shape).astype(np.float32)
    extra = max(0, MIN_RAYS - len(o) - len(o2))                                        # scenes most rays miss
    o3 = (rng.uniform(-0.3, 0.3, (extra, 3)) + off).astype(np.float32)
    d3 = rng.normal(size=(extra, 3)).astype(np.float32)
    return np.concatenate([o, o2, o3]).astype(np.float32), np.concatenate([d, d2, d3]).astype(np.float32)


@pytest.mark.parametrize("name", FAMILIES + WORLDS + ONLY)
def test_rebuilt_matches_reference_hit_rule(scenes, name):
    cs = scenes[name]
    e = cs.export("rebuilt", width=4)
    prims, ranks = e["prims"].reshape(-1, 3, 4), _prim_ranks(e["prims"])
    o, d = _test_rays(cs, _offset(name))
    assert len(o) >= MIN_RAYS
    t_ref, prim = cs.oracle.trace(o, d)
    r_ref = np.where(t_ref >= 0, cs.oracle_ranks(prim), -1)
    t_ref = np.where(t_ref >= 0, t_ref, np.inf).astype(np.float32)
    t_new, r_new = _trace_wide_rays(e, prims, ranks, o, d)
    same = r_ref == r_new
    assert np.array_equal(t_ref[same].view(np.uint32), t_new[same].view(np.uint32)), "same primitive, different t"
    differ = np.nonzero(~same)[0]
    share = len(differ) / len(o)
    print(f"\n{name}: {len(o)} rays, {int((r_new >= 0).sum())} hit, {len(differ)} differ from the reference, "
          f"share {share:.2e}")
    for i in differ:
        bt, br = _best(_prim_t(prims, o[i], d[i], np.float32(np.inf)), ranks)
        assert br == r_new[i] and np.float32(bt).view(np.uint32) == t_new[i].view(np.uint32), \
            f"ray {i}: rebuilt ({t_new[i]}, {r_new[i]}) is not the brute-force hit ({bt}, {br}); reference {t_ref[i]}"
    assert share <= MAX_DIFFERING_SHARE
    assert (r_new >= 0).sum() >= 1000


# ------------------------------------------------------------------------------------------ axis cameras
@pytest.fixture(scope="module")
def axis_cameras(scenes):
    return custom_scene.axis_cameras(custom_scene.planar_plane_y(scenes["planar"]),
                                     custom_scene.planar_straight_xy(scenes["planar"]))


def test_axis_cameras_give_zero_components(axis_cameras):
    rays = {k: custom_scene.camera_rays(cam, 8, 8, 4)[1] for k, cam in axis_cameras.items()}
    for k in ("dy_plus0", "in_plane"):
        assert (rays[k][:, 1] == 0).all() and not np.signbit(rays[k][:, 1]).any()
    # d.y = (-0) - (+0) - offset.y, and offset.y = right.y * (+-0) + up.y * (+-0) is -0 only when both zero lens
    # coordinates are negative: -0 on three samples in four, +0 on the fourth (no camera gives -0 on every sample)
    minus = np.signbit(rays["dy_minus0"][:, 1])
    assert (rays["dy_minus0"][:, 1] == 0).all() and 0.7 <= minus.mean() < 1
    assert (rays["straight"] == np.array([0, 0, -1], np.float32)).all()


@pytest.mark.parametrize("cam_name", ["dy_plus0", "dy_minus0", "straight", "in_plane"])
@pytest.mark.parametrize("name", ["s2", "planar"])
def test_axis_camera_rays_match_reference(scenes, axis_cameras, name, cam_name):
    """The primary rays of the hand-built cameras (8x8, 64 samples): rebuilt == reference wherever both hit the same
    primitive, every other ray confirmed by brute force, at most MAX_DIFFERING_SHARE of them."""
    cs = scenes[name]
    e = cs.export("rebuilt", width=4)
    prims, ranks = e["prims"].reshape(-1, 3, 4), _prim_ranks(e["prims"])
    o, d = custom_scene.camera_rays(axis_cameras[cam_name], 8, 8, 64)
    t_ref, prim = cs.oracle.trace(o, d)
    r_ref = np.where(t_ref >= 0, cs.oracle_ranks(prim), -1)
    t_ref = np.where(t_ref >= 0, t_ref, np.inf).astype(np.float32)
    t_new, r_new = _trace_wide_rays(e, prims, ranks, o, d)
    same = r_ref == r_new
    assert np.array_equal(t_ref[same].view(np.uint32), t_new[same].view(np.uint32))
    differ = np.nonzero(~same)[0]
    print(f"\n{name}/{cam_name}: {len(o)} rays, {int((r_new >= 0).sum())} hit, {len(differ)} differ from the reference")
    for i in differ:
        bt, br = _best(_prim_t(prims, o[i], d[i], np.float32(np.inf)), ranks)
        assert br == r_new[i] and np.float32(bt).view(np.uint32) == t_new[i].view(np.uint32)
    assert len(differ) <= MAX_DIFFERING_SHARE * len(o)
    assert (r_new >= 0).sum() > 0


# ------------------------------------------------------------------------------------------ large spheres
@pytest.mark.parametrize("name", ["s2", "s3_ground", "s9_ground"])
def test_ground_sphere_grazing_rays(scenes, name):
    """The rays that leave the radius-999 sphere with a spurious f32 root above t = 0.001: the reference's box test
    rejects them, and so must the rebuilt tree, with the sphere tested per ray as one of two (s2), of three (s3_ground,
    the generic loop) and next to eight spheres inside the tree (s9_ground; before large spheres stayed per ray there,
    the tree returned the spurious root for all of these rays)."""
    cs = scenes[name]
    e = cs.export("rebuilt", width=4)
    prims, ranks = e["prims"].reshape(-1, 3, 4), _prim_ranks(e["prims"])
    for cam in custom_scene.ground_graze_cameras().values():
        o, d = custom_scene.camera_rays(cam, 2, 2, 1)
        t_ref, _ = cs.oracle.trace(o, d)
        t_new, r_new = _trace_wide_rays(e, prims, ranks, o, d)
        bt, _ = _best(_prim_t(prims, o[0], d[0], np.float32(np.inf)), ranks)
        assert 0.001 <= bt < 0.002, "the f32 root exists"
        assert (t_ref == -1).all() and (r_new == -1).all(), (t_ref, t_new, r_new)


def test_more_than_eight_large_spheres_are_refused(scenes):
    """Large spheres are tested per ray, at most eight of them: nine among ten is an error with a message, for the
    export and the device scene alike (they share the build); width 2 and eight large ones among ten build."""
    big = [((3.0 * k, -5.0, 0.0), 1.0 + 0.25 * k, k % 5) for k in range(9)]
    small = [((0.0, 0.0, 0.0), 0.05, 0)]
    bad = custom_scene.CustomScene([], big + small, synth.SPHERE_MATS)
    with pytest.raises(crt_amd.CrtError, match="more than 8 spheres of radius >= 1"):
        bad.export("rebuilt", width=4)
    assert bad.export("rebuilt", width=2, leaf_size=4)["n_ray_spheres"] == 0
    ok = custom_scene.CustomScene([], big[:8] + small + small, synth.SPHERE_MATS)
    e = ok.export("rebuilt", width=4)
    assert e["n_ray_spheres"] == 8 and e["sphere_first"] == 2


def test_no_objects_is_refused(scenes):
    """n_objects == 0 through the host-only export, both paths (tests/test_gpu_synth.py pins crt_scene_create_ex)."""
    import ctypes as C
    from crt_amd import _lib
    for keep_nodes, message in ((False, "no BVH nodes"), (True, "scene leaf object out of range")):
        d = _lib.SceneDesc()
        C.memmove(C.byref(d), C.byref(scenes["s1"].desc), C.sizeof(d))
        d.n_objects = 0
        if not keep_nodes:
            d.n_scene_nodes = 0
        for mode in ("reference", "rebuilt"):
            with pytest.raises(crt_amd.CrtError, match=message):
                crt_amd.export_desc(d, mode)
