"""Render kernels on synthetic meshes, sphere counts 0-40 and axis rays, against the CPU oracle (GPU).

The asset scenes never produce these: sphere counts other than two (the generic per-ray sphere loop for 1 and 3-8
spheres, spheres inside the 4-wide tree's leaves above eight, the empty 4-wide root of a sphere-only scene), exactly
coincident triangles (the tie rule), zero-area triangles, a mesh of one triangle, twelve meshes, leaf sizes 1 and 16,
coordinates round 1000, and primary rays with exactly zero direction components.  Scenes come from
tests/helpers/synth_scenes.py and reach the library through the C ABI (tests/helpers/custom_scene.py).

* reference-BVH path (variants 0, 1, 2, 3, 10): fp32 sums, RGBA8 and the four work counters equal the oracle's;
* rebuilt trees (4-wide default, leaf 1, leaf 16, GPU build, spatial splits; width 2 leaf 16): per ray against the
  reference tree (crt_scene_compare_dump): no t mismatch, at most MAX_DIFFERING_SHARE of the rays on another primitive,
  and every such ray confirmed by brute force over the exported primitives; the frame within RMS_TOL of the oracle;
  variants 7 and 8 bit-identical to variant 4;
* the control (the standard sphere pair through the helper) and the anchor (cornell_bunny through the helper) are
  bit-identical to HostScene.upload, so a helper bug cannot pass for a kernel result.
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
from crt_amd import _lib, assets

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import custom_scene  # noqa: E402
from bvh_emulation import _best, _prim_ranks, _prim_t, _trace_wide_rays  # noqa: E402
from custom_scene import FAMILIES, ONLY, WORLDS, CustomScene, camera_desc, world_offset  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
CHECKED = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
RMS_TOL = 1e-4
MAX_DIFFERING_SHARE = 1e-3        # the same cap as tests/test_synth_scenes.py
MAX_DUMP = 4096
NT = 16                           # oracle threads
ALL = FAMILIES + WORLDS + ONLY
TREES = {"w4": dict(width=4), "w4_leaf1": dict(width=4, leaf_size=1), "w4_leaf16": dict(width=4, leaf_size=16),
         "w4_gpu": dict(width=4, gpu_build=True), "w4_sbvh": dict(width=4, spatial_splits=True),
         "w2_leaf16": dict(width=2, leaf_size=16)}


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    return custom_scene.synth_worlds(custom_scene.family_files(tmp_path_factory.mktemp("synth")))


@pytest.fixture(scope="module")
def ref_scenes(worlds):
    return {k: cs.upload(0) for k, cs in worlds.items()}


def _camera(name, spp):
    cam = crt_amd.camera(spp)
    off = world_offset(name)
    for k in range(3):
        cam.origin[k] = float(np.float32(cam.origin[k]) + off[k])
        cam.lower_left[k] = float(np.float32(cam.lower_left[k]) + off[k])
    return cam


def _render(scene, cam, w, h, spp, variant, count_work=False, stack_lds=None):
    r = crt_amd.Renderer(w, h)
    r.set_kernel_variant(variant)
    if stack_lds is not None:
        r.set_stack_lds(stack_lds)
    r.set_camera(cam)
    r.init_rand(41)
    r.render(scene, spp, 20, count_work=count_work)
    r.resolve(crt_amd.pixel_sample_scale(spp))
    r.synchronize()                 # reports a device-side error of the render (stack overflow, checked build)
    return r


def _exact(lin, rgba, o_sum, o_rgba):
    diff = np.argwhere(lin.view(np.uint32) != o_sum.view(np.uint32))
    assert len(diff) == 0, f"{len(diff)} fp32 words differ, first at {diff[:5].tolist()}"
    assert np.array_equal(rgba, o_rgba)


_oracle_cache = {}


def _oracle(worlds, name, cam, w, h, spp, key="bench"):
    k = (name, key, w, h, spp)
    if k not in _oracle_cache:
        _oracle_cache[k] = worlds[name].oracle.render(crt_amd.camera_floats(cam), w, h, spp, 20, nthreads=NT)
    return _oracle_cache[k]


def _check_reference(worlds, ref_scenes, name, cam, w, h, spp, variant, key="bench"):
    o_sum, o_rgba, o_cnt = _oracle(worlds, name, cam, w, h, spp, key)
    r = _render(ref_scenes[name], cam, w, h, spp, variant)
    _exact(r.linear(), r.rgba8(), o_sum, o_rgba)
    cnt = _render(ref_scenes[name], cam, w, h, spp, variant, count_work=True).counters()
    for k in ("rays", "box_tests", "tri_tests", "sphere_tests"):
        assert cnt[k] == o_cnt[k], (k, cnt[k], o_cnt[k])


# ------------------------------------------------------------------------------------------ a. reference BVH
@pytest.mark.parametrize("variant", [0, 3, 10])
@pytest.mark.parametrize("name", ALL)
def test_reference_bvh_bit_exact(worlds, ref_scenes, name, variant):
    _check_reference(worlds, ref_scenes, name, _camera(name, 16), 64, 36, 16, variant)


@pytest.mark.parametrize("variant", [1, 2])
def test_reference_bvh_bit_exact_leaf_round_variants(worlds, ref_scenes, variant):
    _check_reference(worlds, ref_scenes, "ties", _camera("ties", 16), 64, 36, 16, variant)


def test_reference_bvh_partial_tiles(worlds, ref_scenes):
    _check_reference(worlds, ref_scenes, "soup", _camera("soup", 16), 100, 37, 16, 10)


# ------------------------------------------------------------------------------------------ e. control and anchor
@pytest.mark.parametrize("name,asset", [("s2", "cornell"), (None, "cornell_bunny")])
def test_helper_path_is_bit_identical_to_host_upload(worlds, ref_scenes, name, asset):
    """The standard pair through the helper (s2, the control) and the unchanged cornell_bunny scene (the anchor) against
    HostScene.upload: reference and rebuilt frames, RGBA8, RNG state and ray counts."""
    hs = crt_amd.HostScene(assets.scene_files(asset))
    cs = worlds[name] if name else CustomScene(assets.scene_files(asset))
    cam = crt_amd.camera(16)
    for opts, variant in ((dict(), 3), (dict(bvh="rebuilt", width=4), 4)):
        a = _render(hs.upload(0, **opts), cam, 64, 36, 16, variant)
        b = _render(cs.upload(0, **opts), cam, 64, 36, 16, variant)
        _exact(b.linear(), b.rgba8(), a.linear(), a.rgba8())
        assert np.array_equal(a.rng_state(), b.rng_state()) and a.counters()["rays"] == b.counters()["rays"]
    if asset == "cornell_bunny":
        g = np.load(Path(__file__).resolve().parent / "golden" / "cornell_bunny_64x36_16spp.npz")
        b = _render(cs.upload(0), cam, 64, 36, 16, 3)
        _exact(b.linear(), b.rgba8(), g["sum"], g["rgba"])


def test_scene_without_objects_is_refused(worlds):
    """n_objects == 0: CRT_ERR_INVALID_ARGUMENT, no scene, a message (crt_hip.h).  Two paths: with no scene BVH node
    either, the node count is refused; with the scene nodes left in place, the leaf that names object 0."""
    for keep_nodes, message in ((False, b"no BVH nodes"), (True, b"scene leaf object out of range")):
        d = _lib.SceneDesc()
        C.memmove(C.byref(d), C.byref(worlds["s1"].desc), C.sizeof(d))
        d.n_objects = 0
        if not keep_nodes:
            d.n_scene_nodes = 0
        for opts in (crt_amd.scene_options("reference"), crt_amd.scene_options("rebuilt", width=4)):
            h = C.c_void_p()
            rc = _lib.hip().crt_scene_create_ex(C.byref(d), 0, C.byref(opts), C.byref(h))
            assert rc == -1 and not h.value                  # CRT_ERR_INVALID_ARGUMENT
            assert message in _lib.hip().crt_last_error()


# ------------------------------------------------------------------------------------------ c. rebuilt trees
def _check_rebuilt(worlds, ref_scenes, name, tree, cam, w, h, spp, key="bench"):
    cs = worlds[name]
    opts = TREES[tree]
    fast = cs.upload(0, bvh="rebuilt", **opts)
    r = crt_amd.Renderer(w, h)
    r.set_camera(cam)
    r.init_rand(41)
    res, dump = r.compare_dump(ref_scenes[name], fast, spp, 20, max_dump=MAX_DUMP)
    r.synchronize()
    share = res["rank_mismatch"] / max(1, res["rays"])
    print(f"\n{name}/{tree}: {res['rays']} rays, {res['rank_mismatch']} on another primitive (share {share:.2e}), "
          f"{res['t_mismatch']} t mismatches")
    assert res["rays"] >= w * h * spp
    assert res["t_mismatch"] == 0
    assert res["rank_mismatch"] <= MAX_DIFFERING_SHARE * res["rays"] and res["rank_mismatch"] <= MAX_DUMP, res
    if len(dump):
        e = cs.export("rebuilt", **opts)
        prims, ranks = e["prims"].reshape(-1, 3, 4), _prim_ranks(e["prims"])
        for row in dump:
            o, d = row[0:3].copy(), row[3:6].copy()
            rank_a, rank_b = (int(x) for x in row[6:8].view(np.int32))
            bt, br = _best(_prim_t(prims, o, d, np.float32(np.inf)), ranks)
            assert br == rank_b, (row, bt, br)
            if br >= 0:
                assert np.float32(bt).view(np.uint32) == row[9].view(np.uint32), (row, bt, br)
                assert rank_a < 0 or row[8] > row[9], ("the reference's hit is not farther", row)
    variant = 4 if opts["width"] == 4 else 3
    f = _render(fast, cam, w, h, spp, variant)
    o_sum, _, o_cnt = _oracle(worlds, name, cam, w, h, spp, key)
    rms = np.sqrt(np.mean(((f.linear() - o_sum) / spp).astype(np.float64) ** 2, axis=(0, 1)))
    assert (rms <= RMS_TOL).all(), f"per-channel RMS {rms}"
    return fast, f


@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("name", ALL)
def test_rebuilt_tree(worlds, ref_scenes, name, tree):
    _check_rebuilt(worlds, ref_scenes, name, tree, _camera(name, 16), 64, 36, 16)


WIDE_TREES = [t for t in TREES if TREES[t]["width"] == 4]


def _variants_7_and_8_equal_4(fast, cam, w, h, spp):
    """Sums, RGBA8, RNG state and ray count of the benchmarked kernels against variant 4 on the same tree."""
    base = _render(fast, cam, w, h, spp, 4)
    for variant in (7, 8):
        r = _render(fast, cam, w, h, spp, variant)
        _exact(r.linear(), r.rgba8(), base.linear(), base.rgba8())
        assert np.array_equal(r.rng_state(), base.rng_state())
        assert r.counters()["rays"] == base.counters()["rays"]


@pytest.mark.parametrize("tree", WIDE_TREES)
@pytest.mark.parametrize("name", ALL)
def test_rebuilt_variants_7_and_8_equal_variant_4(worlds, name, tree):
    """96x54 at 64 spp, so that variant 8 runs its cost probe, on every 4-wide tree: leaves of 1 and of up to 16
    primitives, spheres in the leaves, the GPU-built and the spatial-split tree all go through the benchmarked
    kernels' leaf rounds."""
    fast = worlds[name].upload(0, bvh="rebuilt", **TREES[tree])
    _variants_7_and_8_equal_4(fast, _camera(name, 64), 96, 54, 64)


def test_one_entry_lds_stack_equals_default(worlds):
    """many_meshes has the deepest tree here: with one LDS entry every further push goes to the HBM overflow region."""
    fast = worlds["many_meshes"].upload(0, bvh="rebuilt", width=4, leaf_size=1)
    assert fast.stats()["stack_bound"] > 2
    cam = _camera("many_meshes", 16)
    for variant in (4, 7):
        a = _render(fast, cam, 64, 36, 16, variant)
        b = _render(fast, cam, 64, 36, 16, variant, stack_lds=1)
        _exact(b.linear(), b.rgba8(), a.linear(), a.rgba8())
        assert np.array_equal(a.rng_state(), b.rng_state())


@pytest.mark.parametrize("name", ["s1", "s2", "s3", "s3_ground", "s8", "before", "twins", "only3", "soup"])
def test_per_ray_sphere_tests_counter(worlds, name):
    """Every ray tests every per-ray sphere once (the generic loop for 1 and 3-8, the pair path for 2)."""
    cs = worlds[name]
    fast = cs.upload(0, bvh="rebuilt", width=4)
    n = cs.export("rebuilt", width=4)["n_ray_spheres"]
    assert n == cs.n_spheres > 0
    cnt = _render(fast, _camera(name, 16), 64, 36, 16, 4, count_work=True).counters()
    assert cnt["rays"] >= 64 * 36 * 16 and cnt["sphere_tests"] == cnt["rays"] * n


# ------------------------------------------------------------------------------------------ d. axis rays
@pytest.fixture(scope="module")
def axis_cameras(worlds):
    return custom_scene.axis_cameras(custom_scene.planar_plane_y(worlds["planar"]),
                                     custom_scene.planar_straight_xy(worlds["planar"]))


@pytest.mark.parametrize("cam_name", ["dy_plus0", "dy_minus0", "straight", "in_plane"])
@pytest.mark.parametrize("name", ["s2", "planar"])
def test_axis_rays(worlds, ref_scenes, axis_cameras, name, cam_name):
    cam = axis_cameras[cam_name]
    if cam_name == "dy_minus0":         # the zero lens offset's sign decides: -0 on three samples in four
        dy = custom_scene.camera_rays(cam, 8, 8, 64)[1][:, 1]
        assert (dy == 0).all() and np.signbit(dy).mean() >= 0.7 and not np.signbit(dy).all()
    for variant in (0, 3, 10):
        _check_reference(worlds, ref_scenes, name, cam, 8, 8, 64, variant, key=cam_name)
    for tree in TREES:
        fast, _ = _check_rebuilt(worlds, ref_scenes, name, tree, cam, 8, 8, 64, key=cam_name)
        if TREES[tree]["width"] == 4:
            _variants_7_and_8_equal_4(fast, cam, 8, 8, 64)


@pytest.mark.parametrize("name", ["soup", "many_meshes"])
def test_axis_ray_visits_only_the_boxes_it_enters(worlds, name):
    """d = (0, 0, -1) from a point whose ray misses every primitive: with nothing to prune by, the child boxes a
    counting render tests are exactly those of the nodes whose boxes the ray enters, whatever the order.  The count
    comes from the restated traversal (checked against the float64 slab test in tests/test_synth_scenes.py).  A slab
    test that loses a zero component's axis (an unclamped reciprocal: inf - inf = NaN, which min/max drop) still finds
    every hit, but walks into boxes the ray never enters; only this count shows it."""
    cs = worlds[name]
    e = cs.export("rebuilt", width=4)
    prims, ranks = e["prims"].reshape(-1, 3, 4), _prim_ranks(e["prims"])
    grid = np.stack(np.meshgrid(np.arange(-9, 10), np.arange(-9, 10)), -1).reshape(-1, 2) / np.float32(37.0)
    o = np.concatenate([grid, np.full((len(grid), 1), 0.25)], 1).astype(np.float32)
    d = np.tile(np.array([0, 0, -1], np.float32), (len(o), 1))
    boxes = np.zeros(len(o), np.int64)
    _, rank = _trace_wide_rays(e, prims, ranks, o, d, box_tests=boxes)
    miss = np.nonzero(rank < 0)[0]
    assert len(miss) > 0
    k = miss[np.argmax(boxes[miss])]                   # the missing ray that walks deepest into the tree
    assert boxes[k] >= 12
    x, y = float(o[k, 0]), float(o[k, 1])
    cam = camera_desc((x, y, 0.25), (x, y, -0.75), (0, 0, 0), (0, 0, 0), spp=1)
    fast = cs.upload(0, bvh="rebuilt", width=4)
    for variant in (4, 7):
        r = crt_amd.Renderer(8, 8)
        r.set_kernel_variant(variant)
        r.set_camera(cam)
        r.init_rand(41)
        r.render(fast, 1, 1, count_work=True)
        r.synchronize()
        cnt = r.counters()
        assert cnt["rays"] == 64 and cnt["box_tests"] == 64 * int(boxes[k]), (cnt, int(boxes[k]))


# ------------------------------------------------------------------------------------------ large spheres
@pytest.mark.parametrize("cam_name", ["graze0", "graze1", "graze2"])
@pytest.mark.parametrize("name", ["s2", "s3_ground", "s9_ground"])
def test_ground_sphere_grazing_rays(worlds, ref_scenes, name, cam_name):
    """Every primary ray leaves the radius-999 sphere with a spurious f32 root above t = 0.001 that the reference's box
    test never lets Sphere::hit produce (custom_scene.ground_graze_cameras).  The sphere is one of two per-ray spheres
    (s2, the pair path), of three (s3_ground, the generic loop), and the one per-ray sphere next to eight in the tree
    (s9_ground).  A tree without the box replay returns the root for every primary ray."""
    cam = custom_scene.ground_graze_cameras()[cam_name]
    for variant in (0, 3, 10):
        _check_reference(worlds, ref_scenes, name, cam, 8, 8, 64, variant, key=cam_name)
    _check_rebuilt(worlds, ref_scenes, name, "w4", cam, 8, 8, 64, key=cam_name)
    if name == "s9_ground":
        cnt = _render(worlds[name].upload(0, bvh="rebuilt", width=4), cam, 8, 8, 64, 4, count_work=True).counters()
        assert cnt["sphere_tests"] >= cnt["rays"]          # the ground sphere per ray, the others in the leaves


@pytest.mark.parametrize("cam_name", ["graze0", "graze1", "graze2"])
def test_ground_sphere_grazing_rays_width_2_known_gap(worlds, ref_scenes, cam_name):
    """OPEN GAP, pinned so that it is measured and cannot change unnoticed: the threaded width-2 layouts (variants 0-3)
    keep every sphere in the tree and replay no reference box, so on these rays the standard scene's radius-999 sphere is
    hit at its spurious f32 root where the reference sees the sky.  Every primary ray differs (64 pixels x 64 samples);
    each differing ray is one the reference misses and brute force over the exported primitives confirms.  On ordinary
    frames the rate is the 3 in 98 million of DESIGN.md section 2b.  Closing it needs the box replay in the variant 0-3
    kernels; when that lands, this test is to become the width-4 assertion (no differing ray)."""
    cs = worlds["s2"]
    opts = TREES["w2_leaf16"]
    r = crt_amd.Renderer(8, 8)
    r.set_camera(custom_scene.ground_graze_cameras()[cam_name])
    r.init_rand(41)
    res, dump = r.compare_dump(ref_scenes["s2"], cs.upload(0, bvh="rebuilt", **opts), 64, 20, max_dump=MAX_DUMP)
    r.synchronize()
    print(f"\ns2/w2_leaf16/{cam_name}: {res}")
    assert res["t_mismatch"] == 0 and res["rank_mismatch"] == res["a_miss"] == 64 * 64 and res["b_miss"] == 0
    e = cs.export("rebuilt", **opts)
    prims, ranks = e["prims"].reshape(-1, 3, 4), _prim_ranks(e["prims"])
    for row in dump[:64]:
        bt, br = _best(_prim_t(prims, row[0:3].copy(), row[3:6].copy(), np.float32(np.inf)), ranks)
        assert br == int(row[7:8].view(np.int32)[0]) and np.float32(bt).view(np.uint32) == row[9].view(np.uint32)
        assert 0.001 <= bt < 0.002


def test_more_than_eight_large_spheres_are_refused():
    import synth_scenes as synth
    big = [((3.0 * k, -5.0, 0.0), 1.0 + 0.25 * k, k % 5) for k in range(9)]
    bad = CustomScene([], big + [((0.0, 0.0, 0.0), 0.05, 0)], synth.SPHERE_MATS)
    with pytest.raises(crt_amd.CrtError, match="more than 8 spheres of radius >= 1"):
        bad.upload(0, bvh="rebuilt", width=4)
    bad.upload(0)                                          # the reference BVH takes the same scene


# ------------------------------------------------------------------------------------------ checked build
CHILD = r"""
import json, sys
from pathlib import Path
import numpy as np
repo = Path(sys.argv[1])
sys.path[:0] = [str(repo / "raytracer-cuda_amd"), str(repo / "oracle"), str(repo / "tests" / "helpers")]
import crt_amd
import custom_scene
from crt_amd import _lib
worlds = custom_scene.synth_worlds(custom_scene.family_files(sys.argv[2]))
out = {"flags": int(_lib.hip().crt_build_flags()), "frames": {}}
for name in json.loads(sys.argv[4]):
    sc = worlds[name].upload(0, bvh="rebuilt", width=4)
    for var in (4, 8):
        r = crt_amd.Renderer(96, 54)
        r.set_kernel_variant(var)
        r.set_camera(crt_amd.camera(64))
        r.init_rand(41)
        r.render(sc, 64, 20)
        r.synchronize()
        out["frames"][f"{name}/{var}"] = r.linear().view(np.uint32).tolist()
json.dump(out, open(sys.argv[3], "w"))
"""


def test_checked_build_reports_nothing_and_matches(worlds, tmp_path):
    """Spheres inside the tree's leaves (s9_ground) and coincident triangles (ties) through the checked library, in a
    child process (one HIP library per process): no device-side report, the fast library's frames."""
    names = ["s9_ground", "ties"]
    assert CHECKED.exists() and _lib.hip().crt_build_flags() == 0
    res = tmp_path / "checked.json"
    (tmp_path / "scenes").mkdir()
    env = dict(os.environ, CRT_HIP_LIB=str(CHECKED))
    p = subprocess.run([sys.executable, "-c", CHILD, str(REPO), str(tmp_path / "scenes"), str(res), json.dumps(names)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(res.read_text())
    assert got["flags"] == _lib.BUILD_CHECKED
    for name in names:
        fast = worlds[name].upload(0, bvh="rebuilt", width=4)
        for var in (4, 8):
            r = _render(fast, crt_amd.camera(64), 96, 54, 64, var)
            chk = np.array(got["frames"][f"{name}/{var}"], np.uint32).reshape(54, 96, 3)
            assert np.array_equal(chk, r.linear().view(np.uint32)), f"checked build differs: {name} variant {var}"
