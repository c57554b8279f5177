"""A crt_scene_desc with the caller's spheres, materials and object order, and the oracle scene of the same world.

SceneManager always adds the same two spheres after the meshes; the C ABI takes any list.  CustomScene copies
HostScene.desc() (the product's loader and mesh BVH builds) and replaces the sphere, object, material and scene-node
arrays; the scene-level BVH is taken from the oracle's build of the same object list (tests/test_host_parity.py pins
the two builders against each other).  The oracle side is pyoracle.OracleScene(loaded, spheres, order).

translate=(x, y, z) moves every vertex of both loaders' output (they normalise every scene to the origin, so a far
scene cannot come out of an OBJ file) and rebuilds the mesh BVHs with the product's host builder.
"""
import ctypes as C

import numpy as np

import crt_amd
import objload
import pyoracle
from crt_amd import _lib

from bvh_emulation import _prim_ranks

MESH, SPHERE = 0, 1                      # crt_object_kind


class SphereDesc(C.Structure):           # crt_hip.h crt_sphere_desc
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("material", C.c_int32)]


class ObjectDesc(C.Structure):           # crt_hip.h crt_object_desc
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32)]


def mat_row(kind, albedo=(0, 0, 0), emission=(0, 0, 0), roughness=0.0, ior=1.0):
    """One material row (type, albedo3, emission3, roughness, ior); kind: 0 lambertian, 1 metal, 2 dielectric, 3 light."""
    return [float(kind), *albedo, *emission, roughness, ior]


# SceneManager::createWorld / createRandomWorld (CUDAKernels.h:56-84): the ground sphere and the small metal one
STANDARD_SPHERES = [((0.0, -1000.0, 0.0), 999.0, 0), ((np.float32(0.2), np.float32(0.2), 0.0), 0.05, 1)]
STANDARD_MATS = [mat_row(0, (0.5, 0.5, 0.5)), mat_row(1, (0.7, 0.6, 0.5), roughness=0.0)]


class CustomScene:
    """files: OBJ list (may be empty); spheres: [(centre3, radius, index into sphere_mats)]; sphere_mats: material
    rows; order: [(kind, index)] (default: meshes, then spheres)."""

    def __init__(self, files, spheres=STANDARD_SPHERES, sphere_mats=STANDARD_MATS, order=None, translate=None):
        files = [str(f) for f in files]
        self.loaded = objload.load_scene(files)
        self.hs = crt_amd.HostScene(files) if files else None
        n_loader_mats = len(self.loaded.matdata)
        n_meshes = len(self.loaded.mesh_info)
        self._keep = []
        d = self.hs.desc() if self.hs else _lib.SceneDesc()
        assert (d.n_materials - 2 if self.hs else 0) == n_loader_mats
        if translate is not None:
            self._translate(d, np.asarray(translate, np.float32))
        sph5 = np.array([[*c, r, n_loader_mats + m] for c, r, m in spheres], np.float32).reshape(-1, 5)
        smat = np.array(sphere_mats, np.float32).reshape(-1, 9)
        if order is None:
            order = [(MESH, i) for i in range(n_meshes)] + [(SPHERE, i) for i in range(len(sph5))]
        self.order = [(int(k), int(i)) for k, i in order]
        self.n_spheres = len(sph5)
        self.oracle = pyoracle.OracleScene(self.loaded, (sph5, smat), self.order)

        sa = (SphereDesc * max(1, len(sph5)))()
        for s, row in zip(sa, sph5):
            s.center[:] = row[:3].tolist()
            s.radius = float(row[3])
            s.material = int(row[4])
        oa = (ObjectDesc * len(self.order))(*[ObjectDesc(k, i) for k, i in self.order])
        ma = (_lib.MaterialDesc * (n_loader_mats + len(smat)))()
        if n_loader_mats:
            C.memmove(ma, d.materials, n_loader_mats * C.sizeof(_lib.MaterialDesc))
        for m, row in zip(list(ma)[n_loader_mats:], smat):
            m.type = int(row[0])
            m.albedo[:] = row[1:4].tolist()
            m.emission[:] = row[4:7].tolist()
            m.roughness, m.ior = float(row[7]), float(row[8])
        boxes, ints = self.oracle.nodes(-1)
        self.scene_nodes = (boxes, ints)
        na = (_lib.BvhNodeDesc * len(ints))()
        for nd, b, i in zip(na, boxes, ints):
            nd.bmin[:] = b[:3].tolist()
            nd.bmax[:] = b[3:].tolist()
            nd.left, nd.right, nd.obj_index, nd.obj_count, nd.is_leaf = (int(x) for x in i)
        d.spheres, d.n_spheres = C.cast(sa, C.c_void_p), len(sph5)
        d.objects, d.n_objects = C.cast(oa, C.c_void_p), len(self.order)
        d.materials, d.n_materials = C.cast(ma, C.c_void_p), len(ma)
        d.scene_nodes, d.n_scene_nodes = C.cast(na, C.c_void_p), len(na)
        self._keep += [sa, oa, ma, na]
        self.desc = d
        self._ref_export = None

    def _translate(self, d, t):
        """Both sides' vertices + t; mesh BVHs, permutations and boxes rebuilt by the product's host builder."""
        pos, idx, fm, info, _ = self.hs.loader_arrays()
        pos = (pos + t).astype(np.float32)
        self.loaded.positions = (self.loaded.positions + t).astype(np.float32)
        assert np.array_equal(pos, self.loaded.positions)
        idx, fm = idx.copy(), fm.copy()
        meshes = (_lib.MeshDesc * d.n_meshes)()
        C.memmove(meshes, d.meshes, C.sizeof(meshes))
        for m, (vo, vc, io, ic, fo, _) in zip(meshes, info.astype(np.int64)):
            nodes, pidx, pfm, box, _ = crt_amd.build_mesh_bvh(pos[vo:vo + vc], idx[io:io + ic], fm[fo:fo + ic // 3])
            idx[io:io + ic], fm[fo:fo + ic // 3] = pidx, pfm
            nodes = np.ascontiguousarray(nodes)
            m.nodes, m.node_count = nodes.ctypes.data, len(nodes)
            m.aabb[:] = box.tolist()
            self._keep.append(nodes)
        d.positions, d.indices, d.face_materials = pos.ctypes.data, idx.ctypes.data, fm.ctypes.data
        d.meshes = C.cast(meshes, C.c_void_p)
        self._keep += [pos, idx, fm, meshes]

    # ---- product side
    def export(self, bvh="reference", **options):
        return crt_amd.export_desc(self.desc, bvh, **options)

    def upload(self, device=0, bvh="reference", **options):
        return crt_amd.create_scene(self.desc, device, bvh, **options)

    # ---- oracle primitive ids -> reference ranks
    def ref_export(self):
        if self._ref_export is None:
            self._ref_export = self.export("reference")
        return self._ref_export

    def oracle_ranks(self, prim):
        """Reference DFS rank of OracleScene.trace's primitive ids.  The reference export holds the meshes' triangles
        in mesh order (after the build permutation), then the spheres in the order the scene BVH's leaves are
        flattened (depth first, left child first)."""
        ranks = _prim_ranks(self.ref_export()["prims"])
        info = self.loaded.mesh_info.astype(np.int64)
        base = np.concatenate([[0], np.cumsum(info[:, 3] // 3)]) if len(info) else np.zeros(1, np.int64)
        _, ints = self.scene_nodes
        emit, todo = [], [0]
        while todo:
            left, right, obj, _, leaf = ints[todo.pop()]
            if leaf:
                if self.order[obj][0] == SPHERE:
                    emit.append(self.order[obj][1])
            else:
                todo += [right, left]
        slot = np.zeros(max(1, self.n_spheres), np.int64)
        slot[emit] = np.arange(len(emit))
        prim = np.asarray(prim, np.int64)
        mesh = prim[:, 0] >= 0
        at = np.where(mesh, base[np.maximum(prim[:, 0], 0)] + prim[:, 1], base[-1] + slot[np.maximum(-1 - prim[:, 0], 0)])
        return ranks[at]


def camera_desc(origin, lower_left, horizontal, vertical, right=(1, 0, 0), up=(0, 1, 0), lens_radius=0.0, spp=1):
    """A crt_camera_desc by hand (Camera::getRay reads exactly these, Camera.cuh:32-44)."""
    d = _lib.CameraDesc()
    for name, v in (("origin", origin), ("lower_left", lower_left), ("horizontal", horizontal),
                    ("vertical", vertical), ("right", right), ("up", up)):
        getattr(d, name)[:] = [float(np.float32(x)) for x in v]
    d.lens_radius = float(lens_radius)
    d.samples_per_pixel = int(spp)
    d.pixel_sample_scale = crt_amd.pixel_sample_scale(spp)
    return d


FAMILIES = ("soup", "ties", "degenerate", "planar", "many_meshes", "far")
WORLDS = ("s0", "s1", "s2", "s3", "s3_ground", "s8", "s9_ground", "s40", "before", "interleaved", "twins", "tangent")
ONLY = ("only3", "only12")


def family_files(directory):
    import synth_scenes as synth
    return {k: getattr(synth, k)(str(directory)) for k in FAMILIES}


def synth_worlds(files):
    """name -> CustomScene: the generated families (family_files) with the standard sphere pair, the sphere worlds
    over the Cornell mesh (two of its files where the order interleaves two meshes), and the sphere-only scenes."""
    import synth_scenes as synth
    from crt_amd import assets
    out = {k: CustomScene(f, translate=synth.FAR_OFFSET if k == "far" else None) for k, f in files.items()}
    one, two = assets.scene_files("cornell"), assets.scene_files("cornell_bunny")
    floor = float(objload.load_scene(one).positions[:, 1].min())
    for k, (spheres, order, two_meshes) in synth.sphere_worlds(floor).items():
        out[k] = CustomScene(two if two_meshes else one, spheres, synth.SPHERE_MATS, order)
    out["s2"] = CustomScene(one)        # the control: SceneManager's own pair, through this helper
    for k, spheres in synth.SPHERES_ONLY.items():
        out[k] = CustomScene([], spheres, synth.SPHERE_MATS)
    assert set(out) == set(FAMILIES + WORLDS + ONLY)
    return out


# worlds for the split-by-split checks of the SAH builders (tests/helpers/sah_model.py)
SAH_WORLDS = ("spheres9", "spheres17", "spheres40", "soup200_spheres12", "concentric", "concentric_soup",
              "concentric_tris", "grid8", "grid24")
# Triangle counts of the sized soups.  The GPU builder's constants are item counts: SAH_SMALL 16 / 17, SCAN_ITEMS 1024,
# SAH_CHUNK 4096 and twice that.  At width 4 a soup of n triangles is n items, at width 2 it is n + 2 (SizedSoup), so
# n - 2 stands next to every n.
SAH_SOUP_SIZES = (1, 2, 14, 15, 16, 17, 33, 1022, 1023, 1024, 1025)    # checked split by split (and host against GPU)
SAH_SOUP_SIZES_BIG = (4093, 4094, 4095, 4096, 4097, 8191, 8193, 20000)  # host against GPU only


class SizedSoup:
    """synth_scenes.sized_soup(n) through SceneManager itself (crt_amd.HostScene: the standard sphere pair).  At width
    4 the pair is tested per ray and the SAH builder sees exactly n items; at width 2 every sphere is an item: n + 2."""

    def __init__(self, directory, n):
        import synth_scenes as synth
        self.n = n
        self.hs = crt_amd.HostScene(synth.sized_soup(str(directory), n))
        self.desc = self.hs.desc()

    def export(self, bvh="reference", **options):
        return crt_amd.export_desc(self.desc, bvh, **options)


def sah_worlds(directory):
    """name -> CustomScene: sphere worlds of more than 8 spheres (all of them items of the tree, alone and among 200
    triangles), 20 concentric spheres (coincident box centres; alone and among 100 triangles), 20 concentric triangles
    and the rippled grids."""
    import synth_scenes as synth
    d = str(directory)
    out = {f"spheres{k}": CustomScene([], synth.random_spheres(k, seed=30 + k), synth.SPHERE_MATS) for k in (9, 17, 40)}
    out["soup200_spheres12"] = CustomScene(synth.sized_soup(d, 200), synth.random_spheres(12, seed=29), synth.SPHERE_MATS)
    out["concentric"] = CustomScene([], synth.concentric_spheres(), synth.SPHERE_MATS)
    out["concentric_soup"] = CustomScene(synth.sized_soup(d, 100), synth.concentric_spheres(), synth.SPHERE_MATS)
    out["concentric_tris"] = CustomScene(synth.concentric_triangles(d))
    out["grid8"] = CustomScene(synth.grid(d, 8))
    out["grid24"] = CustomScene(synth.grid(d, 24))
    assert set(out) == set(SAH_WORLDS)
    return out


def world_offset(name):
    import synth_scenes as synth
    return np.asarray(synth.FAR_OFFSET if name == "far" else (0, 0, 0), np.float32)


def _planar_triangles(planar):
    info = planar.loaded.mesh_info[0].astype(np.int64)
    idx = planar.loaded.indices[info[2]:info[2] + info[3]].reshape(-1, 3)[2:]      # all but the floor's two
    return planar.loaded.positions[info[0]:info[0] + info[1]][idx]                  # [n, 3 vertices, xyz]


def planar_plane_y(planar):
    """The y of the even 1/64 level (other than 0) of the planar scene that holds the most horizontal triangles: the
    plane of a stack of quads, which no vertical quad ends on (synth_scenes.planar)."""
    tri = _planar_triangles(planar)
    flat = tri[(tri[:, :, 1] == tri[:, :1, 1]).all(1)][:, 0, 1] * 64
    assert np.array_equal(flat, np.round(flat)) and (flat.astype(np.int64) % 2 == 0).all()
    levels, cnt = np.unique(flat[flat != 0], return_counts=True)
    assert cnt.max() >= 4, "at least two quads share the plane"
    return float(levels[np.argmax(cnt)]) / 64


def planar_straight_xy(planar):
    """A point inside the first triangle of the planar scene that faces z: a ray along (0, 0, -1) through it hits."""
    tri = _planar_triangles(planar)
    t = tri[(tri[:, :, 2] == tri[:, :1, 2]).all(1)][0]
    p = t[0] + np.float32(0.3) * (t[1] - t[0]) + np.float32(0.2) * (t[2] - t[0])     # off the grid: on no box face
    return float(p[0]), float(p[1])


def axis_cameras(plane_y, straight_xy):
    """name -> crt_camera_desc with lens radius 0, 64 spp (Camera::getRay: d = ((ll + u h) + v vert) - origin - offset)."""
    z = 0.0
    return {
        # vertical = 0 and lower_left.y == origin.y: d.y = y - y = +0 for every sample
        "dy_plus0": camera_desc((0, 0.0625, 0.3), (-0.5, 0.0625, -0.2), (1, 0, 0), (0, 0, 0), spp=64),
        # every y term -0 and origin.y = +0: d.y = (-0) - (+0) = -0 wherever the zero lens offset comes out +0
        "dy_minus0": camera_desc((0, z, 0.3), (-0.5, -z, -0.2), (1, -z, 0), (0, -z, 0), spp=64),
        # horizontal = vertical = 0: every sample of every pixel starts along (0, 0, -1)
        "straight": camera_desc((*straight_xy, 0.25), (*straight_xy, -0.75), (0, 0, 0), (0, 0, 0), spp=64),
        # origin on the exact y of a plane of the planar scene, d.y = 0: rays inside a zero-thickness box
        "in_plane": camera_desc((0, plane_y, 0.3), (-0.5, plane_y, -0.2), (1, 0, 0), (0, 0, 0), spp=64),
    }


def camera_rays(cam, w, h, samples, seed=41):
    """Camera::getRay for every pixel, `samples` consecutive draws of each pixel's generator: (o, d) float32 [n, 3]."""
    xy = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.int32)
    state = np.stack([pyoracle.rng_init(seed, i) for i in range(w * h)])
    cam19 = crt_amd.camera_floats(cam)
    rays = np.concatenate([pyoracle.kat_get_ray(cam19, w, h, xy, state) for _ in range(samples)])
    return rays[:, :3].copy(), rays[:, 3:].copy()


def ground_graze_cameras():
    """Cameras whose every primary ray is one of tests/golden/ground_sphere_rays.json: it starts a hair inside the
    radius-999 ground sphere and leaves it; Sphere::hit's f32 far root lands just above t = 0.001, but the reference's
    box test has already rejected the ray (tests/test_rebuilt_bvh.py::test_ground_sphere_box_culls_spurious_root).
    horizontal = vertical = 0, lens radius 0, lower_left = fl(o + d): d comes back as fl(fl(o + d) - o)."""
    import json
    from pathlib import Path
    g = json.loads((Path(__file__).resolve().parents[1] / "golden" / "ground_sphere_rays.json").read_text())
    out = {}
    for k, ray in enumerate(g["rays"]):
        o, d = np.array(ray["o"], np.float32), np.array(ray["d"], np.float32)
        out[f"graze{k}"] = camera_desc(o, (o + d).astype(np.float32), (0, 0, 0), (0, 0, 0), spp=64)
    return out
