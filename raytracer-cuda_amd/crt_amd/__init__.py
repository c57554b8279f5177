"""crt_amd — Python front-end of the MI355X path tracer.

Mirrors the reference's host API for the render path (CudaRayTracer/src):
  HostScene      ~ SceneManager host half (OBJ load, normalisation, BVH builds; C++ libcrt_host.so)
  Scene          ~ the device scene (SceneManager::getBVHNodes()/getWorld(); libcrt_hip.so)
  Renderer       ~ CUDARenderer (initialize / updateCamera / render / getImageData)
  camera(...)    ~ CRT::Camera(aspect, fov, position, target, up, aperture, focus)
All compute runs in the HIP library; nothing here computes pixels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import CameraDesc, CrtError, SceneDesc, SceneStats, WorkCounters, build, check, check_host

RENDER_ACCUMULATE = 1
RENDER_COUNT_WORK = 2

# The screenshot-reproducing bench pose: the reference's default pose
# (Raytracer.h:77-82, pos (0,4,4), target ignored) does not frame the box.
BENCH_CAMERA = dict(aspect=16.0 / 9.0, vfov=80.0, pos=(0.0, 0.0, 0.3), up=(0.0, 1.0, 0.0),
                    aperture=0.000001, focus=0.3, yaw=-90.0, pitch=0.0)


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def camera(spp: int = 1, aspect=16.0 / 9.0, vfov=80.0, pos=(0.0, 0.0, 0.3), up=(0.0, 1.0, 0.0),
           aperture=0.000001, focus=0.3, yaw=-90.0, pitch=0.0) -> CameraDesc:
    """CRT::Camera (Camera.cuh:18-30, :159-182) computed by the C++ host library."""
    d = CameraDesc()
    check_host(_lib.host().crth_camera(C.c_float(aspect), C.c_float(vfov), _p(np.asarray(pos, np.float32)),
                                       _p(np.asarray(up, np.float32)), C.c_float(aperture), C.c_float(focus),
                                       C.c_float(yaw), C.c_float(pitch), int(spp), C.byref(d)), "crth_camera")
    return d


def camera_floats(d: CameraDesc) -> np.ndarray:
    """19-float layout shared with the oracle (origin, llc, horizontal, vertical, right, up, lens_radius)."""
    return np.array(list(d.origin) + list(d.lower_left) + list(d.horizontal) + list(d.vertical) +
                    list(d.right) + list(d.up) + [d.lens_radius], dtype=np.float32)


class HostScene:
    """SceneManager host half: load OBJ files, normalise, build mesh + scene BVHs (C++)."""

    def __init__(self, obj_files, build_device=None):
        """build_device: None = mesh BVHs built by the host restatement; k = on GPU k (crt_build_mesh_bvh,
        same trees)."""
        files = [str(f) for f in obj_files]
        arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
        h = C.c_void_p()
        bd = -1 if build_device is None else int(build_device)
        check_host(_lib.host().crth_scene_load_ex(arr, len(files), bd, C.byref(h)), "crth_scene_load_ex")
        self.h = h
        self.files = files

    def device_build_ms(self) -> float:
        """Device time of the GPU mesh BVH builds of this load (0.0 for host builds)."""
        return float(_lib.host().crth_scene_build_ms(self.h))

    def __del__(self):
        # at interpreter exit the module's globals may already be gone (None); the process frees the scene then
        if getattr(self, "h", None) and _lib is not None:
            _lib.host().crth_scene_destroy(self.h)
            self.h = None

    def counts(self):
        c = np.zeros(5, np.int64)
        check_host(_lib.host().crth_scene_counts(self.h, _p(c)), "crth_scene_counts")
        return dict(n_meshes=int(c[0]), n_slots=int(c[1]), n_indices=int(c[2]), n_faces=int(c[3]),
                    n_materials=int(c[4]))

    def loader_arrays(self):
        c = self.counts()
        pos = np.zeros((c["n_slots"], 3), np.float32)
        idx = np.zeros(c["n_indices"], np.uint32)
        fm = np.zeros(c["n_faces"], np.int32)
        info = np.zeros((c["n_meshes"], 6), np.uint32)
        mats = np.zeros((c["n_materials"], 9), np.float32)
        check_host(_lib.host().crth_scene_loader_arrays(self.h, _p(pos), _p(idx), _p(fm), _p(info), _p(mats)),
                   "crth_scene_loader_arrays")
        return pos, idx, fm, info, mats

    def desc(self) -> SceneDesc:
        d = SceneDesc()
        check_host(_lib.host().crth_scene_desc(self.h, C.byref(d)), "crth_scene_desc")
        return d

    def mesh_bvh(self, i: int):
        """(boxes[n,6], ints[n,5] = left,right,obj_index,obj_count,is_leaf) in builder index order."""
        d = self.desc()
        meshes = C.cast(d.meshes, C.POINTER(_lib.MeshDesc))
        m = meshes[i]
        return _nodes_to_np(m.nodes, m.node_count), np.array(m.aabb, np.float32)

    def scene_bvh(self):
        d = self.desc()
        return _nodes_to_np(d.scene_nodes, d.n_scene_nodes)

    def permuted(self):
        d = self.desc()
        idx = np.ctypeslib.as_array(C.cast(d.indices, C.POINTER(C.c_uint32)), (d.n_indices,)).copy()
        fm = np.ctypeslib.as_array(C.cast(d.face_materials, C.POINTER(C.c_int32)), (d.n_faces,)).copy()
        return idx, fm

    def upload(self, device: int = 0, bvh: str = "reference", leaf_size: int = 0, layouts: int = 0,
               traversal_cost: float = 0.0, width: int = 0, gpu_build: bool = False, stack_cap: int = 0,
               spatial_splits: bool = False, spatial_alpha: float = 0.0, spatial_max_dup: float = 0.0) -> "Scene":
        """Device scene.  bvh="reference": the reference's BVHs, bit-exact (crth_scene_upload);
        bvh="rebuilt": binned-SAH BVH with the reference's hit rule (crt_scene_create_ex)."""
        h = C.c_void_p()
        if (bvh == "reference" and not leaf_size and not layouts and not traversal_cost and not width and not gpu_build
                and not stack_cap and not spatial_splits):
            check_host(_lib.host().crth_scene_upload(self.h, int(device), C.byref(h)), "crth_scene_upload")
            return Scene(h, device)
        o = scene_options(bvh, leaf_size, layouts, traversal_cost, width, gpu_build, stack_cap, spatial_splits,
                          spatial_alpha, spatial_max_dup)
        d = self.desc()
        check(_lib.hip().crt_scene_create_ex(C.byref(d), int(device), C.byref(o), C.byref(h)), "crt_scene_create_ex")
        return Scene(h, device)

    def export(self, bvh: str = "reference", **options) -> dict:
        """The device arrays crt_scene_create_ex would upload (host only, crt_scene_export)."""
        return export_desc(self.desc(), bvh, **options)


    def identity(self, bvh: str = "reference", **options) -> np.ndarray:
        """The per-rank identity table of the ray queries, int32 [ranks, 3] = (object, primitive, material) (host only,
        crt_scene_export_identity); the same for every bvh mode."""
        return identity_desc(self.desc(), bvh, **options)


def identity_desc(d: SceneDesc, bvh: str = "reference", **options) -> np.ndarray:
    """crt_scene_export_identity of any scene description."""
    o = scene_options(bvh, **options)
    n = C.c_int64(0)
    check(_lib.hip().crt_scene_export_identity(C.byref(d), C.byref(o), None, C.byref(n)), "crt_scene_export_identity")
    out = np.zeros((n.value, 3), np.int32)
    check(_lib.hip().crt_scene_export_identity(C.byref(d), C.byref(o), _p(out), C.byref(n)), "crt_scene_export_identity")
    return out


def export_desc(d: SceneDesc, bvh: str = "reference", **options) -> dict:
    """crt_scene_export of any scene description (HostScene.desc() or a caller's own)."""
    o = scene_options(bvh, **options)
    info = (C.c_int64 * 10)()
    check(_lib.hip().crt_scene_export(C.byref(d), C.byref(o), None, None, None, info), "crt_scene_export")
    nodes = np.zeros((info[0], 4), np.float32)
    prims = np.zeros((info[1], 4), np.float32)
    rank_code = np.zeros(info[2], np.int32)
    check(_lib.hip().crt_scene_export(C.byref(d), C.byref(o), _p(nodes), _p(prims), _p(rank_code), info),
          "crt_scene_export")
    keys = ("node_float4s", "prim_float4s", "ranks", "nodes_per_layout", "layouts", "width", "stack_bound",
            "excluded", "sphere_first", "n_ray_spheres")
    out = dict(zip(keys, (int(v) for v in info)))
    out.update(nodes=nodes, prims=prims, rank_code=rank_code)
    return out


def create_scene(d: SceneDesc, device: int = 0, bvh: str = "reference", **options) -> "Scene":
    """crt_scene_create_ex of any scene description (the caller keeps the arrays alive during the call)."""
    o = scene_options(bvh, **options)
    h = C.c_void_p()
    check(_lib.hip().crt_scene_create_ex(C.byref(d), int(device), C.byref(o), C.byref(h)), "crt_scene_create_ex")
    return Scene(h, device)


def scene_options(bvh: str = "reference", leaf_size: int = 0, layouts: int = 0, traversal_cost: float = 0.0,
                  width: int = 0, gpu_build: bool = False, stack_cap: int = 0, spatial_splits: bool = False,
                  spatial_alpha: float = 0.0, spatial_max_dup: float = 0.0):
    modes = {"reference": _lib.BVH_REFERENCE, "rebuilt": _lib.BVH_REBUILT}
    if bvh not in modes:
        raise ValueError(f"bvh must be one of {sorted(modes)}")
    o = _lib.SceneOptions()
    o.bvh, o.leaf_size, o.layouts = modes[bvh], int(leaf_size), int(layouts)
    o.traversal_cost = float(traversal_cost)
    o.width = int(width)
    o.gpu_build = int(bool(gpu_build))
    o.stack_cap = int(stack_cap)
    o.spatial_splits = int(bool(spatial_splits))
    o.spatial_alpha = float(spatial_alpha)
    o.spatial_max_dup = float(spatial_max_dup)
    return o


def _nodes_to_np(ptr, n):
    if n == 0:
        return np.zeros((0, 6), np.float32), np.zeros((0, 5), np.int32)
    raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (n * C.sizeof(_lib.BvhNodeDesc),))
    rec = raw.view(np.dtype([("b", "<f4", 6), ("i", "<i4", 5)]))
    return rec["b"].copy(), rec["i"].copy()


# crt_hit as a numpy record (two 16-B rows)
HIT_DTYPE = np.dtype([("t", "<f4"), ("object", "<i4"), ("primitive", "<i4"), ("material", "<i4"),
                      ("normal", "<f4", 3), ("front_face", "<i4")])


def pack_rays(rays_or_o, d=None, tmax=None) -> np.ndarray:
    """crt_ray rows, float32 [n, 8] = (o.xyz, tmax, d.xyz, 0), from an [n, 8] array or from origins [n, 3], directions
    [n, 3] and tmax (None = inf, a scalar or [n])."""
    if d is None:
        r = np.ascontiguousarray(rays_or_o, np.float32)
        if r.ndim != 2 or r.shape[1] != 8:
            raise ValueError("rays must have shape [n, 8]")
        return r
    o = np.asarray(rays_or_o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions differ in shape")
    r = np.zeros((len(o), 8), np.float32)
    r[:, :3], r[:, 4:7] = o, d
    r[:, 3] = np.inf if tmax is None else np.asarray(tmax, np.float32)
    return r


def validate_rays(rays) -> int:
    """Index of the first ray that breaks a precondition of the ray queries, or -1 (crt_trace_validate_rays; no GPU)."""
    r = pack_rays(rays)
    bad = C.c_int64(-1)
    rc = _lib.hip().crt_trace_validate_rays(_p(r), len(r), C.byref(bad))
    if rc not in (0, -1):
        check(rc, "crt_trace_validate_rays")
    return int(bad.value) if rc else -1


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"     # no torch import for numpy callers


def _hit_fields(f32, i32) -> dict:
    return {"t": f32[:, 0], "object": i32[:, 1], "primitive": i32[:, 2], "material": i32[:, 3],
            "normal": f32[:, 4:7], "front_face": i32[:, 7]}


class Scene:
    """Device scene handle (crt_scene)."""

    def __init__(self, handle, device):
        self.h = handle
        self.device = device

    def stats(self) -> dict:
        s = SceneStats()
        check(_lib.hip().crt_scene_get_stats(self.h, C.byref(s)), "crt_scene_get_stats")
        return {k: getattr(s, k) for k, _ in SceneStats._fields_}

    def close(self):
        if getattr(self, "h", None) and _lib is not None:   # None: interpreter exit (see HostScene.__del__)
            _lib.hip().crt_scene_destroy(self.h)
            self.h = None

    __del__ = close

    # ---- ray queries (crt_hip.h "ray queries", DESIGN.md "Ray queries")
    @staticmethod
    def _trace_options(mode, grid_waves, stack_lds, refill_threshold):
        o = _lib.TraceOptions()
        o.mode, o.grid_waves, o.stack_lds, o.refill_threshold = int(mode), int(grid_waves), int(stack_lds), int(refill_threshold)
        return o

    def _trace_torch(self, rays, o, want_hits, count_work, count=None, out=None):
        import torch
        if count is not None or out is not None:
            # the kinds first, the device last (these checks come before any library call)
            if count is not None and (not _is_torch(count) or count.dtype != torch.int32 or count.numel() != 1
                                      or count.dim() > 1):
                raise ValueError("count must be a 1-element int32 tensor")
            kind = (torch.float32, torch.int32) if want_hits else (torch.uint8,)
            if out is not None and (not _is_torch(out) or out.dtype not in kind or not out.is_contiguous()
                                    or tuple(out.shape) != ((rays.shape[0], 8) if want_hits else (rays.shape[0],))):
                raise ValueError("out must be a contiguous " + ("float32 or int32 [n, 8]" if want_hits else "uint8 [n]")
                                 + " tensor as long as the rays")
        if (rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous()
                or not rays.is_cuda or rays.device.index != self.device):
            raise ValueError("rays must be a contiguous float32 [n, 8] tensor on the scene's device")
        for name, x in (("count", count), ("out", out)):
            if x is not None and (not x.is_cuda or x.device.index != self.device):
                raise ValueError(f"{name} must be on the scene's device")
        n = rays.shape[0]
        if out is not None:
            hits, occ = (out, None) if want_hits else (None, out)
        else:
            hits = torch.empty((n, 8), dtype=torch.float32, device=rays.device) if want_hits else None
            occ = None if want_hits else torch.empty((n,), dtype=torch.uint8, device=rays.device)
        stream = torch.cuda.current_stream(rays.device).cuda_stream
        flags = _lib.TRACE_COUNT_WORK if count_work else 0
        if count is not None:
            check(_lib.require("crt_scene_trace_indirect_device")(
                self.h, rays.data_ptr(), count.data_ptr(), n, C.byref(o), hits.data_ptr() if want_hits else None,
                None if want_hits else occ.data_ptr(), flags, stream), "crt_scene_trace_indirect_device")
        else:
            check(_lib.hip().crt_scene_trace_device(self.h, rays.data_ptr(), n, C.byref(o),
                                                    hits.data_ptr() if want_hits else None,
                                                    None if want_hits else occ.data_ptr(), flags, stream),
                  "crt_scene_trace_device")
        return hits if want_hits else occ

    def trace(self, rays_or_o, d=None, tmax=None, *, mode=0, grid_waves=0, stack_lds=0, refill_threshold=0,
              count_work=False, count=None, out=None) -> dict:
        """Closest hit of every ray over [0.001, inf), reported when t <= tmax: a dict of arrays t, object, primitive,
        material, normal [n, 3], front_face (a miss: t = -1, the rest 0; see crt_hit in crt_hip.h).

        numpy: rays float32 [n, 8] (pack_rays), or origins, directions and tmax; the rays are checked on the host
        (CrtError names the first bad one) and the result is numpy.  torch: a contiguous float32 [n, 8] tensor on the
        scene's device; the query is enqueued on torch's current stream without a host copy and the dict holds views
        of ONE [n, 8] tensor of crt_hit rows, float32 columns (t, normal) of the tensor itself ("f32") and int32
        columns (object, primitive, material, front_face) of its int32 view ("i32").  The caller keeps the
        preconditions.  count_work fills trace_stats()' work counts (numpy rays then go through the device entry too).

        A torch query (and a numpy one with count_work) is asynchronous: a device error of its kernel, such as a
        traversal-stack entry dropped below the tree's bound, is raised by the next trace_stats() call, not here.
        The numpy path without count_work waits for the kernel and raises such an error itself.

        count (torch rays only): a 1-element int32 tensor on the scene's device.  The query traces rays [0, min(count,
        n)), count read by the kernel on the stream when it runs and never by the host (crt_scene_trace_indirect_device;
        a negative count is its bit pattern, so it clamps to n); the result has n rows of which only those are
        written.  out: the [n, 8] float32 or int32 tensor to write the hit rows into instead of a new one."""
        o = self._trace_options(mode, grid_waves, stack_lds, refill_threshold)
        if count is not None or out is not None:
            if not _is_torch(rays_or_o):
                raise ValueError("count= and out= take torch rays")
            if d is not None or tmax is not None:
                raise ValueError("a torch query takes one [n, 8] tensor of crt_ray rows")
            torch = __import__("torch")
            got = self._trace_torch(rays_or_o, o, True, count_work, count, out)
            f32, i32 = (got.view(torch.float32), got.view(torch.int32))
            return dict(_hit_fields(f32, i32), f32=f32, i32=i32)
        if _is_torch(rays_or_o):
            if d is not None or tmax is not None:
                raise ValueError("a torch query takes one [n, 8] tensor of crt_ray rows")
            f32 = self._trace_torch(rays_or_o, o, True, count_work)
            i32 = f32.view(__import__("torch").int32)
            return dict(_hit_fields(f32, i32), f32=f32, i32=i32)
        r = pack_rays(rays_or_o, d, tmax)
        if count_work:
            import torch
            self._check_rays(r)
            f32 = self._trace_torch(torch.from_numpy(r).to(f"cuda:{self.device}"), o, True, True).cpu().numpy()
        else:
            f32 = np.zeros((len(r), 8), np.float32)
            check(_lib.hip().crt_scene_trace(self.h, _p(r), len(r), C.byref(o), _p(f32)), "crt_scene_trace")
        return {k: v.copy() for k, v in _hit_fields(f32, f32.view(np.int32)).items()}

    def occluded(self, rays_or_o, d=None, tmax=None, *, mode=0, grid_waves=0, stack_lds=0, refill_threshold=0,
                 count_work=False, count=None, out=None):
        """uint8 [n]: 1 where trace() with the same rays reports a hit (the 4-wide stream kernel retires a lane at its
        first accepted hit with t <= tmax).  numpy in, numpy out; a torch tensor in, a torch tensor out (see trace,
        also for where a device error of an asynchronous query is raised: trace_stats(), and for count and out: out
        is a uint8 [n] tensor here)."""
        o = self._trace_options(mode, grid_waves, stack_lds, refill_threshold)
        if count is not None or out is not None:
            if not _is_torch(rays_or_o):
                raise ValueError("count= and out= take torch rays")
            if d is not None or tmax is not None:
                raise ValueError("a torch query takes one [n, 8] tensor of crt_ray rows")
            return self._trace_torch(rays_or_o, o, False, count_work, count, out)
        if _is_torch(rays_or_o):
            if d is not None or tmax is not None:
                raise ValueError("a torch query takes one [n, 8] tensor of crt_ray rows")
            return self._trace_torch(rays_or_o, o, False, count_work)
        r = pack_rays(rays_or_o, d, tmax)
        if count_work:
            import torch
            self._check_rays(r)
            return self._trace_torch(torch.from_numpy(r).to(f"cuda:{self.device}"), o, False, True).cpu().numpy()
        out = np.zeros(len(r), np.uint8)
        check(_lib.hip().crt_scene_occluded(self.h, _p(r), len(r), C.byref(o), _p(out)), "crt_scene_occluded")
        return out

    @staticmethod
    def _check_rays(r):
        check(_lib.hip().crt_trace_validate_rays(_p(r), len(r), None), "crt_trace_validate_rays")

    def trace_stats(self) -> dict:
        """Of the last ray query on this scene (crt_scene_trace_last_stats; waits for it): kernel_ms, and for a
        count_work query rays, box_tests, tri_tests, sphere_tests, step_lane_slots, step_active_lanes (lane fill =
        step_active_lanes / step_lane_slots)."""
        s = _lib.TraceStats()
        check(_lib.hip().crt_scene_trace_last_stats(self.h, C.byref(s)), "crt_scene_trace_last_stats")
        return {k: (float if k == "kernel_ms" else int)(getattr(s, k)) for k, _ in _lib.TraceStats._fields_}

    # ---- path steps (crt_hip.h "path steps", DESIGN.md "Path steps")
    def path_step(self, rays, hits, paths, max_bounces, rng, linear):
        """One bounce of material scattering for a batch of paths, in place on torch tensors (paths.path_step)."""
        from . import paths as _paths
        _paths.path_step(self, rays, hits, paths, max_bounces, rng, linear)

    def path_advance(self, renderer, rays, hits, paths, max_bounces, remaining, rng=None, linear=None, out=None,
                     count_in=None, totals=None):
        """Step, regenerate and compact a batch of paths into an output batch (paths.advance): returns (rays_out,
        paths_out, count), count a 1-element int32 device tensor.  count_in: the device count of the input entries
        (the count of the advance before); totals: an int64 [2] device tensor the call adds to."""
        from . import paths as _paths
        return _paths.advance(self, renderer, rays, hits, paths, max_bounces, remaining, rng, linear, out, count_in,
                              totals)

    def path_finish(self, renderer, rays, paths, max_bounces, remaining, rng=None, linear=None, count_in=None,
                    totals=None):
        """Run a batch of paths, and their pixels' remaining samples, to the end in one kernel (paths.finish)."""
        from . import paths as _paths
        _paths.finish(self, renderer, rays, paths, max_bounces, remaining, rng, linear, count_in, totals)


def load_scene(obj_files, device: int = 0, **upload_options):
    hs = HostScene(obj_files)
    return hs, hs.upload(device, **upload_options)


class Renderer:
    """CUDARenderer equivalent over crt_renderer (CUDARenderer.cuh:9-60)."""

    def __init__(self, width: int, height: int, device: int = 0):
        h = C.c_void_p()
        check(_lib.hip().crt_renderer_create(int(width), int(height), int(device), C.byref(h)), "crt_renderer_create")
        self.h, self.width, self.height, self.device = h, width, height, device
        self._owned = True

    @classmethod
    def _borrow(cls, handle, width: int, height: int, device: int, owner):
        """A view of a renderer owned by someone else (e.g. a Viewer); never destroys it."""
        r = cls.__new__(cls)
        r.h, r.width, r.height, r.device, r._owned, r._owner = C.c_void_p(handle), width, height, device, False, owner
        return r

    def close(self):
        if getattr(self, "h", None) and _lib is not None:   # None: interpreter exit (see HostScene.__del__)
            if getattr(self, "_owned", True):
                _lib.hip().crt_renderer_destroy(self.h)
            self.h = None

    __del__ = close

    def init_rand(self, seed: int = 41, subsequence_base: int = 0, stream=None):
        check(_lib.hip().crt_renderer_init_rand(self.h, int(seed), int(subsequence_base), stream), "init_rand")

    def set_schedule(self, probe_spp: int = -1, min_spp: int = 64, tile_key: int = 2, probe_stride: int = 0):
        flags = ((int(tile_key) & 0xf) << 16) | ((int(probe_stride) & 0xf) << 20)
        check(_lib.hip().crt_renderer_set_schedule(self.h, int(probe_spp), int(min_spp), flags), "set_schedule")

    def set_critical_tiles(self, tiles: int = -1, lanes: int = 16):
        check(_lib.hip().crt_renderer_set_critical_tiles(self.h, int(tiles), int(lanes)), "set_critical_tiles")

    def set_tail_fill(self, tiles: int = -1, spp: int = 0):
        """Variant 8: the first `tiles` tiles of the cost order hold back their last `spp` samples, which follow the
        launch's tiles as small items (crt_renderer_set_tail_fill; -1 = automatic, 0 = off).  Results never depend on
        it.  Raises CrtError naming the entry when the loaded library predates it."""
        check(_lib.require("crt_renderer_set_tail_fill")(self.h, int(tiles), int(spp)), "set_tail_fill")

    def last_tail_fill(self) -> dict:
        """The last render's tail fill (crt_renderer_last_tail_fill): tiles, held-back samples, parts rendered inside
        the main launch and by the sweep; all 0 when it rendered without.  Waits for that render."""
        a = (C.c_int * 4)()
        check(_lib.require("crt_renderer_last_tail_fill")(self.h, a), "last_tail_fill")
        return dict(zip(("tiles", "spp", "in_launch", "swept"), (int(v) for v in a)))

    def set_top_levels(self, levels: int = -1):
        """4-wide kernels: a new ray's first node steps from the LDS copy of the tree's top nodes (-1 = default)."""
        check(_lib.hip().crt_renderer_set_top_levels(self.h, int(levels)), "set_top_levels")

    def set_pixel_shard(self, shard: int = 0, shards: int = 1):
        """Render only every shards-th 8x8 tile (from shard) with all samples; other pixels stay 0 (bit-exact
        multi-GPU mode, crt_renderer_set_pixel_shard)."""
        check(_lib.hip().crt_renderer_set_pixel_shard(self.h, int(shard), int(shards)), "set_pixel_shard")

    def set_kernel_variant(self, variant: int):
        check(_lib.hip().crt_renderer_set_kernel_variant(self.h, int(variant)), "set_kernel_variant")

    def set_occupancy_target(self, waves_per_simd: int):
        check(_lib.hip().crt_renderer_set_occupancy_target(self.h, int(waves_per_simd)), "set_occupancy_target")

    def set_regen_threshold(self, lanes: int):
        check(_lib.hip().crt_renderer_set_regen_threshold(self.h, int(lanes)), "set_regen_threshold")

    def set_stack_lds(self, entries: int):
        check(_lib.hip().crt_renderer_set_stack_lds(self.h, int(entries)), "set_stack_lds")

    def set_camera(self, cam: CameraDesc):
        self._cam = cam
        check(_lib.hip().crt_renderer_set_camera(self.h, C.byref(cam)), "set_camera")

    def render(self, scene: Scene, spp: int, max_bounces: int = 20, accumulate=False, count_work=False, stream=None):
        flags = (RENDER_ACCUMULATE if accumulate else 0) | (RENDER_COUNT_WORK if count_work else 0)
        check(_lib.hip().crt_renderer_render(self.h, scene.h, int(spp), int(max_bounces), flags, stream), "render")

    def render_wavefront(self, scene: Scene, spp: int, max_bounces: int = 20, accumulate=False, trace_options=None,
                         stream=None, sync_every=None, finish_below=None) -> dict:
        """The frame of render() as a wavefront in the library (crt_renderer_render_wavefront): camera rays, then trace /
        advance rounds over the handle's own batches (164 B per pixel, allocated by the first call), one host wait per
        round.  The same sums, RNG state and ray count, bit for bit.  trace_options: keywords of Scene.trace (mode,
        grid_waves, stack_lds, refill_threshold).  Synchronous.  Returns {"rays", "iterations", "ms"}.

        sync_every: None is that loop.  An int is the loop enqueued ahead (crt_renderer_render_wavefront_queued): the
        rounds take their batch size from the device, and the host waits once per sync_every rounds (0: the library's
        default).  The same frame and the same numbers for every value.

        finish_below: None keeps the dispatch above.  An int is the queued loop with a hand-off
        (crt_renderer_render_wavefront_finish; sync_every None is then 0): as soon as the batch size the host holds
        is <= finish_below, the batch goes to one kernel that runs its paths and their pixels' samples to the end
        (Scene.path_finish).  0 never hands off, a value >= the number of pixels is the whole frame through that
        kernel, -1 the library's default.  The same frame and rays; iterations counts the finish as one."""
        o = Scene._trace_options(**dict(dict(mode=0, grid_waves=0, stack_lds=0, refill_threshold=0), **(trace_options or {})))
        s = _lib.WavefrontStats()
        flags = RENDER_ACCUMULATE if accumulate else 0
        if finish_below is not None:
            fn = _lib.require("crt_renderer_render_wavefront_finish")
            check(fn(self.h, scene.h, int(spp), int(max_bounces), flags, C.byref(o), int(sync_every or 0),
                     int(finish_below), C.byref(s), stream), "render_wavefront_finish")
        elif sync_every is None:
            fn = _lib.require("crt_renderer_render_wavefront")
            check(fn(self.h, scene.h, int(spp), int(max_bounces), flags, C.byref(o), C.byref(s), stream), "render_wavefront")
        else:
            fn = _lib.require("crt_renderer_render_wavefront_queued")
            check(fn(self.h, scene.h, int(spp), int(max_bounces), flags, C.byref(o), int(sync_every), C.byref(s), stream),
                  "render_wavefront_queued")
        return {"rays": int(s.rays), "iterations": int(s.iterations), "ms": float(s.ms)}

    def resolve(self, scale: float, stream=None):
        check(_lib.hip().crt_renderer_resolve(self.h, C.c_float(scale), stream), "resolve")

    def synchronize(self, stream=None):
        check(_lib.hip().crt_renderer_synchronize(self.h, stream), "synchronize")

    def linear(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 3), np.float32)
        check(_lib.hip().crt_renderer_read_linear(self.h, _p(out)), "read_linear")
        return out

    def write_linear(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr, np.float32)
        check(_lib.hip().crt_renderer_write_linear(self.h, _p(a)), "write_linear")

    def rgba8(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.uint8)
        check(_lib.hip().crt_renderer_read_rgba8(self.h, _p(out)), "read_rgba8")
        return out

    def rng_state(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 6), np.uint32)
        check(_lib.hip().crt_renderer_read_rng(self.h, _p(out)), "read_rng")
        return out

    def counters(self) -> dict:
        w = WorkCounters()
        check(_lib.hip().crt_renderer_get_counters(self.h, C.byref(w)), "get_counters")
        return {k: int(getattr(w, k)) for k, _ in WorkCounters._fields_}

    def schedule_stats(self) -> dict:
        """Lane-slot diagnostics of the last counting render (see crt_renderer_get_schedule_stats)."""
        a = (C.c_ulonglong * 3)()
        check(_lib.hip().crt_renderer_get_schedule_stats(self.h, a), "get_schedule_stats")
        return {"step_lane_slots": int(a[0]), "round_lane_slots": int(a[1]), "wave_trace_calls": int(a[2])}

    def section_profile(self) -> dict:
        """Shader-clock cycles per section of the last counting render (variant 4), summed over waves."""
        a = (C.c_ulonglong * 8)()
        check(_lib.hip().crt_renderer_get_section_profile_ex(self.h, a, 8), "get_section_profile_ex")
        return dict(zip(("cyc_regen", "cyc_step", "cyc_round", "passes", "waves", "cyc_shade", "cyc_next", "cyc_sph"),
                        (int(v) for v in a)))

    def last_kernel_name(self) -> str:
        return (_lib.hip().crt_renderer_last_kernel_name(self.h) or b"").decode()

    def last_launch_frozen(self) -> int:
        """Which twin of last_kernel_name() the last render launched (crt_renderer_last_launch_frozen): 1 = the frozen
        twin of a plain variant-8 kernel, 0 = its open twin or any other kernel.  Raises CrtError naming the entry when
        the loaded library predates it."""
        return int(_lib.require("crt_renderer_last_launch_frozen")(self.h))

    def last_schedule(self) -> dict:
        """The last variant-8 render's occupancy choice (crt_renderer_last_schedule): rho = the probe's largest tile work
        over the mean work per occupancy-6 wave slot (0 without the probe-based choice), the occupancy launched, and the
        largest and mean tile works."""
        a = (C.c_float * 4)()
        check(_lib.hip().crt_renderer_last_schedule(self.h, a), "last_schedule")
        return {"rho": a[0], "occupancy": int(a[1]), "max_tile_work": a[2], "mean_tile_work": a[3]}

    def last_timings(self) -> dict:
        """HIP-event ms of the last render: the whole render, the probe + tile sort before the main kernel, and the
        main render kernel alone (crt_renderer_last_timings)."""
        a = (C.c_float * 3)()
        check(_lib.hip().crt_renderer_last_timings(self.h, a), "last_timings")
        return {"render_ms": float(a[0]), "probe_sort_ms": float(a[1]), "main_kernel_ms": float(a[2])}

    def set_temporal_order(self, on: bool):
        """Variant 7: tiles most expensive first by the previous frame's rays per pixel (crt_renderer_set_temporal_order)."""
        check(_lib.hip().crt_renderer_set_temporal_order(self.h, int(bool(on))), "set_temporal_order")

    def set_drain_threshold(self, lanes: int):
        """Variant 7: regeneration threshold once the pixel queue is empty, 0 = unchanged (crt_renderer_set_drain_threshold)."""
        check(_lib.hip().crt_renderer_set_drain_threshold(self.h, int(lanes)), "set_drain_threshold")

    def set_wave_drain(self, sixty_fourths: int):
        """Variants 4/8: a draining wave passes at sixty_fourths/64 of its live lanes (crt_renderer_set_wave_drain)."""
        check(_lib.hip().crt_renderer_set_wave_drain(self.h, int(sixty_fourths)), "set_wave_drain")

    def set_xcd_regions(self, on: bool):
        """Variant 8: XCD groups render equal-cost screen strips (crt_renderer_set_xcd_regions)."""
        check(_lib.hip().crt_renderer_set_xcd_regions(self.h, int(bool(on))), "set_xcd_regions")

    # ---- self-tests of the schedules (crt_hip.h crt_selftest_tile_schedule ff.): stages on caller-supplied costs
    SCHEDULE_BUFFERS = {"order": 0, "tile_key": 1, "pix_cost": 2, "pix_rays": 3, "tile_order": 4}

    def schedule_buffer(self, which: str) -> np.ndarray:
        """A schedule buffer of this renderer, whole, as uint32 (crt_selftest_schedule_buffer): "order", "tile_key",
        "pix_cost" (the probe's per-pixel costs), "pix_rays" (the last temporal frame's rays per pixel), "tile_order";
        empty while the buffer is not allocated."""
        fn = _lib.require("crt_selftest_schedule_buffer")
        n = C.c_int64(0)
        check(fn(self.h, self.SCHEDULE_BUFFERS[which], None, 0, C.byref(n)), "selftest_schedule_buffer")
        out = np.zeros(n.value, np.uint32)
        check(fn(self.h, self.SCHEDULE_BUFFERS[which], _p(out), n.value, C.byref(n)), "selftest_schedule_buffer")
        return out

    def selftest_tile_schedule(self, pix_cost, stride=1, key_mode=2, shard=0, shards=1, xcd_regions=False, stats=False):
        """Variant 8 / 10's tile schedule on per-pixel costs (crt_selftest_tile_schedule): returns (keys as sorted
        [tiles], order [tiles], the rest of the order buffer, (largest tile work, total work) or None)."""
        c = np.ascontiguousarray(pix_cost, np.uint32).reshape(-1)
        if c.size != self.width * self.height:
            raise ValueError("pix_cost must hold width * height costs")
        st = (C.c_ulonglong * 2)()
        check(_lib.require("crt_selftest_tile_schedule")(self.h, _p(c), int(stride), int(key_mode), int(shard), int(shards),
                                                         int(bool(xcd_regions)), st if stats else None),
              "selftest_tile_schedule")
        keys, order = self.schedule_buffer("tile_key"), self.schedule_buffer("order")
        return keys, order[:keys.size], order[keys.size:], ((int(st[0]), int(st[1])) if stats else None)

    def selftest_pixel_order(self, kind: str, costs=None, shard=0, shards=1) -> np.ndarray:
        """Variant 7's orders (crt_selftest_pixel_order): kind "probe" (costs per pixel), "temporal" (costs = a
        rays-per-pixel map), "rows", "shard".  Returns the whole order buffer; schedule_buffer("tile_order") and
        ("tile_key") hold the temporal order's tiles and keys."""
        k = {"probe": 0, "temporal": 1, "rows": 2, "shard": 3}[kind]
        c = None
        if k <= 1:
            c = np.ascontiguousarray(costs, np.uint32).reshape(-1)
            if c.size != self.width * self.height:
                raise ValueError("costs must hold width * height entries")
        check(_lib.require("crt_selftest_pixel_order")(self.h, k, None if c is None else _p(c), int(shard), int(shards)),
              "selftest_pixel_order")
        return self.schedule_buffer("order")

    # ---- adaptive sampling (crt_hip.h crt_renderer_render_adaptive ff.)
    def _tiles(self):
        return (self.height + 7) // 8, (self.width + 7) // 8

    def render_adaptive(self, scene: Scene, spp_min: int, spp_max: int, tolerance: float, max_bounces: int = 20,
                        list_by_error: bool = False, critical_tiles: bool = False, stream=None) -> dict:
        """A frame whose 8x8 tiles stop receiving samples once their error estimate is <= tolerance
        (crt_renderer_render_adaptive): spp_min samples (even, >= 2) everywhere, then passes that double the samples
        of the unconverged tiles up to spp_max.  A tile that ends at n samples holds render(n)'s sums and RNG state bit
        for bit; tile_spp() says which n, resolve_adaptive() scales each tile by its own.  tolerance: +inf refines
        nothing, a negative one everything; there is no default, and the result is biased (the rule looks at the samples
        it stops).  Measurements only, no result depends on them: list_by_error True lists a pass's tiles largest error
        first instead of in tile order, critical_tiles True runs a pass's first tiles at set_critical_tiles' threshold.
        Synchronous.  Returns
        {"samples", "passes", "tiles_refined", "tiles_at_max", "ms", "mean_spp"}."""
        if not isinstance(scene, Scene):
            raise ValueError("render_adaptive: scene must be a Scene")
        for name, v in (("spp_min", spp_min), ("spp_max", spp_max), ("max_bounces", max_bounces)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"render_adaptive: {name} must be an int")
        if spp_min < 2 or spp_min % 2:
            raise ValueError("render_adaptive: spp_min must be even and >= 2")
        if spp_max < spp_min or spp_max >= 1 << 31:
            raise ValueError("render_adaptive: spp_max must be in [spp_min, 2^31)")
        if max_bounces < 1:
            raise ValueError("render_adaptive: max_bounces must be >= 1")
        try:
            tol = float(tolerance)
        except (TypeError, ValueError):
            raise ValueError("render_adaptive: tolerance must be a number") from None
        if tol != tol:
            raise ValueError("render_adaptive: tolerance is NaN")
        if scene.device != self.device:
            raise ValueError("render_adaptive: scene and renderer are on different devices")
        o = _lib.AdaptiveOptions(int(spp_min), int(spp_max), tol, (1 if list_by_error else 0) | (2 if critical_tiles else 0))
        s = _lib.AdaptiveStats()
        check(_lib.require("crt_renderer_render_adaptive")(self.h, scene.h, C.byref(o), int(max_bounces), 0, C.byref(s),
                                                           stream), "render_adaptive")
        return {"samples": int(s.samples), "passes": int(s.passes), "tiles_refined": int(s.tiles_refined),
                "tiles_at_max": int(s.tiles_at_max), "ms": float(s.ms),
                "mean_spp": int(s.samples) / (self.width * self.height)}

    def resolve_adaptive(self, stream=None):
        """resolve() with each pixel's own scale, 1 / the samples its tile holds (crt_renderer_resolve_adaptive)."""
        check(_lib.require("crt_renderer_resolve_adaptive")(self.h, stream), "resolve_adaptive")

    def tile_spp(self) -> np.ndarray:
        """Samples held per 8x8 tile, int32 [tiles_y, tiles_x], after an adaptive render."""
        out = np.zeros(self._tiles(), np.int32)
        check(_lib.require("crt_renderer_read_tile_spp")(self.h, _p(out)), "read_tile_spp")
        return out

    def tile_error(self) -> np.ndarray:
        """The last error estimate per 8x8 tile, float32 [tiles_y, tiles_x], after an adaptive render."""
        out = np.zeros(self._tiles(), np.float32)
        check(_lib.require("crt_renderer_read_tile_error")(self.h, _p(out)), "read_tile_error")
        return out

    def adaptive_prev(self) -> np.ndarray:
        """The half-buffer sums of the adaptive state, float32 [height, width, 3]."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        check(_lib.require("crt_renderer_read_adaptive_prev")(self.h, _p(out)), "read_adaptive_prev")
        return out

    def selftest_adaptive_plan(self, sum, prev, tile_spp, n: int, next: int, tolerance: float):
        """One plan step on caller-supplied buffers (crt_selftest_adaptive_plan): sum and prev [height, width, 3]
        float32, tile_spp [tiles_y, tiles_x] int32.  Returns the listed tiles, largest error first; tile_error(),
        tile_spp(), adaptive_prev() and linear() hold the rest."""
        ty, tx = self._tiles()
        s, p = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (sum, prev))
        t = np.ascontiguousarray(tile_spp, np.int32).reshape(-1)
        if s.size != self.width * self.height * 3 or p.size != s.size:
            raise ValueError("selftest_adaptive_plan: sum and prev must hold height * width * 3 floats")
        if t.size != ty * tx:
            raise ValueError("selftest_adaptive_plan: tile_spp must hold tiles_y * tiles_x entries")
        if n < 2 or n % 2 or next < n:
            raise ValueError("selftest_adaptive_plan: n must be even and >= 2, next >= n")
        if float(tolerance) != float(tolerance):
            raise ValueError("selftest_adaptive_plan: tolerance is NaN")
        lst, cnt = np.zeros(ty * tx, np.uint32), C.c_uint32(0)
        check(_lib.require("crt_selftest_adaptive_plan")(self.h, _p(s), _p(p), _p(t), int(n), int(next),
                                                         C.c_float(float(tolerance)), _p(lst), C.byref(cnt)),
              "selftest_adaptive_plan")
        return lst[:cnt.value].copy()

    # ---- denoiser (crt_hip.h crt_renderer_compute_guides ff.)
    def compute_guides(self, scene: Scene, stream=None, **trace_options):
        """The first-hit guide buffers of this renderer's camera over `scene` (crt_renderer_compute_guides): pixel-centre
        rays, Scene.trace's closest hits, and one record (normal.xyz, t, position.xyz, key) per pixel on the device.
        trace_options: keywords of Scene.trace (mode, grid_waves, stack_lds, refill_threshold).  Consumes no RNG state,
        touches no sums; valid until the camera, the scene or the frame size changes.  Asynchronous."""
        if not isinstance(scene, Scene):
            raise ValueError("compute_guides: scene must be a Scene")
        if scene.device != self.device:
            raise ValueError("compute_guides: scene and renderer are on different devices")
        unknown = set(trace_options) - {"mode", "grid_waves", "stack_lds", "refill_threshold"}
        if unknown:
            raise ValueError(f"compute_guides: unknown trace option {sorted(unknown)[0]}")
        o = Scene._trace_options(**dict(dict(mode=0, grid_waves=0, stack_lds=0, refill_threshold=0), **trace_options))
        check(_lib.require("crt_renderer_compute_guides")(self.h, scene.h, C.byref(o), stream), "compute_guides")

    def guides(self) -> np.ndarray:
        """The guide records, float32 [height, width, 8]: normal.xyz, t (-1: a miss), position.xyz, key (the object
        index as int bits, 0x7fffffff for a miss: read it through .view(np.int32))."""
        out = np.zeros((self.height, self.width, 8), np.float32)
        check(_lib.require("crt_renderer_read_guides")(self.h, _p(out)), "read_guides")
        return out

    @staticmethod
    def _filter_sigmas(who, first, sigmas, iterations):
        """Either a-trous filter's iterations and three sigmas (`first` names the colour term's), checked: the floats."""
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 1 <= iterations <= 8:
            raise ValueError(f"{who}: iterations must be an int in 1..8")
        sig = []
        for name, v in zip((first, "sigma_normal", "sigma_position"), sigmas):
            try:
                f = float(np.float32(v))
            except (TypeError, ValueError):
                raise ValueError(f"{who}: {name} must be a number") from None
            if not (f == float("inf") or 2.0 ** -50 <= f <= 2.0 ** 50):
                raise ValueError(f"{who}: {name} must be in [2^-50, 2^50] or +inf (that term off)")
            sig.append(f)
        return sig

    @staticmethod
    def _denoise_options(who, sigma_color, sigma_normal, sigma_position, iterations, tile_scale, direct_only):
        sig = Renderer._filter_sigmas(who, "sigma_color", (sigma_color, sigma_normal, sigma_position), iterations)
        flags = (_lib.DENOISE_TILE_SCALE if tile_scale else 0) | (_lib.DENOISE_DIRECT_ONLY if direct_only else 0)
        return _lib.DenoiseOptions(int(iterations), *sig, flags, 0)

    @staticmethod
    def _positive_scale(who, scale, hint=""):
        try:
            sc = float(np.float32(scale))
        except (TypeError, ValueError):
            raise ValueError(f"{who}: scale must be a number{hint}") from None
        if not sc > 0:
            raise ValueError(f"{who}: scale must be > 0")
        return sc

    def _flat(self, who, name, a, k):
        """`a` as a flat float32 array of height * width * k floats."""
        f = np.ascontiguousarray(a, np.float32).reshape(-1)
        if f.size != self.width * self.height * k:
            raise ValueError(f"{who}: {name} must hold height * width * {k} floats")
        return f

    @staticmethod
    def _denoise_stats(s) -> dict:
        return {"guides_ms": float(s.guides_ms), "filter_ms": float(s.filter_ms), "iterations": int(s.iterations),
                "pixels_hit": int(s.pixels_hit)}

    def denoise(self, sigma_color, sigma_normal, sigma_position, iterations: int = 5, scale=None, tile_scale: bool = False,
                direct_only: bool = False, stream=None) -> dict:
        """The edge-avoiding a-trous filter over scale * the sums, guided by compute_guides' buffers
        (crt_renderer_denoise; crt_hip.h states every operation).  The sigmas have no defaults: their scale depends on
        the scene; float("inf") switches a term off.  scale: what resolve() would take, e.g. pixel_sample_scale(spp);
        tile_scale True (after render_adaptive) takes 1 / each tile's own sample count instead.  The result is
        denoised(); the sums, the RNG state and rgba8() are untouched.  direct_only: a measurement switch, the same
        bits through the direct kernel alone.  Synchronous.
        Returns {"guides_ms", "filter_ms", "iterations", "pixels_hit"}."""
        o = self._denoise_options("denoise", sigma_color, sigma_normal, sigma_position, iterations, tile_scale, direct_only)
        if tile_scale:
            if scale is not None:
                raise ValueError("denoise: scale and tile_scale exclude each other")
            sc = 1.0
        else:
            sc = self._positive_scale("denoise", scale, " (or tile_scale=True)")
        s = _lib.DenoiseStats()
        check(_lib.require("crt_renderer_denoise")(self.h, C.byref(o), C.c_float(sc), C.byref(s), stream), "denoise")
        return self._denoise_stats(s)

    def denoise_iteration_ms(self) -> dict:
        """The last denoise()'s launches, timed one by one (crt_renderer_denoise_iteration_ms): {"input_ms": the kernel
        that forms scale * sums, "iteration_ms": [one per iteration run, stride 1 << i]}."""
        out = np.zeros(9, np.float32)
        check(_lib.require("crt_renderer_denoise_iteration_ms")(self.h, _p(out)), "denoise_iteration_ms")
        n = int(np.flatnonzero(out[1:] > 0).max(initial=-1)) + 1
        return {"input_ms": float(out[0]), "iteration_ms": [float(v) for v in out[1:1 + n]]}

    def denoised(self) -> np.ndarray:
        """The last denoise()'s frame, float32 [height, width, 3], linear."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        check(_lib.require("crt_renderer_read_denoised")(self.h, _p(out)), "read_denoised")
        return out

    def resolve_denoised(self, stream=None):
        """resolve(1.0) of the denoised frame into rgba8() (crt_renderer_resolve_denoised)."""
        check(_lib.require("crt_renderer_resolve_denoised")(self.h, stream), "resolve_denoised")

    def denoised_device_ptr(self) -> int:
        """The denoised frame on the device (height * width * 3 floats) for torch interop; 0 before compute_guides."""
        fn = _lib.require("crt_renderer_denoised_device_ptr")
        return fn(self.h) or 0

    def selftest_denoise(self, color, guides, sigma_color, sigma_normal, sigma_position, iterations: int = 5,
                         direct_only: bool = False) -> np.ndarray:
        """The filter on caller-supplied buffers (crt_selftest_denoise): color [height, width, 3] float32 (it replaces
        the sums), guides [height, width, 8] float32 (key as int bits).  Returns the filtered frame."""
        o = self._denoise_options("selftest_denoise", sigma_color, sigma_normal, sigma_position, iterations, False,
                                  direct_only)
        c = self._flat("selftest_denoise", "color", color, 3)
        g = self._flat("selftest_denoise", "guides", guides, 8)
        out = np.zeros((self.height, self.width, 3), np.float32)
        check(_lib.require("crt_selftest_denoise")(self.h, _p(c), _p(g), C.byref(o), _p(out)), "selftest_denoise")
        return out

    # ---- reprojection (crt_hip.h crt_renderer_reproject ff.)
    @staticmethod
    def _reproject_options(who, position_tolerance, normal_min, max_history):
        vals = []
        for name, v in (("position_tolerance", position_tolerance), ("normal_min", normal_min), ("max_history", max_history)):
            try:
                vals.append(float(np.float32(v)))
            except (TypeError, ValueError):
                raise ValueError(f"{who}: {name} must be a number") from None
        tol, nmin, cap = vals
        if not (tol == float("inf") or 2.0 ** -50 <= tol <= 2.0 ** 50):
            raise ValueError(f"{who}: position_tolerance must be in [2^-50, 2^50] or +inf (that term off)")
        if not (nmin == float("-inf") or -1.0 <= nmin <= 1.0):
            raise ValueError(f"{who}: normal_min must be in [-1, 1] or -inf (that term off)")
        if not 1.0 <= cap <= 2.0 ** 24:
            raise ValueError(f"{who}: max_history must be in [1, 2^24]")
        return _lib.ReprojectOptions(tol, nmin, cap, 0, 0)

    def _reproject(self, name, position_tolerance, normal_min, max_history, scale, stream) -> dict:
        """reproject() and reproject_moments(): `name` is the method's and, after crt_renderer_, the entry's."""
        o = self._reproject_options(name, position_tolerance, normal_min, max_history)
        sc = self._positive_scale(name, scale)
        s = _lib.ReprojectStats()
        check(_lib.require("crt_renderer_" + name)(self.h, C.byref(o), C.c_float(sc), C.byref(s), stream), name)
        return {"reproject_ms": float(s.reproject_ms), "pixels_reprojected": int(s.pixels_reprojected),
                "pixels_hit": int(s.pixels_hit)}

    def reproject(self, position_tolerance, normal_min=float("-inf"), *, max_history, scale=None, stream=None) -> dict:
        """Blend scale * the sums into the history that follows the camera (crt_renderer_reproject; crt_hip.h states
        every operation), guided by compute_guides' buffers of this frame and of the previous call's.  No defaults for
        position_tolerance (relative to the distance from the previous camera; a few pixel footprints) and max_history
        (the cap of the per-pixel length: the floor 1 / max_history of the blend weight); float("inf") / float("-inf")
        switch the position / normal term off.  scale: what resolve() would take.  The result is history(); the sums,
        the RNG state, rgba8(), guides() and denoised() are untouched.  Synchronous.
        Returns {"reproject_ms", "pixels_reprojected", "pixels_hit"}."""
        return self._reproject("reproject", position_tolerance, normal_min, max_history, scale, stream)

    def history(self) -> np.ndarray:
        """The last reproject()'s history, float32 [height, width, 4]: linear r, g, b and the length."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        check(_lib.require("crt_renderer_read_history")(self.h, _p(out)), "read_history")
        return out

    def resolve_history(self, stream=None):
        """resolve(1.0) of the history colours into rgba8() (crt_renderer_resolve_history)."""
        check(_lib.require("crt_renderer_resolve_history")(self.h, stream), "resolve_history")

    def history_device_ptr(self) -> int:
        """The latest history on the device (height * width * 4 floats) for torch interop; 0 before the first
        reproject().  Two buffers alternate: ask again after every reproject()."""
        fn = _lib.require("crt_renderer_history_device_ptr")
        return fn(self.h) or 0

    def reset_history(self):
        """The next reproject() starts over (crt_renderer_reset_history)."""
        check(_lib.require("crt_renderer_reset_history")(self.h), "reset_history")

    def denoise_history(self, sigma_color, sigma_normal, sigma_position, iterations: int = 5, direct_only: bool = False,
                        stream=None) -> dict:
        """denoise() with c_0 = the history colours instead of scale * the sums (crt_renderer_denoise_history): the same
        filter, the result is denoised().  Synchronous.  Returns {"guides_ms", "filter_ms", "iterations", "pixels_hit"}."""
        o = self._denoise_options("denoise_history", sigma_color, sigma_normal, sigma_position, iterations, False, direct_only)
        s = _lib.DenoiseStats()
        check(_lib.require("crt_renderer_denoise_history")(self.h, C.byref(o), C.byref(s), stream), "denoise_history")
        return self._denoise_stats(s)

    def _selftest_reproject(self, name, color, guides, prev_guides, prev_history, prev_moments, prev_camera,
                            position_tolerance, normal_min, max_history):
        """selftest_reproject() and, with a name that ends in _moments, selftest_reproject_moments()."""
        moments = name.endswith("_moments")
        o = self._reproject_options(name, position_tolerance, normal_min, max_history)
        c = self._flat(name, "color", color, 3)
        g = self._flat(name, "guides and prev_guides", guides, 8)
        pg = self._flat(name, "guides and prev_guides", prev_guides, 8)
        ph = None if prev_history is None else self._flat(name, "prev_history", prev_history, 4)
        if moments and (prev_history is None) != (prev_moments is None):
            raise ValueError(f"{name}: prev_moments goes with prev_history (both or neither)")
        pm = None if prev_moments is None else self._flat(name, "prev_moments", prev_moments, 2)
        if isinstance(prev_camera, _lib.CameraDesc):
            cam = prev_camera
        else:
            f = np.ascontiguousarray(prev_camera, np.float32).reshape(-1)
            if f.size < 12:
                raise ValueError(f"{name}: prev_camera must be a CameraDesc or at least 12 floats")
            cam = _lib.CameraDesc()
            C.memmove(C.byref(cam), f.ctypes.data, 4 * min(f.size, 19))
        out = np.zeros((self.height, self.width, 4), np.float32)
        out_m = np.zeros((self.height, self.width, 2), np.float32)
        prev = [None if ph is None else _p(ph)] + ([None if pm is None else _p(pm)] if moments else [])
        outs = [_p(out)] + ([_p(out_m)] if moments else [])
        check(_lib.require("crt_" + name)(self.h, _p(c), _p(g), _p(pg), *prev, C.byref(cam), C.byref(o), *outs), name)
        return (out, out_m) if moments else out

    def selftest_reproject(self, color, guides, prev_guides, prev_history, prev_camera, position_tolerance,
                           normal_min=float("-inf"), *, max_history) -> np.ndarray:
        """The reprojection on caller-supplied buffers (crt_selftest_reproject): color [height, width, 3] float32 (it
        replaces the sums, scale 1), guides and prev_guides [height, width, 8], prev_history [height, width, 4] or None
        (no previous frame), prev_camera a CameraDesc or its floats (origin, lower_left, horizontal, vertical first).
        Returns the new history [height, width, 4]."""
        return self._selftest_reproject("selftest_reproject", color, guides, prev_guides, prev_history, None, prev_camera,
                                        position_tolerance, normal_min, max_history)

    # ---- variance-guided filtering of the history (crt_hip.h crt_renderer_reproject_moments ff.)
    def reproject_moments(self, position_tolerance, normal_min=float("-inf"), *, max_history, scale=None, stream=None) -> dict:
        """reproject() that also carries the first two luminance moments of every pixel (crt_renderer_reproject_moments):
        the same history, bit for bit, plus moments() for denoise_history_variance().  A plain reproject() or
        reset_history() ends the moments' validity, and the next reproject_moments() then starts the whole history
        over.  Synchronous.  Returns {"reproject_ms", "pixels_reprojected", "pixels_hit"}."""
        return self._reproject("reproject_moments", position_tolerance, normal_min, max_history, scale, stream)

    def moments(self) -> np.ndarray:
        """The last reproject_moments()'s moments, float32 [height, width, 2]: the history's means of the luminance
        and of its square."""
        out = np.zeros((self.height, self.width, 2), np.float32)
        check(_lib.require("crt_renderer_read_moments")(self.h, _p(out)), "read_moments")
        return out

    @staticmethod
    def _denoise_variance_options(who, sigma_luminance, sigma_normal, sigma_position, min_history, iterations, direct_only):
        sig = Renderer._filter_sigmas(who, "sigma_luminance", (sigma_luminance, sigma_normal, sigma_position), iterations)
        try:
            mh = float(np.float32(min_history))
        except (TypeError, ValueError):
            raise ValueError(f"{who}: min_history must be a number") from None
        if not 1.0 <= mh <= 2.0 ** 24:
            raise ValueError(f"{who}: min_history must be in [1, 2^24]")
        return _lib.DenoiseVarianceOptions(int(iterations), *sig, mh, _lib.DENOISE_DIRECT_ONLY if direct_only else 0, 0)

    def denoise_history_variance(self, sigma_luminance, sigma_normal, sigma_position, *, min_history, iterations: int = 5,
                                 direct_only: bool = False, stream=None) -> dict:
        """The variance-guided a-trous filter over the history of reproject_moments()
        (crt_renderer_denoise_history_variance; crt_hip.h states every operation): a per-pixel variance from the
        moments, or from the 7 x 7 neighbourhood where the history is shorter than min_history, sets the width of the
        luminance edge-stop.  No defaults for the sigmas and min_history (the paper: sigma_luminance 4, 4 frames);
        float("inf") switches a term off.  The result is denoised(), the estimate variance().  Synchronous.
        Returns {"guides_ms", "filter_ms", "iterations", "pixels_hit"}."""
        o = self._denoise_variance_options("denoise_history_variance", sigma_luminance, sigma_normal, sigma_position,
                                           min_history, iterations, direct_only)
        s = _lib.DenoiseStats()
        check(_lib.require("crt_renderer_denoise_history_variance")(self.h, C.byref(o), C.byref(s), stream),
              "denoise_history_variance")
        return self._denoise_stats(s)

    def variance(self) -> np.ndarray:
        """The last denoise_history_variance()'s per-pixel variance estimate (before the filter), float32 [height, width]."""
        out = np.zeros((self.height, self.width), np.float32)
        check(_lib.require("crt_renderer_read_variance")(self.h, _p(out)), "read_variance")
        return out

    def selftest_reproject_moments(self, color, guides, prev_guides, prev_history, prev_moments, prev_camera,
                                   position_tolerance, normal_min=float("-inf"), *, max_history):
        """selftest_reproject() with the moments (crt_selftest_reproject_moments): prev_moments [height, width, 2] or
        None together with prev_history.  Returns (history [height, width, 4], moments [height, width, 2])."""
        return self._selftest_reproject("selftest_reproject_moments", color, guides, prev_guides, prev_history, prev_moments,
                                        prev_camera, position_tolerance, normal_min, max_history)

    def selftest_denoise_variance(self, history, moments, guides, sigma_luminance, sigma_normal, sigma_position, *,
                                  min_history, iterations: int = 5, direct_only: bool = False):
        """The estimate and the filter on caller-supplied buffers (crt_selftest_denoise_variance): history [height,
        width, 4] (r, g, b, len), moments [height, width, 2], guides [height, width, 8].  Returns (the filtered frame
        [height, width, 3], the variance estimate [height, width])."""
        o = self._denoise_variance_options("selftest_denoise_variance", sigma_luminance, sigma_normal, sigma_position,
                                           min_history, iterations, direct_only)
        h = self._flat("selftest_denoise_variance", "history", history, 4)
        m = self._flat("selftest_denoise_variance", "moments", moments, 2)
        g = self._flat("selftest_denoise_variance", "guides", guides, 8)
        out = np.zeros((self.height, self.width, 3), np.float32)
        out_v = np.zeros((self.height, self.width), np.float32)
        check(_lib.require("crt_selftest_denoise_variance")(self.h, _p(h), _p(m), _p(g), C.byref(o), _p(out), _p(out_v)),
              "selftest_denoise_variance")
        return out, out_v

    def set_leaf_carry(self, lanes: int, max_pairs: int):
        """Variant 8's leaf-pair carry: measured and removed in round 5; the library reports
        CRT_ERR_UNSUPPORTED, so this raises CrtError (profiles/r04c/leaf_carry.patch restores the kernels)."""
        check(_lib.hip().crt_renderer_set_leaf_carry(self.h, int(lanes), int(max_pairs)), "set_leaf_carry")

    @staticmethod
    def has_timing_history() -> bool:
        """Whether the loaded library exports crt_renderer_timing_history (ABI >= 3; older base builds in A/B runs)."""
        return hasattr(_lib.hip(), "crt_renderer_timing_history")

    def timing_history(self, back: int) -> dict:
        """last_timings() of an earlier render: back = 0 is the last one, up to 31 (crt_renderer_timing_history)."""
        a = (C.c_float * 3)()
        check(_lib.hip().crt_renderer_timing_history(self.h, int(back), a), "timing_history")
        return {"render_ms": float(a[0]), "probe_sort_ms": float(a[1]), "main_kernel_ms": float(a[2])}

    def last_kernel_ms(self) -> float:
        return float(_lib.hip().crt_renderer_last_kernel_ms(self.h))

    def attach_linear(self, device_ptr: int | None):
        """Render into caller-owned device memory (W*H*3 f32), e.g. a torch tensor to RCCL-reduce."""
        check(_lib.hip().crt_renderer_attach_linear(self.h, C.c_void_p(device_ptr) if device_ptr else None),
              "attach_linear")

    def linear_device_ptr(self) -> int:
        return int(_lib.hip().crt_renderer_linear_device_ptr(self.h) or 0)

    def rng_device_ptr(self) -> int:
        return int(_lib.hip().crt_renderer_rng_device_ptr(self.h) or 0)

    def render_frame(self, scene: Scene, spp: int, max_bounces: int = 20, seed: int = 41, subsequence_base: int = 0,
                     stream=None):
        """Fresh RNG (initRandState) + spp samples + writeColor: one reference frame."""
        self.init_rand(seed, subsequence_base, stream)
        self.render(scene, spp, max_bounces, stream=stream)
        self.resolve(pixel_sample_scale(spp), stream)
        self.synchronize(stream)

    def compare(self, scene_a: Scene, scene_b: Scene, spp: int, max_bounces: int = 20) -> dict:
        """Per-ray hit agreement of two device scenes (crt_scene_compare); paths follow scene_a.
        Call init_rand first; the RNG state is consumed."""
        out = (C.c_uint64 * 5)()
        check(_lib.hip().crt_scene_compare(self.h, scene_a.h, scene_b.h, int(spp), int(max_bounces), out),
              "crt_scene_compare")
        keys = ("rays", "rank_mismatch", "t_mismatch", "b_miss", "a_miss")
        return dict(zip(keys, (int(v) for v in out)))

    def compare_dump(self, scene_a: Scene, scene_b: Scene, spp: int, max_bounces: int = 20, max_dump: int = 256):
        """compare() plus the differing rays: array [n, 10] = o.xyz, d.xyz, rank_a, rank_b (int bits), t_a, t_b."""
        out = (C.c_uint64 * 5)()
        buf = np.zeros((max_dump, 10), np.float32)
        check(_lib.hip().crt_scene_compare_dump(self.h, scene_a.h, scene_b.h, int(spp), int(max_bounces), out,
                                                _p(buf), int(max_dump)), "crt_scene_compare_dump")
        keys = ("rays", "rank_mismatch", "t_mismatch", "b_miss", "a_miss")
        res = dict(zip(keys, (int(v) for v in out)))
        return res, buf[:min(max_dump, res["rank_mismatch"])]


def pixel_sample_scale(spp: int) -> float:
    """m_PixelSampleScale = 1.f / m_SamplesPerPixel (Camera.cuh:23), rounded to f32 (spp 0 gives inf, as in C)."""
    with np.errstate(divide="ignore"):
        return float(np.float32(1.0) / np.float32(spp))


def device_count() -> int:
    n = C.c_int(0)
    check(_lib.hip().crt_device_count(C.byref(n)), "device_count")
    return n.value


KEY_W, KEY_A, KEY_S, KEY_D, KEY_SPACE, KEY_LCONTROL, KEY_F = 1, 2, 4, 8, 16, 32, 64


def _input(mouse_x=0.0, mouse_y=0.0, right_mouse=False, keys=0, focus_steps=0) -> _lib.CrthInput:
    return _lib.CrthInput(float(mouse_x), float(mouse_y), int(bool(right_mouse)), int(keys), int(focus_steps))


class CameraController:
    """CRT::Camera + Camera::updateCamera on the host (crth_camera_*; Camera.cuh:46-157). No GPU."""

    def __init__(self, aspect=16.0 / 9.0, vfov=80.0, pos=(0.0, 4.0, 4.0), up=(0.0, 1.0, 0.0), aperture=0.000001,
                 focus=None):
        pos = np.asarray(pos, np.float32)
        if focus is None:
            focus = float(np.sqrt(np.float32(np.dot(pos, pos))))
        h = C.c_void_p()
        check_host(_lib.host().crth_camera_create(aspect, vfov, _p(pos), _p(np.asarray(up, np.float32)), aperture,
                                                  focus, C.byref(h)), "crth_camera_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None) and _lib is not None:   # None: interpreter exit (see HostScene.__del__)
            _lib.host().crth_camera_destroy(self.h)
            self.h = None

    __del__ = close

    def update(self, dt, ww, wh, **inp):
        check_host(_lib.host().crth_camera_update(self.h, dt, ww, wh, C.byref(_input(**inp))), "crth_camera_update")

    def get(self):
        d = CameraDesc()
        st = np.zeros(6, np.float32)
        check_host(_lib.host().crth_camera_get(self.h, C.byref(d), _p(st)), "crth_camera_get")
        return d, {"yaw": float(st[0]), "pitch": float(st[1]), "moving": bool(st[2]), "rotating": bool(st[3]),
                   "high_quality": bool(st[4]), "focus": float(st[5])}


class Viewer:
    """The reference's Raytracer loop, headless (crth_viewer_*; Raytracer.h:52-102): one frame() per
    updateAndRender with the input the window would have delivered."""

    def __init__(self, obj_files, width, height, device=0, bvh="reference", aspect=16.0 / 9.0, vfov=80.0,
                 aperture=0.000001, pos=None, focus=0.0, seed=41, accumulate=False, bvh_width=0, **scene_kw):
        files = [str(f).encode() for f in obj_files]
        arr = (C.c_char_p * len(files))(*files)
        opts = scene_options(bvh, width=bvh_width, **scene_kw)
        pos_a = None if pos is None else np.asarray(pos, np.float32)
        h = C.c_void_p()
        check_host(_lib.host().crth_viewer_create(arr, len(files), device, C.byref(opts), width, height, aspect, vfov,
                                                  aperture, None if pos_a is None else _p(pos_a), focus, seed,
                                                  int(bool(accumulate)), C.byref(h)), "crth_viewer_create")
        self.h, self.width, self.height, self.device = h, width, height, device
        self.renderer = Renderer._borrow(_lib.host().crth_viewer_renderer(h), width, height, device, self)

    def close(self):
        if getattr(self, "h", None) and _lib is not None:   # None: interpreter exit (see HostScene.__del__)
            self.renderer.h = None
            _lib.host().crth_viewer_destroy(self.h)
            self.h = None

    __del__ = close

    def frame(self, dt=1.0 / 60.0, **inp) -> dict:
        fi = _lib.CrthFrameInfo()
        check_host(_lib.host().crth_viewer_frame(self.h, dt, C.byref(_input(**inp)), C.byref(fi)), "crth_viewer_frame")
        return {"frame": fi.frame, "spp": fi.spp, "accumulated": fi.accumulated, "moving": bool(fi.moving),
                "high_quality": bool(fi.high_quality), "kernel_ms": fi.kernel_ms, "frame_ms": fi.frame_ms}

    def set_reproject(self, position_tolerance=None, normal_min=float("-inf"), *, max_history=None, denoise=None,
                      denoise_iterations: int = 5):
        """The reproject mode (crth_viewer_set_reproject): after each frame's render the viewer computes the guides,
        runs Renderer.reproject with these options and the frame's pixel_sample_scale and resolves the history; with
        denoise = (sigma_color, sigma_normal, sigma_position) it filters the history first (Renderer.denoise_history)
        and resolves that.  position_tolerance None switches the mode off and resets the history.  Not together with
        accumulate."""
        if position_tolerance is None:
            check_host(_lib.host().crth_viewer_set_reproject(self.h, None, None), "crth_viewer_set_reproject")
            return
        o = Renderer._reproject_options("set_reproject", position_tolerance, normal_min, max_history)
        d = None
        if denoise is not None:
            try:
                sc, sn, sx = denoise
            except (TypeError, ValueError):
                raise ValueError("set_reproject: denoise must be (sigma_color, sigma_normal, sigma_position)") from None
            d = Renderer._denoise_options("set_reproject", sc, sn, sx, denoise_iterations, False, False)
        check_host(_lib.host().crth_viewer_set_reproject(self.h, C.byref(o), None if d is None else C.byref(d)),
                   "crth_viewer_set_reproject")

    def set_denoise_variance(self, sigma_luminance=None, sigma_normal=None, sigma_position=None, *, min_history=None,
                             iterations: int = 5):
        """The variance-guided filter of the reproject mode (crth_viewer_set_denoise_variance): each frame's chain
        becomes render, guides, Renderer.reproject_moments, Renderer.denoise_history_variance with these options,
        resolve_denoised.  It needs set_reproject() before it, without that call's denoise.  sigma_luminance None
        switches it off."""
        if sigma_luminance is None:
            check_host(_lib.host().crth_viewer_set_denoise_variance(self.h, None), "crth_viewer_set_denoise_variance")
            return
        d = Renderer._denoise_variance_options("set_denoise_variance", sigma_luminance, sigma_normal, sigma_position,
                                               min_history, iterations, False)
        check_host(_lib.host().crth_viewer_set_denoise_variance(self.h, C.byref(d)), "crth_viewer_set_denoise_variance")

    def camera(self) -> CameraDesc:
        d = CameraDesc()
        check_host(_lib.host().crth_viewer_camera(self.h, C.byref(d)), "crth_viewer_camera")
        return d


IMAGE_FORMATS = {"ppm": 0, "png": 1}


def encode_image(rgba: np.ndarray, fmt: str = "png", flip: bool = True) -> bytes:
    """PNG/PPM bytes of an (H, W, 4) uint8 framebuffer (row 0 = bottom, as the renderer holds it);
    flip=True writes the top row first, like WindowManager::drawFrame (WindowManager.h:79-93)."""
    a = np.ascontiguousarray(rgba, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise CrtError("rgba must be (H, W, 4) uint8")
    h, w = a.shape[:2]
    n = C.c_uint64(0)
    L = _lib.host()
    check_host(L.crth_encode_image(IMAGE_FORMATS[fmt], _p(a), w, h, int(flip), None, C.byref(n)), "crth_encode_image")
    out = np.empty(n.value, np.uint8)
    check_host(L.crth_encode_image(IMAGE_FORMATS[fmt], _p(a), w, h, int(flip), _p(out), C.byref(n)), "crth_encode_image")
    return out[: n.value].tobytes()


def write_image(path: str, rgba: np.ndarray, flip: bool = True) -> None:
    """Write .png / .ppm by extension (crth_write_image)."""
    a = np.ascontiguousarray(rgba, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise CrtError("rgba must be (H, W, 4) uint8")
    check_host(_lib.host().crth_write_image(str(path).encode(), _p(a), a.shape[1], a.shape[0], int(flip)),
               "crth_write_image")


NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("left", "<i4"), ("right", "<i4"),
                       ("obj_index", "<i4"), ("obj_count", "<i4"), ("is_leaf", "<i4")])   # crt_bvh_node_desc


def build_mesh_bvh(positions, indices, face_materials, device=None):
    """Mesh::buildBVHMesh + Mesh ctor box (Mesh.cuh:39-47, :121-264) on one mesh.

    device=None: the sequential host restatement (crth_build_mesh_bvh); device=k: the GPU-parallel build
    on device k (crt_build_mesh_bvh).  Returns (nodes [NODE_DTYPE], permuted indices, permuted face
    materials, mesh box (6,), device ms or None).  Raises CrtError; a GPU build that must defer to the
    host builder raises with status CRT_ERR_UNSUPPORTED (-5)."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1)
    idx = np.ascontiguousarray(indices, np.uint32).copy()
    fm = np.ascontiguousarray(face_materials, np.int32).copy()
    n_tri = len(idx) // 3
    nodes = np.zeros(max(1, 2 * n_tri - 1), NODE_DTYPE)
    cnt = C.c_int32(0)
    box = np.zeros(6, np.float32)
    if device is None:
        rc = _lib.host().crth_build_mesh_bvh(_p(pos), len(pos) // 3, _p(idx), _p(fm), len(idx), _p(nodes),
                                             C.byref(cnt), _p(box))
        check_host(rc, "crth_build_mesh_bvh")
        ms = None
    else:
        t = C.c_float(0)
        rc = _lib.hip().crt_build_mesh_bvh(int(device), _p(pos), len(pos) // 3, _p(idx), _p(fm), len(idx), _p(nodes),
                                           C.byref(cnt), _p(box), C.byref(t))
        if rc != 0:
            err = CrtError(f"crt_build_mesh_bvh failed (status {rc}): "
                           f"{_lib.hip().crt_last_error().decode(errors='replace')}")
            err.status = rc
            raise err
        ms = t.value
    return nodes[:cnt.value], idx, fm, box, ms


from . import paths  # noqa: E402  (path steps: camera_rays, Scene.path_step, the wavefront driver paths.render)
from .paths import camera_rays  # noqa: E402
