"""ctypes bindings of the two C ABIs (include/crt_hip.h, include/crt_host.h).

The shared libraries are built in-tree (raytracer-cuda_amd/lib/) by `make`; this
module never falls back to anything else: if libcrt_hip.so is missing or does not
load, every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parents[1]          # raytracer-cuda_amd/
REPO = PKG_ROOT.parent
LIB_DIR = PKG_ROOT / "lib"
# CRT_HIP_LIB: an alternative build of the same library (A/B profiling builds, tools/); default in-tree
HIP_LIB = Path(os.environ["CRT_HIP_LIB"]) if os.environ.get("CRT_HIP_LIB") else LIB_DIR / "libcrt_hip.so"
# CRT_HOST_LIB: an alternative build of the host library (the sanitizer build, `make asan`, tools/run_asan.sh)
HOST_LIB = Path(os.environ["CRT_HOST_LIB"]) if os.environ.get("CRT_HOST_LIB") else LIB_DIR / "libcrt_host.so"


class CrtError(RuntimeError):
    pass


def build(jobs: int = 8) -> None:
    """Compile libcrt_hip.so (gfx950) + libcrt_host.so + crt_render in-tree."""
    subprocess.run(["make", "-C", str(PKG_ROOT), f"-j{jobs}", "all"], check=True)


class CameraDesc(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("lower_left", C.c_float * 3), ("horizontal", C.c_float * 3),
                ("vertical", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("lens_radius", C.c_float), ("samples_per_pixel", C.c_int32), ("pixel_sample_scale", C.c_float)]


class CrthInput(C.Structure):        # crt_host.h crth_input
    _fields_ = [("mouse_x", C.c_float), ("mouse_y", C.c_float), ("right_mouse", C.c_int32), ("keys", C.c_uint32),
                ("focus_steps", C.c_int32)]


class CrthFrameInfo(C.Structure):    # crt_host.h crth_frame_info
    _fields_ = [("frame", C.c_int64), ("spp", C.c_int32), ("accumulated", C.c_int32), ("moving", C.c_int32),
                ("high_quality", C.c_int32), ("kernel_ms", C.c_float), ("frame_ms", C.c_double)]


class SceneDesc(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("n_positions", C.c_uint64), ("indices", C.c_void_p),
                ("n_indices", C.c_uint64), ("face_materials", C.c_void_p), ("n_faces", C.c_uint64),
                ("meshes", C.c_void_p), ("n_meshes", C.c_int32), ("spheres", C.c_void_p), ("n_spheres", C.c_int32),
                ("objects", C.c_void_p), ("n_objects", C.c_int32), ("scene_nodes", C.c_void_p),
                ("n_scene_nodes", C.c_int32), ("materials", C.c_void_p), ("n_materials", C.c_int32)]


class BvhNodeDesc(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("left", C.c_int32), ("right", C.c_int32),
                ("obj_index", C.c_int32), ("obj_count", C.c_int32), ("is_leaf", C.c_int32)]


class MeshDesc(C.Structure):
    _fields_ = [("vertex_offset", C.c_uint32), ("vertex_count", C.c_uint32), ("index_offset", C.c_uint32),
                ("index_count", C.c_uint32), ("face_offset", C.c_uint32), ("material_id_offset", C.c_uint32),
                ("nodes", C.c_void_p), ("node_count", C.c_int32), ("aabb", C.c_float * 6)]


class MaterialDesc(C.Structure):      # crt_hip.h crt_material_desc
    _fields_ = [("type", C.c_int32), ("albedo", C.c_float * 3), ("emission", C.c_float * 3), ("roughness", C.c_float),
                ("ior", C.c_float)]


class SceneStats(C.Structure):
    _fields_ = [("device_nodes", C.c_int64), ("device_prims", C.c_int64), ("device_bytes", C.c_int64),
                ("max_depth", C.c_int32), ("n_materials", C.c_int32), ("bvh", C.c_int32), ("layouts", C.c_int32),
                ("excluded_prims", C.c_int64), ("width", C.c_int32), ("stack_bound", C.c_int32),
                ("spatial_splits", C.c_int64), ("references", C.c_int64)]


class SceneOptions(C.Structure):
    _fields_ = [("bvh", C.c_int32), ("leaf_size", C.c_int32), ("layouts", C.c_int32),
                ("traversal_cost", C.c_float), ("width", C.c_int32), ("gpu_build", C.c_int32),
                ("stack_cap", C.c_int32), ("spatial_splits", C.c_int32),
                ("spatial_alpha", C.c_float), ("spatial_max_dup", C.c_float)]


BVH_REFERENCE = 0
BVH_REBUILT = 1
ABI_VERSION = 3          # include/crt_hip.h CRT_ABI_VERSION
BUILD_CHECKED = 1        # crt_build_flags(): the -DCRT_CHECKED build


class WorkCounters(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("box_tests", C.c_uint64), ("tri_tests", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("paths", C.c_uint64)]


class Ray(C.Structure):              # crt_hip.h crt_ray: two 16-B rows
    _fields_ = [("origin", C.c_float * 3), ("tmax", C.c_float), ("dir", C.c_float * 3), ("reserved", C.c_float)]


class Hit(C.Structure):              # crt_hip.h crt_hit: two 16-B rows
    _fields_ = [("t", C.c_float), ("object", C.c_int32), ("primitive", C.c_int32), ("material", C.c_int32),
                ("normal", C.c_float * 3), ("front_face", C.c_int32)]


class TraceOptions(C.Structure):     # crt_hip.h crt_trace_options
    _fields_ = [("mode", C.c_int32), ("grid_waves", C.c_int32), ("stack_lds", C.c_int32),
                ("refill_threshold", C.c_int32)]


class TraceStats(C.Structure):       # crt_hip.h crt_trace_stats
    _fields_ = [("kernel_ms", C.c_float), ("rays", C.c_uint64), ("box_tests", C.c_uint64), ("tri_tests", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("step_lane_slots", C.c_uint64), ("step_active_lanes", C.c_uint64)]


TRACE_COUNT_WORK = 1     # crt_scene_trace_device flags


class Path(C.Structure):             # crt_hip.h crt_path: two 16-B rows
    _fields_ = [("throughput", C.c_float * 3), ("bounce", C.c_int32), ("pixel", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32 * 2)]


PATH_ACTIVE, PATH_ENDED = 0, 1       # crt_path.status


class WavefrontStats(C.Structure):   # crt_hip.h crt_wavefront_stats
    _fields_ = [("rays", C.c_uint64), ("iterations", C.c_uint32), ("ms", C.c_float)]


class AdaptiveOptions(C.Structure):  # crt_hip.h crt_adaptive_options
    _fields_ = [("spp_min", C.c_int32), ("spp_max", C.c_int32), ("tolerance", C.c_float), ("reserved", C.c_int32)]


class AdaptiveStats(C.Structure):    # crt_hip.h crt_adaptive_stats
    _fields_ = [("samples", C.c_uint64), ("passes", C.c_uint32), ("tiles_refined", C.c_uint32),
                ("tiles_at_max", C.c_uint32), ("ms", C.c_float)]


class DenoiseOptions(C.Structure):   # crt_hip.h crt_denoise_options
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_int32)]


class DenoiseStats(C.Structure):     # crt_hip.h crt_denoise_stats
    _fields_ = [("guides_ms", C.c_float), ("filter_ms", C.c_float), ("iterations", C.c_uint32),
                ("pixels_hit", C.c_uint32)]


class ReprojectOptions(C.Structure):  # crt_hip.h crt_reproject_options
    _fields_ = [("position_tolerance", C.c_float), ("normal_min", C.c_float), ("max_history", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_int32)]


class ReprojectStats(C.Structure):    # crt_hip.h crt_reproject_stats
    _fields_ = [("reproject_ms", C.c_float), ("pixels_reprojected", C.c_uint32), ("pixels_hit", C.c_uint32)]


class DenoiseVarianceOptions(C.Structure):   # crt_hip.h crt_denoise_variance_options
    _fields_ = [("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float), ("min_history", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_int32)]


DENOISE_TILE_SCALE = 1               # crt_denoise_options.flags
DENOISE_DIRECT_ONLY = 0x80000000     # measurement switch: every iteration through the direct kernel

_P, _i32, _u32, _i64, _u64, _f32 = C.c_void_p, C.c_int, C.c_uint32, C.c_int64, C.c_ulonglong, C.c_float

# Every entry of libcrt_hip.so, named here and nowhere else: name -> (argtypes, restype, optional).  hip() binds from this
# table and the exported symbol lists below are read off it (tests check them against include/*.h).  optional: the entry
# joined ABI version 3 after its first release (the path steps, the path queues, the indirect calls, the schedule
# self-tests, the path finish, adaptive sampling, the denoiser, the live-allocation count, which twin of a variant-8 kernel
# ran, the reprojection, variant 8's tail fill, the material self-test, the variance-guided filter): bound when the loaded
# library has it, so an older build of the same ABI still loads; its Python front-end raises CrtError through require().
HIP_SIG = {
    "crt_abi_version": ([], _i32, False),
    "crt_build_flags": ([], _i32, False),
    "crt_last_error": ([], C.c_char_p, False),
    "crt_device_count": ([_P], _i32, False),
    "crt_scene_create": ([_P, _i32, _P], _i32, False),
    "crt_scene_create_ex": ([_P, _i32, _P, _P], _i32, False),
    "crt_scene_get_stats": ([_P, _P], _i32, False),
    "crt_scene_compare": ([_P, _P, _P, _i32, _i32, _P], _i32, False),
    "crt_scene_compare_dump": ([_P, _P, _P, _i32, _i32, _P, _P, _i32], _i32, False),
    "crt_scene_export": ([_P, _P, _P, _P, _P, _P], _i32, False),
    "crt_renderer_set_stack_lds": ([_P, _i32], _i32, False),
    "crt_renderer_get_section_profile": ([_P, _P], _i32, False),
    "crt_renderer_get_section_profile_ex": ([_P, _P, _i32], _i32, False),
    "crt_scene_destroy": ([_P], None, False),
    "crt_renderer_create": ([_i32, _i32, _i32, _P], _i32, False),
    "crt_renderer_destroy": ([_P], None, False),
    "crt_renderer_init_rand": ([_P, _u64, _u64, _P], _i32, False),
    "crt_renderer_set_camera": ([_P, _P], _i32, False),
    "crt_renderer_render": ([_P, _P, _i32, _i32, C.c_uint, _P], _i32, False),
    "crt_renderer_resolve": ([_P, _f32, _P], _i32, False),
    "crt_renderer_render_frame": ([_P, _P, _P], _i32, False),
    "crt_renderer_synchronize": ([_P, _P], _i32, False),
    "crt_renderer_read_linear": ([_P, _P], _i32, False),
    "crt_renderer_read_rgba8": ([_P, _P], _i32, False),
    "crt_renderer_read_rng": ([_P, _P], _i32, False),
    "crt_renderer_write_linear": ([_P, _P], _i32, False),
    "crt_renderer_get_counters": ([_P, _P], _i32, False),
    "crt_renderer_linear_device_ptr": ([_P], _P, False),
    "crt_renderer_rgba_device_ptr": ([_P], _P, False),
    "crt_renderer_rng_device_ptr": ([_P], _P, False),
    "crt_renderer_last_kernel_ms": ([_P], _f32, False),
    "crt_renderer_last_kernel_name": ([_P], C.c_char_p, False),
    "crt_renderer_last_timings": ([_P, _P], _i32, False),
    "crt_renderer_last_schedule": ([_P, _P], _i32, False),
    "crt_renderer_timing_history": ([_P, _i32, _P], _i32, False),
    "crt_renderer_set_leaf_carry": ([_P, _i32, _i32], _i32, False),
    "crt_renderer_set_xcd_regions": ([_P, _i32], _i32, False),
    "crt_renderer_set_temporal_order": ([_P, _i32], _i32, False),
    "crt_renderer_set_drain_threshold": ([_P, _i32], _i32, False),
    "crt_renderer_set_wave_drain": ([_P, _i32], _i32, False),
    "crt_renderer_attach_linear": ([_P, _P], _i32, False),
    "crt_renderer_set_kernel_variant": ([_P, _i32], _i32, False),
    "crt_renderer_get_schedule_stats": ([_P, _P], _i32, False),
    "crt_renderer_set_regen_threshold": ([_P, _i32], _i32, False),
    "crt_renderer_set_occupancy_target": ([_P, _i32], _i32, False),
    "crt_build_mesh_bvh": ([_i32, _P, _u32, _P, _P, _u32, _P, _P, _P, _P], _i32, False),
    "crt_renderer_set_schedule": ([_P, _i32, _i32, _i32], _i32, False),
    "crt_renderer_set_critical_tiles": ([_P, _i32, _i32], _i32, False),
    "crt_renderer_set_pixel_shard": ([_P, _i32, _i32], _i32, False),
    "crt_renderer_set_top_levels": ([_P, _i32], _i32, False),
    "crt_selftest_math": ([_P, _P, _i32, _P, _P], _i32, False),
    "crt_selftest_rng": ([_u64, _P, _i32, _i32, _P, _P], _i32, False),
    "crt_selftest_geometry": ([_i32, _P, _i32, _P, _i32, _i32, _P, _P], _i32, False),
    "crt_selftest_scan": ([_P, _i32, _P], _i32, False),
    "crt_selftest_rcp": ([_u32, _u32, _P, _P], _i32, False),
    "crt_selftest_uv_div": ([_i32, _P], _i32, False),
    "crt_selftest_sqrt": ([_u32, _u32, _P, _P], _i32, False),
    "crt_selftest_unit": ([_P, _i32, _P], _i32, False),
    "crt_trace_validate_rays": ([_P, _i64, _P], _i32, False),
    "crt_scene_export_identity": ([_P, _P, _P, _P], _i32, False),
    "crt_scene_trace": ([_P, _P, _i64, _P, _P], _i32, False),
    "crt_scene_occluded": ([_P, _P, _i64, _P, _P], _i32, False),
    "crt_scene_trace_device": ([_P, _P, _i64, _P, _P, _P, C.c_uint, _P], _i32, False),
    "crt_scene_trace_last_stats": ([_P, _P], _i32, False),
    "crt_renderer_camera_rays_device": ([_P, _P, _i64, _P, _P, _P, _P], _i32, True),
    "crt_scene_path_step_device": ([_P, _P, _P, _P, _i64, _i32, _P, _P, _i64, _P], _i32, True),
    "crt_scene_export_shade_rows": ([_P, _P, _P], _i32, True),
    "crt_scene_path_advance_device": ([_P, _P, _P, _P, _P, _i64, _i32, _P, _P, _P, _P, _P, _P, _P], _i32, True),
    "crt_path_advance_entries": ([], _i32, True),
    "crt_renderer_render_wavefront": ([_P, _P, _i32, _i32, C.c_uint, _P, _P, _P], _i32, True),
    "crt_scene_trace_indirect_device": ([_P, _P, _P, _i64, _P, _P, _P, C.c_uint, _P], _i32, True),
    "crt_scene_path_advance_indirect_device": ([_P, _P, _P, _P, _P, _P, _i64, _i32, _P, _P, _P, _P, _P, _P, _P, _P], _i32, True),
    "crt_renderer_render_wavefront_queued": ([_P, _P, _i32, _i32, C.c_uint, _P, _i32, _P, _P], _i32, True),
    "crt_scene_path_finish_device": ([_P, _P, _P, _P, _P, _i64, _i32, _P, _P, _P, _P, _P], _i32, True),
    "crt_renderer_render_wavefront_finish": ([_P, _P, _i32, _i32, C.c_uint, _P, _i32, _i64, _P, _P], _i32, True),
    "crt_selftest_tile_schedule": ([_P, _P, _i32, _i32, _i32, _i32, _i32, _P], _i32, True),
    "crt_selftest_pixel_order": ([_P, _i32, _P, _i32, _i32], _i32, True),
    "crt_selftest_schedule_buffer": ([_P, _i32, _P, _i64, _P], _i32, True),
    "crt_renderer_render_adaptive": ([_P, _P, _P, _i32, C.c_uint, _P, _P], _i32, True),
    "crt_renderer_resolve_adaptive": ([_P, _P], _i32, True),
    "crt_renderer_read_tile_spp": ([_P, _P], _i32, True),
    "crt_renderer_read_tile_error": ([_P, _P], _i32, True),
    "crt_renderer_read_adaptive_prev": ([_P, _P], _i32, True),
    "crt_selftest_adaptive_plan": ([_P, _P, _P, _P, _i32, _i32, _f32, _P, _P], _i32, True),
    "crt_renderer_compute_guides": ([_P, _P, _P, _P], _i32, True),
    "crt_renderer_denoise": ([_P, _P, _f32, _P, _P], _i32, True),
    "crt_renderer_resolve_denoised": ([_P, _P], _i32, True),
    "crt_renderer_read_denoised": ([_P, _P], _i32, True),
    "crt_renderer_read_guides": ([_P, _P], _i32, True),
    "crt_renderer_denoised_device_ptr": ([_P], _P, True),
    "crt_selftest_denoise": ([_P, _P, _P, _P, _P], _i32, True),
    "crt_renderer_denoise_iteration_ms": ([_P, _P], _i32, True),
    "crt_debug_live_allocations": ([_P, _P], _i32, True),
    "crt_renderer_last_launch_frozen": ([_P], _i32, True),
    "crt_renderer_reproject": ([_P, _P, _f32, _P, _P], _i32, True),
    "crt_renderer_reset_history": ([_P], _i32, True),
    "crt_renderer_denoise_history": ([_P, _P, _P, _P], _i32, True),
    "crt_renderer_resolve_history": ([_P, _P], _i32, True),
    "crt_renderer_read_history": ([_P, _P], _i32, True),
    "crt_renderer_history_device_ptr": ([_P], _P, True),
    "crt_selftest_reproject": ([_P, _P, _P, _P, _P, _P, _P, _P], _i32, True),
    "crt_renderer_set_tail_fill": ([_P, _i32, _i32], _i32, True),
    "crt_renderer_last_tail_fill": ([_P, _P], _i32, True),
    "crt_selftest_shade": ([_P, _i32, _P], _i32, True),
    "crt_renderer_reproject_moments": ([_P, _P, _f32, _P, _P], _i32, True),
    "crt_renderer_read_moments": ([_P, _P], _i32, True),
    "crt_renderer_denoise_history_variance": ([_P, _P, _P, _P], _i32, True),
    "crt_renderer_read_variance": ([_P, _P], _i32, True),
    "crt_selftest_reproject_moments": ([_P, _P, _P, _P, _P, _P, _P, _P, _P, _P], _i32, True),
    "crt_selftest_denoise_variance": ([_P, _P, _P, _P, _P, _P, _P], _i32, True),
}
HIP_SYMBOLS = list(HIP_SIG)
OPTIONAL_SYMBOLS = tuple(name for name, sig in HIP_SIG.items() if sig[2])

# Every entry of libcrt_host.so: name -> (argtypes, restype).
HOST_SIG = {
    "crth_scene_load": ([_P, _i32, _P], _i32),
    "crth_scene_load_ex": ([_P, _i32, _i32, _P], _i32),
    "crth_scene_build_ms": ([_P], C.c_double),
    "crth_scene_destroy": ([_P], None),
    "crth_scene_desc": ([_P, _P], _i32),
    "crth_scene_upload": ([_P, _i32, _P], _i32),
    "crth_scene_upload_ex": ([_P, _i32, _P, _P], _i32),
    "crth_scene_counts": ([_P, _P], _i32),
    "crth_scene_loader_arrays": ([_P, _P, _P, _P, _P, _P], _i32),
    "crth_camera": ([_f32, _f32, _P, _P, _f32, _f32, _f32, _f32, _i32, _P], _i32),
    "crth_last_error": ([], C.c_char_p),
    "crth_encode_image": ([_i32, _P, _i32, _i32, _i32, _P, _P], _i32),
    "crth_write_image": ([C.c_char_p, _P, _i32, _i32, _i32], _i32),
    "crth_build_mesh_bvh": ([_P, _u32, _P, _P, _u32, _P, _P, _P], _i32),
    "crth_camera_create": ([_f32, _f32, _P, _P, _f32, _f32, _P], _i32),
    "crth_camera_update": ([_P, _f32, _i32, _i32, _P], _i32),
    "crth_camera_get": ([_P, _P, _P], _i32),
    "crth_camera_destroy": ([_P], None),
    "crth_viewer_create": ([_P, _i32, _i32, _P, _i32, _i32, _f32, _f32, _f32, _P, _f32, _u64, _i32, _P], _i32),
    "crth_viewer_frame": ([_P, _f32, _P, _P], _i32),
    "crth_viewer_camera": ([_P, _P], _i32),
    "crth_viewer_renderer": ([_P], _P),
    "crth_viewer_destroy": ([_P], None),
    "crth_viewer_set_reproject": ([_P, _P, _P], _i32),
    "crth_viewer_set_denoise_variance": ([_P, _P], _i32),
}
HOST_SYMBOLS = list(HOST_SIG)

_hip = None
_host = None


def _bind_single_runtime() -> None:
    """Import torch before libcrt_hip.so so the process holds ONE HIP runtime.

    PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64.so.1; once torch is
    loaded, libcrt_hip.so's DT_NEEDED entries resolve to those same objects by SONAME, so
    torch tensors (RCCL framebuffer reduce) and the crt kernels share one device context.
    Set CRT_NO_TORCH=1 to bind the system ROCm runtime instead (no torch interop)."""
    if os.environ.get("CRT_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def _bind(L, table, may_lack=()) -> None:
    """Give L's entries the argtypes and restype of `table`.  Those in `may_lack` may be absent (an older build of this ABI
    version: require() reports one when it is used), and any under CRT_SKIP_ABI_CHECK (an A/B build of an older revision)."""
    any_absent = bool(os.environ.get("CRT_SKIP_ABI_CHECK"))
    for name, sig in table.items():
        if (any_absent or name in may_lack) and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes, fn.restype = sig[0], sig[1]


def hip():
    global _hip
    if _hip is None:
        _bind_single_runtime()
        if not HIP_LIB.exists():
            raise CrtError(f"{HIP_LIB} not built (run `make -C {PKG_ROOT}` or __graft_entry__.build())")
        L = C.CDLL(str(HIP_LIB), mode=C.RTLD_GLOBAL)
        _bind(L, HIP_SIG, OPTIONAL_SYMBOLS)
        # every library is checked, CRT_HIP_LIB overrides included (a stale build would silently misread newer
        # fields); A/B runs against an older revision's build opt out explicitly with CRT_SKIP_ABI_CHECK=1
        if L.crt_abi_version() != ABI_VERSION and not os.environ.get("CRT_SKIP_ABI_CHECK"):
            raise CrtError(f"{HIP_LIB}: C ABI version {L.crt_abi_version()}, these bindings expect {ABI_VERSION} "
                           "(rebuild the library, or set CRT_SKIP_ABI_CHECK=1 for an A/B run of an older build)")
        _hip = L
    return _hip


def host():
    global _host
    if _host is None:
        hip()   # load libcrt_hip.so first (RTLD_GLOBAL) so libcrt_host resolves against the in-tree copy
        if not HOST_LIB.exists():
            raise CrtError(f"{HOST_LIB} not built")
        L = C.CDLL(str(HOST_LIB))
        _bind(L, HOST_SIG)
        _host = L
    return _host


def require(name: str, lib=None):
    """The optional entry `name` of the loaded HIP library (OPTIONAL_SYMBOLS), or CrtError naming it."""
    L = hip() if lib is None else lib
    if not hasattr(L, name):
        raise CrtError(f"{HIP_LIB} does not export {name}: it was built before that entry was added "
                       "(rebuild the library)")
    return getattr(L, name)


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = hip().crt_last_error().decode(errors="replace")
        raise CrtError(f"{what} failed (status {rc}): {msg}")


def check_host(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = host().crth_last_error().decode(errors="replace")
        raise CrtError(f"{what} failed (status {rc}): {msg}")
