"""The C-ABI libraries load and export every symbol include/*.h declares (no GPU needed)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def _declared(header: Path, prefix: str):
    txt = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    names = set(re.findall(r"\b(%s\w+)\s*\(" % prefix, txt))
    return sorted(names)


def _exported(lib: Path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_hip_library_exports_header():
    from crt_amd import _lib
    decl = _declared(REPO / "include" / "crt_hip.h", "crt_")
    exp = _exported(_lib.HIP_LIB)
    missing = [d for d in decl if d not in exp]
    assert not missing, missing
    assert sorted(_lib.HIP_SYMBOLS) == decl
    # only the C ABI is exported
    assert all(s.startswith("crt_") for s in exp if not s.startswith("_")), sorted(exp)[:10]


def test_host_library_exports_header():
    from crt_amd import _lib
    decl = _declared(REPO / "include" / "crt_host.h", "crth_")
    assert not [d for d in decl if d not in _exported(_lib.HOST_LIB)]
    assert sorted(_lib.HOST_SYMBOLS) == decl


# The entries that joined ABI version 3 after its first release: an older build of the same ABI may lack these and no other.
OPTIONAL = {
    "crt_debug_live_allocations", "crt_path_advance_entries", "crt_renderer_camera_rays_device", "crt_renderer_compute_guides",
    "crt_renderer_denoise", "crt_renderer_denoise_history", "crt_renderer_denoise_history_variance",
    "crt_renderer_denoise_iteration_ms", "crt_renderer_denoised_device_ptr", "crt_renderer_history_device_ptr",
    "crt_renderer_last_launch_frozen", "crt_renderer_last_tail_fill", "crt_renderer_read_adaptive_prev",
    "crt_renderer_read_denoised", "crt_renderer_read_guides", "crt_renderer_read_history", "crt_renderer_read_moments",
    "crt_renderer_read_tile_error", "crt_renderer_read_tile_spp", "crt_renderer_read_variance", "crt_renderer_render_adaptive",
    "crt_renderer_render_wavefront", "crt_renderer_render_wavefront_finish", "crt_renderer_render_wavefront_queued",
    "crt_renderer_reproject", "crt_renderer_reproject_moments", "crt_renderer_reset_history", "crt_renderer_resolve_adaptive",
    "crt_renderer_resolve_denoised", "crt_renderer_resolve_history", "crt_renderer_set_tail_fill", "crt_scene_export_shade_rows",
    "crt_scene_path_advance_device", "crt_scene_path_advance_indirect_device", "crt_scene_path_finish_device",
    "crt_scene_path_step_device", "crt_scene_trace_indirect_device", "crt_selftest_adaptive_plan", "crt_selftest_denoise",
    "crt_selftest_denoise_variance", "crt_selftest_pixel_order", "crt_selftest_reproject", "crt_selftest_reproject_moments",
    "crt_selftest_schedule_buffer", "crt_selftest_shade", "crt_selftest_tile_schedule",
}


def test_binding_table_is_the_only_list():
    from crt_amd import _lib
    assert _lib.HIP_SYMBOLS == list(_lib.HIP_SIG) and _lib.HOST_SYMBOLS == list(_lib.HOST_SIG)
    assert set(_lib.OPTIONAL_SYMBOLS) == OPTIONAL and len(_lib.OPTIONAL_SYMBOLS) == len(OPTIONAL)
    for table, fields in ((_lib.HIP_SIG, 3), (_lib.HOST_SIG, 2)):
        for name, sig in table.items():
            assert len(sig) == fields and isinstance(sig[0], list), name
            assert sig[1] is None or isinstance(sig[1], type(C.c_int)), name
    assert all(isinstance(sig[2], bool) for sig in _lib.HIP_SIG.values())


def test_libraries_load_without_gpu():
    from crt_amd import _lib
    L = _lib.hip()
    assert L.crt_abi_version() == 3
    n = C.c_int(-1)
    assert L.crt_device_count(C.byref(n)) == 0 and n.value >= 0
    _lib.host()


def test_timings_need_a_render():
    from crt_amd import _lib
    ms = (C.c_float * 3)()
    assert _lib.hip().crt_renderer_last_timings(None, ms) == -1
    assert _lib.hip().crt_renderer_timing_history(None, 0, ms) == -1
    assert _lib.hip().crt_build_flags() == 0


def test_errors_are_reported_not_thrown():
    import crt_amd
    from crt_amd import _lib
    h = C.c_void_p()
    rc = _lib.hip().crt_renderer_create(0, 10, 0, C.byref(h))
    assert rc == -1 and b"size" in _lib.hip().crt_last_error()
    assert _lib.hip().crt_scene_create(None, 0, C.byref(h)) == -1
    with pytest.raises(crt_amd.CrtError):
        crt_amd._lib.check(-1, "x")


def test_cli_binary_built():
    assert (REPO / "raytracer-cuda_amd" / "bin" / "crt_render").exists()
