"""Which blocks of the regeneration pass a wave issues for disjoint lane sets (profiling build only).

    tools/build_profile_lib.sh sites -DCRT_PROFILE_SITES
    CRT_HIP_LIB=raytracer-cuda_amd/lib_exp/sites/libcrt_hip.so python tools/pass_site_count.py [--spp 256]

A wave instruction costs its issue slot whatever the number of lanes that run it.  With Camera::getRay ahead of the
bounce-limit test and the roulette in next_ray, a pass ran the camera block once for the lanes that came in without a
path and once more, on a second trip of next_ray's loop, for the lanes the limit or the roulette ended; and shade_rec
normalised a vector at one site per material (unit-sphere point, glass direction, sky direction).  The build marks, per
lane and pass, which of these blocks the lane takes (crt_hip.hip, CRT_PROFILE_SITES); variant 8 ballots the marks.  The
lane populations decide the instruction count of either code shape:

    trips of next_ray's loop, camera first  = 1 + [a lane was ended inside next_ray and has samples left]
    camera blocks, camera first             = [entry lane] + [ended lane];   merged: [entry lane or ended lane]
    unit() sites, one per material          = [sphere point] + [glass] + [sky];   shared: [any of the three]

With the per-block VALU of the gfx950 ISA this gives the predicted change in VALU wave-instructions per ray.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "raytracer-cuda_amd")]
import crt_amd  # noqa: E402
from crt_amd import _lib, assets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--w", type=int, default=2560)
ap.add_argument("--h", type=int, default=1440)
ap.add_argument("--spp", type=int, default=256)
ap.add_argument("--scene", default="cornell_bunny")
ap.add_argument("--valu-unit", type=float, default=35.0, help="VALU of one unit() site (len2, sqrt, rcp, 3 mul; ISA)")
ap.add_argument("--valu-camera-fixed", type=float, default=75.0,
                help="VALU of the camera block outside its disk loop (two uniforms, uv_div, lens offset, direction; ISA)")
ap.add_argument("--valu-disk-iter", type=float, default=30.0, help="VALU per unit-disk candidate (ISA)")
ap.add_argument("--disk-iters", type=float, default=2.56, help="wave maximum of disk candidates per block (loop_fusion_count)")
ap.add_argument("--valu-per-ray", type=float, default=41.16, help="VALU wave-instructions per ray (PMC)")
a = ap.parse_args()
L = _lib.hip()
L.crt_profile_site_counts.argtypes = [C.c_void_p, C.c_int]
hs = crt_amd.HostScene(assets.scene_files(a.scene), build_device=0)
sc = hs.upload(0, bvh="rebuilt", width=4, leaf_size=4, traversal_cost=2.0, gpu_build=True)
r = crt_amd.Renderer(a.w, a.h)
r.set_camera(crt_amd.camera(a.spp))
buf = np.zeros(12, np.uint64)
for k in range(2):   # the first frame warms up; the counters are reset before the second
    _lib.check(L.crt_profile_site_counts(buf.ctypes.data_as(C.c_void_p), 1), "crt_profile_site_counts")
    r.init_rand(41, 0)
    r.render(sc, a.spp, 20)
    r.synchronize()
_lib.check(L.crt_profile_site_counts(buf.ctypes.data_as(C.c_void_p), 1), "crt_profile_site_counts")
passes, entry, killed, both, ruv, glass, sky, refl, any_unit, n_unit, parked, cam_lanes = (int(v) for v in buf)
rays = r.counters()["rays"]
camera = a.valu_camera_fixed + a.valu_disk_iter * a.disk_iters
saved_cam = both * camera
saved_unit = (n_unit - any_unit) * a.valu_unit
print(json.dumps({
    "kernel": r.last_kernel_name(), "w": a.w, "h": a.h, "spp": a.spp, "scene": a.scene, "rays": rays,
    "passes": passes, "rays_per_pass": round(rays / passes, 2), "parked_lanes_per_pass": round(parked / passes, 2),
    "camera_lanes_per_pass": round(cam_lanes / passes, 2),
    "next_ray_per_pass": {"trips_camera_first": round(1 + killed / passes, 4), "trips_merged": 1.0,
                          "passes_with_entry_lane": round(entry / passes, 4),
                          "passes_with_ended_lane": round(killed / passes, 4),
                          "camera_blocks_camera_first": round((entry + killed) / passes, 4),
                          "camera_blocks_merged": round((entry + killed - both) / passes, 4)},
    "unit_sites_per_pass": {"sphere_point": round(ruv / passes, 4), "glass": round(glass / passes, 4),
                            "sky": round(sky / passes, 4), "metal_reflection": round(refl / passes, 4),
                            "one_per_material": round(n_unit / passes, 4), "shared": round(any_unit / passes, 4)},
    "valu_per_block": {"camera": round(camera, 1), "unit": a.valu_unit},
    "predicted_valu_saved_per_pass": {"camera": round(saved_cam / passes, 1), "unit": round(saved_unit / passes, 1)},
    "predicted_valu_saved_per_ray": {"camera": round(saved_cam / rays, 3), "unit": round(saved_unit / rays, 3),
                                     "total": round((saved_cam + saved_unit) / rays, 3),
                                     "share_of_kernel": round((saved_cam + saved_unit) / rays / a.valu_per_ray, 4)},
    "note": "static per-block VALU from the ISA; the roulette test and the lane masks the merged shape adds are not "
            "counted, nor are the instructions the compiler moves between blocks"}))
