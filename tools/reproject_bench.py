"""The reprojection (Renderer.reproject / denoise_history): what it costs and what it buys.

    python tools/reproject_bench.py [--rows timing,viewer,quality] [--sizes 1280x720,2560x1440] [--reps 7] [--warmup 3]
                                    [--quality-size 1280x720] [--frames 240] [--parent-viewer PATH] [--bounces 20]

No pass / fail: JSON lines.  Scene: cornell_bunny, rebuilt 4-wide tree, default options, bench camera, seed 41.
Camera paths of this tool: still = the bench camera; orbit = yaw -90 + 5 sin(2 pi k / 64), pitch 3 (1 - cos(2 pi k / 64))
degrees at frame k (about half a degree per frame where it is fastest; a pure rotation, like crt_viewer's orbit script:
every ray through the camera's origin keeps its radiance, so nothing the first hit does not describe can lag); strafe =
the bench camera moved sideways to x = 0.2 sin(2 pi k / 64) (parallax: disocclusions, and what glass and mirrors show
changes under a first hit that stays).

  timing   a device-to-device copy rate measured in this process (torch, a 256 MiB buffer: bytes read + bytes written per
           second); per size and path, after a warm-up, `reps` frames of render(1), compute_guides, reproject,
           denoise_history(5 iterations): each step's HIP-event time, medians with minimum and maximum; the
           reprojection with the normal term off and on beside its byte floor over that rate (per pixel: sum 12, current
           guides 32, previous (position, key) rows 16, with the normal term the previous normal rows 16 more, history 16
           read and 16 written; keeping the previous guides costs nothing: two buffers behind an index).
  viewer   crt_viewer's fps over `frames` frames, scripts still and orbit, per size: without the mode, with -reproject,
           with -reproject -denoise, and (--parent-viewer: the parent revision's crt_viewer beside its own libraries)
           the parent without the mode; the runs interleaved, `reps` of each.
  quality  at --quality-size, per path (orbit, strafe), RMS error on linear values against a 1,024-spp frame (seed 1234)
           of the path's last camera after 32 frames: the raw last frame, the history and the filtered history (4.0, inf,
           0.05, 5 iterations) for max_history 8 / 32 / 128 and three tolerances; for one of them the error split by
           guide key (which object the first hit is) and by history length (pixels that restarted in the last frames),
           and the same split for 32 frames of that last camera standing still (what the history is worth where nothing
           moves: the difference per key is what the motion costs).
"""
import argparse
import json
import math
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO / "raytracer-cuda_amd", REPO / "oracle"):
    sys.path.insert(0, str(p))

INF = float("inf")
SIGMAS = (4.0, INF, 0.05)
CAPS = (8.0, 32.0, 128.0)
TOLERANCES = (0.01, 0.05, 0.25)
VIEWER = REPO / "raytracer-cuda_amd" / "bin" / "crt_viewer"


def spread(v, key="ms"):
    return {f"{key}_median": round(statistics.median(v), 4), f"{key}_min": round(min(v), 4), f"{key}_max": round(max(v), 4)}


def size(text):
    w, h = text.split("x")
    return int(w), int(h)


def pose(path, k):
    if path == "still":
        return {}
    a = 2 * math.pi * k / 64
    if path == "strafe":
        return {"pos": (0.2 * math.sin(a), 0.0, 0.3)}
    return {"yaw": -90.0 + 5.0 * math.sin(a), "pitch": 3.0 * (1.0 - math.cos(a))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", default="timing,viewer,quality")
    ap.add_argument("--sizes", default="1280x720,2560x1440")
    ap.add_argument("--quality-size", default="1280x720")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--parent-viewer", default=None)
    ap.add_argument("--bounces", type=int, default=20)
    a = ap.parse_args()
    want = set(a.rows.split(","))

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("reproject_bench: no GPU; nothing here can be measured without one")
    import crt_amd
    from crt_amd import assets
    files = assets.scene_files("cornell_bunny")
    case = {"scene": "cornell_bunny", "bvh": "rebuilt4", "bounces": a.bounces}

    if "timing" in want or "quality" in want:
        hs = crt_amd.HostScene(files)
        sc = hs.upload(0, bvh="rebuilt", width=4)

    def frame_of(r, path, k, tol, nmin, cap):
        r.set_camera(crt_amd.camera(1, **pose(path, k)))
        r.render(sc, 1, a.bounces)
        r.compute_guides(sc)
        return r.reproject(tol, nmin, max_history=cap, scale=1.0)

    if "timing" in want:
        n = 256 << 20
        src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        copy_ms = []
        for k in range(a.warmup + a.reps):
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                copy_ms.append(ev[0].elapsed_time(ev[1]))
        rate = 2 * n / (statistics.median(copy_ms) * 1e-3)
        print(json.dumps(dict(case, row="copy", bytes=n, reps=a.reps, **spread(copy_ms),
                              traffic_gb_per_s=round(rate / 1e9, 1))), flush=True)
        del src, dst
        for w, h in map(size, a.sizes.split(",")):
            for path in ("still", "orbit"):
                for nmin, bytes_per_pixel in ((-INF, 92), (0.9, 108)):
                    r = crt_amd.Renderer(w, h)
                    r.init_rand(41)
                    t = {k: [] for k in ("render", "guides", "reproject", "filter")}
                    taken = hit = 0
                    for k in range(a.warmup + a.reps):
                        s = frame_of(r, path, k, 0.05, nmin, 32.0)
                        f = r.denoise_history(*SIGMAS, iterations=5)
                        if k >= a.warmup:
                            t["render"].append(r.last_kernel_ms())
                            t["guides"].append(f["guides_ms"])
                            t["reproject"].append(s["reproject_ms"])
                            t["filter"].append(f["filter_ms"])
                            taken, hit = s["pixels_reprojected"], s["pixels_hit"]
                    floor_ms = bytes_per_pixel * w * h / rate * 1e3
                    med = {k: statistics.median(v) for k, v in t.items()}
                    print(json.dumps(dict(case, row="timing", width=w, height=h, path=path, normal_term=nmin != -INF,
                                          reps=a.reps, **{k: spread(v) for k, v in t.items()},
                                          floor_bytes_per_pixel=bytes_per_pixel, floor_ms=round(floor_ms, 4),
                                          reproject_over_floor=round(med["reproject"] / floor_ms, 2),
                                          added_ms=round(med["guides"] + med["reproject"] + med["filter"], 4),
                                          added_over_render=round((med["guides"] + med["reproject"] + med["filter"])
                                                                  / med["render"], 3),
                                          pixels_reprojected=taken, pixels_hit=hit)), flush=True)
                    r.close()

    if "viewer" in want:
        modes = {"plain": [], "reproject": ["-reproject", "0.05:-inf:32"],
                 "reproject_denoise": ["-reproject", "0.05:-inf:32", "-denoise", "4:inf:0.05"]}
        programs = [(name, VIEWER, extra) for name, extra in modes.items()]
        if a.parent_viewer:
            programs.append(("parent_plain", Path(a.parent_viewer), []))
        for w, h in map(size, a.sizes.split(",")):
            for script in ("still", "orbit"):
                fps = {name: [] for name, _, _ in programs}
                extra_keys = {}
                for _ in range(a.reps):
                    for name, exe, extra in programs:
                        p = subprocess.run([str(exe), "-w", str(w), "-h", str(h), "-frames", str(a.frames), "-script", script,
                                            "-bvh", "rebuilt", *extra, *map(str, files)], capture_output=True, text=True,
                                           timeout=300)
                        if p.returncode != 0:
                            raise SystemExit(f"{exe} failed: {p.stderr[-500:]}")
                        info = json.loads(p.stdout.strip().splitlines()[-1])
                        fps[name].append(info["fps"])
                        extra_keys[name] = {k: info[k] for k in ("guides_ms_mean", "reproject_ms_mean", "filter_ms_mean",
                                                                 "kernel_ms_mean") if k in info}
                row = dict(case, row="viewer", width=w, height=h, script=script, frames=a.frames, reps=a.reps)
                for name in fps:
                    row[name] = dict(spread(fps[name], "fps"), **extra_keys[name])
                if "parent_plain" in fps:
                    lo, hi = min(fps["parent_plain"]), max(fps["parent_plain"])
                    med = statistics.median(fps["plain"])
                    row["parent_spread_fps"] = round(hi - lo, 1)
                    row["plain_median_minus_parent_median"] = round(med - statistics.median(fps["parent_plain"]), 1)
                    row["plain_within_parent_spread"] = bool(abs(med - statistics.median(fps["parent_plain"])) <= hi - lo)
                print(json.dumps(row), flush=True)

    if "quality" in want:
        w, h = size(a.quality_size)
        frames = 32
        r = crt_amd.Renderer(w, h)
        for path in ("orbit", "strafe"):
            last = crt_amd.camera(1, **pose(path, frames - 1))
            r.set_camera(last)
            r.init_rand(1234)
            r.render(sc, 1024, a.bounces)
            r.synchronize()
            ref = r.linear().astype(np.float64) / 1024

            def rms(img, mask=None):
                d = (img.astype(np.float64) - ref) ** 2
                return float(np.sqrt(np.mean(d if mask is None else d[mask])))

            def split(row, raw, hist, filt):
                key = r.guides().view(np.int32)[..., 7]
                for k in np.unique(key):
                    m = key == k
                    print(json.dumps(dict(row, row=row["row"] + "_by_key", key=int(k), pixels=int(m.sum()),
                                          raw_rms=round(rms(raw, m), 5), history_rms=round(rms(hist[..., 0:3], m), 5),
                                          filtered_history_rms=round(rms(filt, m), 5),
                                          mean_len=round(float(hist[..., 3][m].mean()), 2))), flush=True)
                for name, m in (("len_below_4", hist[..., 3] < 4), ("len_4_and_more", hist[..., 3] >= 4)):
                    if m.any():
                        print(json.dumps(dict(row, row=row["row"] + "_by_len", pixels_with=name, pixels=int(m.sum()),
                                              raw_rms=round(rms(raw, m), 5), history_rms=round(rms(hist[..., 0:3], m), 5),
                                              filtered_history_rms=round(rms(filt, m), 5))), flush=True)

            for cap in CAPS:
                for tol in TOLERANCES:
                    r.reset_history()
                    r.init_rand(41)
                    for k in range(frames):
                        s = frame_of(r, path, k, tol, -INF, cap)
                    r.denoise_history(*SIGMAS, iterations=5)
                    raw, hist, filt = r.linear(), r.history(), r.denoised()
                    row = dict(case, row="quality", path=path, width=w, height=h, frames=frames, max_history=cap,
                               position_tolerance=tol)
                    print(json.dumps(dict(row, raw_rms=round(rms(raw), 5), history_rms=round(rms(hist[..., 0:3]), 5),
                                          filtered_history_rms=round(rms(filt), 5), pixels_reprojected=s["pixels_reprojected"],
                                          pixels_hit=s["pixels_hit"], mean_len=round(float(hist[..., 3].mean()), 2))), flush=True)
                    if cap == 32.0 and tol == 0.05:
                        split(row, raw, hist, filt)
            r.reset_history()
            r.init_rand(41)
            r.set_camera(last)
            for k in range(frames):
                r.render(sc, 1, a.bounces)
                r.compute_guides(sc)
                r.reproject(0.05, max_history=32.0, scale=1.0)
            r.denoise_history(*SIGMAS, iterations=5)
            raw, hist, filt = r.linear(), r.history(), r.denoised()
            row = dict(case, row="quality_still", path=path, width=w, height=h, frames=frames, max_history=32.0,
                       position_tolerance=0.05)
            print(json.dumps(dict(row, raw_rms=round(rms(raw), 5), history_rms=round(rms(hist[..., 0:3]), 5),
                                  filtered_history_rms=round(rms(filt), 5))), flush=True)
            split(row, raw, hist, filt)

if __name__ == "__main__":
    main()
