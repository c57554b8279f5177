"""The variance-guided filter of the history (Renderer.reproject_moments / denoise_history_variance): what
it costs beside the plain chain and what it buys.

    python tools/variance_bench.py [--rows timing,parent_filter,bench_ab,viewer,quality] [--sizes 1280x720,2560x1440]
                                   [--reps 7] [--warmup 3] [--quality-size 1280x720] [--frames 240] [--bounces 20]
                                   [--parent-tree PATH]

No pass / fail: JSON lines.  Scene: cornell_bunny, rebuilt 4-wide tree, default options, bench camera, seed 41.  The camera
paths are tools/reproject_bench.py's: orbit = yaw -90 + 5 sin(2 pi k / 64), pitch 3 (1 - cos(2 pi k / 64)) degrees at
frame k; strafe = the bench camera moved sideways to x = 0.2 sin(2 pi k / 64).

  timing         a device-to-device copy rate measured in this process (torch, a 256 MiB buffer); per size, two renderers
                 over the same orbit frames, one running reproject + denoise_history(4, inf, 0.05), the other
                 reproject_moments + denoise_history_variance(4, inf, 0.05, min_history 4), 5 iterations each: the two
                 reprojections beside their byte floors (per pixel 92, and 16 more for the moments read and written), the
                 filters' launches one by one (slot 0: the kernel that forms c_0 / the estimate kernel), the variance
                 filter again through the direct kernel alone (tiled against direct per stride), and the nominal byte
                 floors: estimate 48 per pixel (history 16, moments 8, key 4, c_0 16, v 4), an iteration 64 (rows 16 in,
                 16 out, guides 32; 60 for the last, which writes 12).
  parent_filter  --parent-tree: the plain filter's launches one by one, measured by a child process per run that loads
                 the parent revision's libraries, interleaved with a child that loads this tree's: three of each.
  bench_ab       --parent-tree: `python bench.py --gpus 1 --steps 5 --warmup 2` in both trees, interleaved, `reps` of
                 each; whether this tree's median lies inside the parent's own spread.
  viewer         crt_viewer's fps over `frames` frames, scripts still and orbit, per size: without the mode, with
                 -reproject -denoise, with -reproject -denoise-variance, and (--parent-tree) the parent's crt_viewer
                 without the mode; interleaved, `reps` of each.
  quality        at --quality-size, per path (orbit, strafe), RMS error on linear values against a 1,024-spp frame (seed
                 1234) of the path's last camera after 32 frames (tolerance 0.05, max_history 32), over all pixels and
                 over the young ones (len < 4): the raw history, denoise_history(4, inf, 0.05), and
                 denoise_history_variance for the sigma sets named in SETS, chosen beforehand; and the same split by
                 guide key.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO / "raytracer-cuda_amd", REPO / "oracle"):
    sys.path.insert(0, str(p))

INF = float("inf")
OLD_SIGMAS = (4.0, INF, 0.05)           # §21's and §23's filter
# the paper's sigma_luminance 4 and 4 frames with §21's position sigma; and the same with the position term off, which
# shows what the luminance term does alone
SETS = {"svgf_4_pos_0.05_minh_4": (4.0, INF, 0.05, 4.0), "svgf_4_alone_minh_4": (4.0, INF, INF, 4.0)}
TOL, CAP = 0.05, 32.0


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


def per_launch(runs):
    """[[slot 0, iteration 0, ...] per frame] -> medians per launch."""
    return [round(statistics.median(col), 4) for col in zip(*runs)]


def parent_env(tree):
    lib = Path(tree) / "raytracer-cuda_amd" / "lib"
    return dict(os.environ, CRT_HIP_LIB=str(lib / "libcrt_hip.so"), CRT_HOST_LIB=str(lib / "libcrt_host.so"),
                CRT_SKIP_ABI_CHECK="1")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", default="timing,parent_filter,bench_ab,viewer,quality")
    ap.add_argument("--sizes", default="1280x720,2560x1440")
    ap.add_argument("--quality-size", default="1280x720")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bounces", type=int, default=20)
    ap.add_argument("--label", default="this tree", help="names the loaded libraries in a plain_filter row")
    a = ap.parse_args()
    if a.parent_tree:
        a.parent_tree = str(Path(a.parent_tree).resolve())
    want = set(a.rows.split(","))
    files = None
    case = {"scene": "cornell_bunny", "bvh": "rebuilt4", "bounces": a.bounces}

    if want & {"timing", "quality", "plain_filter"}:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("variance_bench: no GPU; nothing here can be measured without one")
        import crt_amd
        from crt_amd import assets
        files = assets.scene_files("cornell_bunny")
        hs = crt_amd.HostScene(files)
        sc = hs.upload(0, bvh="rebuilt", width=4)

        def frame_of(r, path, k):
            r.set_camera(crt_amd.camera(1, **pose(path, k)))
            r.render(sc, 1, a.bounces)
            r.compute_guides(sc)
    else:
        from crt_amd import assets
        files = assets.scene_files("cornell_bunny")

    # the child of parent_filter: the plain chain alone, with whatever libraries the environment names
    if "plain_filter" in want:
        for w, h in map(size, a.sizes.split(",")):
            r = crt_amd.Renderer(w, h)
            r.init_rand(41)
            runs, rp = [], []
            for k in range(a.warmup + a.reps):
                frame_of(r, "orbit", k)
                s = r.reproject(TOL, max_history=CAP, scale=1.0)
                r.denoise_history(*OLD_SIGMAS, iterations=5)
                ms = r.denoise_iteration_ms()
                if k >= a.warmup:
                    runs.append([ms["input_ms"]] + ms["iteration_ms"])
                    rp.append(s["reproject_ms"])
            print(json.dumps(dict(case, row="plain_filter", library=a.label, width=w, height=h, reps=a.reps,
                                  launches_ms=per_launch(runs), five_iterations_ms=round(sum(per_launch(runs)[1:]), 4),
                                  reproject=spread(rp))), flush=True)
            r.close()

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
        sl, sn, sx, minh = SETS["svgf_4_pos_0.05_minh_4"]
        for w, h in map(size, a.sizes.split(",")):
            ra, rb = crt_amd.Renderer(w, h), crt_amd.Renderer(w, h)
            for r in (ra, rb):
                r.init_rand(41)
            t = {k: [] for k in ("render", "guides", "reproject", "reproject_moments", "filter", "filter_variance",
                                 "filter_variance_direct")}
            old_runs, new_runs, direct_runs = [], [], []
            for k in range(a.warmup + a.reps):
                frame_of(ra, "orbit", k)
                s0 = ra.reproject(TOL, max_history=CAP, scale=1.0)
                f0 = ra.denoise_history(*OLD_SIGMAS, iterations=5)
                m0 = ra.denoise_iteration_ms()
                frame_of(rb, "orbit", k)
                s1 = rb.reproject_moments(TOL, max_history=CAP, scale=1.0)
                f1 = rb.denoise_history_variance(sl, sn, sx, min_history=minh, iterations=5)
                m1 = rb.denoise_iteration_ms()
                f2 = rb.denoise_history_variance(sl, sn, sx, min_history=minh, iterations=5, direct_only=True)
                m2 = rb.denoise_iteration_ms()
                if k >= a.warmup:
                    t["render"].append(ra.last_kernel_ms())
                    t["guides"].append(f0["guides_ms"])
                    t["reproject"].append(s0["reproject_ms"])
                    t["reproject_moments"].append(s1["reproject_ms"])
                    t["filter"].append(f0["filter_ms"])
                    t["filter_variance"].append(f1["filter_ms"])
                    t["filter_variance_direct"].append(f2["filter_ms"])
                    old_runs.append([m0["input_ms"]] + m0["iteration_ms"])
                    new_runs.append([m1["input_ms"]] + m1["iteration_ms"])
                    direct_runs.append([m2["input_ms"]] + m2["iteration_ms"])
            px = w * h
            floor = {name: round(b * px / rate * 1e3, 4) for name, b in (("reproject", 92), ("reproject_moments", 108),
                                                                         ("estimate", 48), ("iteration", 64),
                                                                         ("last_iteration", 60))}
            med = {k: statistics.median(v) for k, v in t.items()}
            old, new, direct = per_launch(old_runs), per_launch(new_runs), per_launch(direct_runs)
            print(json.dumps(dict(case, row="timing", width=w, height=h, path="orbit", reps=a.reps,
                                  **{k: spread(v) for k, v in t.items()}, floor_ms=floor,
                                  reproject_over_floor=round(med["reproject"] / floor["reproject"], 2),
                                  reproject_moments_over_floor=round(med["reproject_moments"] / floor["reproject_moments"], 2),
                                  plain_launches_ms=old, variance_launches_ms=new, variance_direct_launches_ms=direct,
                                  estimate_over_floor=round(new[0] / floor["estimate"], 2),
                                  variance_iteration_over_plain=[round(n_ / o_, 2) for n_, o_ in zip(new[1:], old[1:])],
                                  tiled_over_direct_per_stride={str(1 << i): round(new[1 + i] / direct[1 + i], 2)
                                                                for i in range(5)},
                                  pixels_reprojected=(s0["pixels_reprojected"], s1["pixels_reprojected"]))), flush=True)
            ra.close()
            rb.close()

    def child(tree, label):
        env = parent_env(tree) if tree else dict(os.environ)
        p = subprocess.run([sys.executable, str(REPO / "tools" / "variance_bench.py"), "--rows", "plain_filter", "--sizes",
                            a.sizes, "--reps", str(a.reps), "--warmup", str(a.warmup), "--label", label], env=env,
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise SystemExit(f"plain_filter child ({label}) failed: {p.stderr[-800:]}")
        return [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]

    if "parent_filter" in want and a.parent_tree:
        for run in range(3):
            for tree, label in ((a.parent_tree, "parent"), (None, "this tree")):
                for row in child(tree, label):
                    print(json.dumps(dict(row, run=run + 1)), flush=True)

    if "bench_ab" in want and a.parent_tree:
        values = {"parent": [], "this tree": []}
        for run in range(a.reps):
            for tree, label in ((Path(a.parent_tree), "parent"), (REPO, "this tree")):
                p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"], cwd=tree,
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    raise SystemExit(f"bench.py in {tree} failed: {p.stderr[-800:]}")
                info = json.loads([line for line in p.stdout.splitlines() if line.startswith("{")][-1])
                values[label].append(info["value"])
                print(json.dumps({"row": "bench_ab", "library": label, "run": run + 1, "value": info["value"],
                                  "unit": info.get("unit"), "ms_per_step": info.get("ms_per_step"),
                                  "cmd": "bench.py --gpus 1 --steps 5 --warmup 2"}), flush=True)
        lo, hi = min(values["parent"]), max(values["parent"])
        med = statistics.median(values["this tree"])
        print(json.dumps({"row": "bench_ab_summary", "parent": spread(values["parent"], "value"),
                          "this_tree": spread(values["this tree"], "value"),
                          "this_median_inside_parent_range": bool(lo <= med <= hi),
                          "this_median_minus_parent_median": round(med - statistics.median(values["parent"]), 2),
                          "parent_spread": round(hi - lo, 2)}), flush=True)

    if "viewer" in want:
        viewer = REPO / "raytracer-cuda_amd" / "bin" / "crt_viewer"
        modes = {"plain": [], "reproject_denoise": ["-reproject", "0.05:-inf:32", "-denoise", "4:inf:0.05"],
                 "reproject_denoise_variance": ["-reproject", "0.05:-inf:32", "-denoise-variance", "4:inf:0.05:4"]}
        programs = [(name, viewer, extra, REPO) for name, extra in modes.items()]
        if a.parent_tree:
            programs.append(("parent_plain", Path(a.parent_tree) / "raytracer-cuda_amd" / "bin" / "crt_viewer", [],
                             Path(a.parent_tree)))
        for w, h in map(size, a.sizes.split(",")):
            for script in ("still", "orbit"):
                fps = {name: [] for name, _, _, _ in programs}
                extra_keys = {}
                for _ in range(a.reps):
                    for name, exe, extra, cwd in programs:
                        p = subprocess.run([str(exe), "-w", str(w), "-h", str(h), "-frames", str(a.frames), "-script", script,
                                            "-bvh", "rebuilt", *extra, *map(str, files)], capture_output=True, text=True,
                                           timeout=300, cwd=cwd)
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
                    row["plain_median_inside_parent_range"] = bool(lo <= med <= hi)
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
                return round(float(np.sqrt(np.mean(d if mask is None else d[mask]))), 5)

            r.reset_history()
            r.init_rand(41)
            for k in range(frames):
                frame_of(r, path, k)
                s = r.reproject_moments(TOL, max_history=CAP, scale=1.0)
            hist = r.history()
            key = r.guides().view(np.int32)[..., 7]
            young = hist[..., 3] < 4
            images = {"history": hist[..., 0:3]}
            r.denoise_history(*OLD_SIGMAS, iterations=5)
            images["denoise_history_4_inf_0.05"] = r.denoised()
            variance = None
            for name, (sl, sn, sx, minh) in SETS.items():
                r.denoise_history_variance(sl, sn, sx, min_history=minh, iterations=5)
                images[name] = r.denoised()
                variance = r.variance()
            row = dict(case, row="quality", path=path, width=w, height=h, frames=frames, max_history=CAP,
                       position_tolerance=TOL)
            print(json.dumps(dict(row, pixels=w * h, young_pixels=int(young.sum()),
                                  young_share=round(float(young.mean()), 4), pixels_reprojected=s["pixels_reprojected"],
                                  raw_frame_rms=rms(r.linear()),
                                  variance_mean=round(float(variance[np.isfinite(variance)].mean()), 5),
                                  variance_mean_young=round(float(variance[young & np.isfinite(variance)].mean()), 5)
                                  if young.any() else None,
                                  all={n_: rms(img) for n_, img in images.items()},
                                  young={n_: rms(img, young) for n_, img in images.items()} if young.any() else None,
                                  old={n_: rms(img, ~young) for n_, img in images.items()})), flush=True)
            for k in np.unique(key):
                m = key == k
                print(json.dumps(dict(row, row="quality_by_key", key=int(k), pixels=int(m.sum()),
                                      young_pixels=int((m & young).sum()),
                                      all={n_: rms(img, m) for n_, img in images.items()})), flush=True)


if __name__ == "__main__":
    main()
