"""The wavefront driver (crt_amd.paths.render) against Renderer.render on the same frame, and where its time goes.

    python tools/path_bench.py [--width 1280 --height 720] [--spp 16] [--bounces 20] [--reps 7] [--warmup 1]
                               [--mode 0]

No pass / fail: JSON lines.  Scene: cornell_bunny, rebuilt 4-wide tree, default options, bench camera, seed 41.

  frame   `reps` pairs of frames, interleaved in one process: Renderer.render (the library's own HIP events,
          last_kernel_ms) and paths.render (torch events round the whole call, host work included: the driver waits
          for the device once or twice per iteration to size the next batch); medians, their ratio, and whether the
          two frames' sums, RNG state and ray counts are equal.
  phases  one more wavefront frame with the driver's per-iteration profile: device milliseconds and shares of trace,
          step, camera and the torch work (select = finding the ended paths and their pixels, compact = scattering the
          new rays and boolean indexing); the rest of the frame time is host time between the phases.
  step    the step kernel alone over that frame's iterations: paths per second, and bytes per second against the bytes
          an entry must move -- ray 32 B read, hit 32 B read, path 32 B read and written, RNG 24 B read and written,
          then the ray's 32 B written by a path that goes on or the sum's 12 B read and written by one that ends.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO / "raytracer-cuda_amd", REPO / "oracle"):
    sys.path.insert(0, str(p))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", type=int, default=0, help="Scene.trace mode of the driver's queries (0 = automatic)")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("path_bench: no GPU; nothing here can be measured without one")
    import crt_amd
    from crt_amd import assets, paths
    hs = crt_amd.HostScene(assets.scene_files("cornell_bunny"))
    sc = hs.upload(0, bvh="rebuilt", width=4)
    r = crt_amd.Renderer(a.width, a.height)
    r.set_camera(crt_amd.camera(a.spp))
    opts = dict(mode=a.mode)
    case = {"scene": "cornell_bunny", "bvh": "rebuilt4", "width": a.width, "height": a.height, "spp": a.spp,
            "bounces": a.bounces, "trace_mode": a.mode}

    def direct():
        r.init_rand(41)
        r.render(sc, a.spp, a.bounces)
        r.synchronize()
        return r.last_kernel_ms()

    def wavefront(profile=None):
        r.init_rand(41)
        r.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = paths.render(sc, r, a.spp, a.bounces, trace_options=opts, profile=profile)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), res

    def state():
        r.synchronize()
        return r.linear().view(np.uint32), r.rng_state()

    for _ in range(a.warmup):
        direct()
        wavefront()
    d_ms, w_ms = [], []
    for _ in range(a.reps):
        d_ms.append(direct())
        d_state = state()
        ms, res = wavefront()
        w_ms.append(ms)
        w_state = state()
    r.init_rand(41)
    r.render(sc, a.spp, a.bounces, count_work=True)
    r.synchronize()
    d_rays = r.counters()["rays"]
    dm, wm = statistics.median(d_ms), statistics.median(w_ms)
    print(json.dumps(dict(case, row="frame", reps=a.reps, render_ms_median=round(dm, 3), render_ms_min=round(min(d_ms), 3),
                          wavefront_ms_median=round(wm, 3), wavefront_ms_min=round(min(w_ms), 3),
                          wavefront_over_render=round(wm / dm, 2), rays=res["rays"], iterations=res["iterations"],
                          render_grays_per_s=round(d_rays / dm / 1e6, 3), wavefront_grays_per_s=round(res["rays"] / wm / 1e6, 3),
                          equal_bits=bool(np.array_equal(d_state[0], w_state[0]) and np.array_equal(d_state[1], w_state[1])
                                          and d_rays == res["rays"]))), flush=True)

    rows = []
    total_ms, res = wavefront(rows)
    keys = ("trace", "step", "select", "camera", "compact")
    ms = {k: sum(row.get(k + "_ms", 0.0) for row in rows) for k in keys}
    device = sum(ms.values())
    print(json.dumps(dict(case, row="phases", frame_ms=round(total_ms, 3), iterations=len(rows),
                          **{k + "_ms": round(v, 3) for k, v in ms.items()},
                          **{k + "_share": round(v / total_ms, 4) for k, v in ms.items()},
                          torch_share=round((ms["select"] + ms["compact"]) / total_ms, 4),
                          host_and_gaps_share=round(1 - device / total_ms, 4))), flush=True)

    n = sum(row["n"] for row in rows)
    ended = sum(row["ended"] for row in rows)
    both = 32 + 32 + 2 * 32 + 2 * 24                     # ray, hit, path read + written, RNG read + written
    moved = n * both + (n - ended) * 32 + ended * 24
    big = [row for row in rows if row["n"] >= a.width * a.height // 2]     # iterations with at least half a frame of paths
    n_big, ms_big = sum(row["n"] for row in big), sum(row["step_ms"] for row in big)
    print(json.dumps(dict(case, row="step", entries=n, ended=ended, step_ms=round(ms["step"], 3),
                          gpaths_per_s=round(n / ms["step"] / 1e6, 3), bytes_per_entry=round(moved / n, 1),
                          gbytes_per_s=round(moved / ms["step"] / 1e6, 1),
                          large_iterations=len(big), large_gpaths_per_s=round(n_big / ms_big / 1e6, 3) if big else None)),
          flush=True)


if __name__ == "__main__":
    main()
