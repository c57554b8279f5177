"""Adaptive sampling (Renderer.render_adaptive) against Renderer.render on the same frame.

    python tools/adaptive_bench.py [--width 1280 --height 720] [--spp-max 256] [--spp-min 16] [--bounces 20] [--reps 5]
                                   [--warmup 1] [--rows overhead,sweep,order] [--tolerances T,T,...]
    python tools/adaptive_bench.py --rows one --tolerance -1 [--by-error]   (one adaptive frame and nothing else: for a profiler)
    python tools/adaptive_bench.py --rows uniform_one             (one render(spp_max) and nothing else, likewise)

No pass / fail: JSON lines.  Scene: cornell_bunny, rebuilt 4-wide tree, default options, bench camera, seed 41.  The
yardstick is Renderer.render in the same process, interleaved with what it is compared to after a warm-up of both;
medians with minimum and maximum.  Renderer.render's time is the library's HIP events round the render (cost probe and
tile sort included); render_adaptive's is its HIP events round the whole call (both halves of the first samples, every
plan, every host wait for a list length, every pass).

  overhead  render_adaptive(tolerance -1), which refines every tile in every pass, against render(spp_max): the same
            samples, sums and RNG state, so the ratio is what the passes, their plans and their waits cost.
  sweep     a reference frame of 4 x spp_max samples from another seed; per tolerance the adaptive frame's time, its
            share of the uniform frame's samples and its RMS error against the reference (all channels, linear values);
            a ladder of uniform frames with their times and RMS errors; and beside each tolerance the uniform frame
            whose time is closest.  Tolerances: --tolerances, or quantiles of the spp_min frame's non-zero tile errors.
  order     the passes' lists in tile order (the library's order) against by error (list_by_error=True) and against tile
            order with the list's first tiles at the critical-tile threshold (critical_tiles=True), one tolerance (the
            median tile error of the spp_min frame), interleaved.
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

LADDER = (1 / 16, 1 / 8, 3 / 16, 1 / 4, 3 / 8, 1 / 2, 3 / 4, 1)     # uniform frames, as fractions of spp_max
QUANTILES = (0.95, 0.85, 0.7, 0.5, 0.3, 0.1)                          # of the spp_min frame's non-zero tile errors


def spread(v):
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp-max", type=int, default=256)
    ap.add_argument("--spp-min", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default="overhead,sweep,order")
    ap.add_argument("--tolerances", default="", help="comma-separated; default: quantiles of the spp_min frame's tile errors")
    ap.add_argument("--tolerance", type=float, default=-1.0, help="--rows one")
    ap.add_argument("--by-error", action="store_true", help="--rows one: the passes' lists by error (runs the rank kernel)")
    a = ap.parse_args()
    want = set(a.rows.split(","))

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_bench: no GPU; nothing here can be measured without one")
    import crt_amd
    from crt_amd import assets
    hs = crt_amd.HostScene(assets.scene_files("cornell_bunny"))
    sc = hs.upload(0, bvh="rebuilt", width=4)
    r = crt_amd.Renderer(a.width, a.height)
    r.set_camera(crt_amd.camera(a.spp_max))
    n_pix = a.width * a.height
    case = {"scene": "cornell_bunny", "bvh": "rebuilt4", "width": a.width, "height": a.height, "spp_min": a.spp_min,
            "spp_max": a.spp_max, "bounces": a.bounces}

    def uniform(spp, seed=41):
        r.init_rand(seed)
        r.render(sc, spp, a.bounces)
        r.synchronize()
        return r.last_kernel_ms()

    def adaptive(tol, by_error=False, critical=False):
        r.init_rand(41)
        r.synchronize()
        return r.render_adaptive(sc, a.spp_min, a.spp_max, tol, a.bounces, list_by_error=by_error, critical_tiles=critical)

    def image(spp_map=None, spp=None):
        """The frame as linear values, float64 [h, w, 3]."""
        lin = r.linear().astype(np.float64)
        if spp_map is None:
            return lin / spp
        per_pixel = np.repeat(np.repeat(spp_map, 8, 0), 8, 1)[:a.height, :a.width]
        return lin / per_pixel[..., None]

    if "uniform_one" in want:
        print(json.dumps(dict(case, row="uniform_one", ms=round(uniform(a.spp_max), 3))), flush=True)
        return
    if "one" in want:
        print(json.dumps(dict(case, row="one", tolerance=a.tolerance, list_by_error=a.by_error,
                              **adaptive(a.tolerance, a.by_error))), flush=True)
        return

    def tile_errors():
        adaptive(float("inf"))
        e = r.tile_error().reshape(-1)
        return e[e > 0]

    if "overhead" in want:
        for _ in range(a.warmup):
            uniform(a.spp_max), adaptive(-1.0)
        u_ms, a_ms = [], []
        for _ in range(a.reps):
            u_ms.append(uniform(a.spp_max))
            u_state = (r.linear().view(np.uint32), r.rng_state())
            res = adaptive(-1.0)
            a_ms.append(res["ms"])
            a_state = (r.linear().view(np.uint32), r.rng_state())
        equal = bool(np.array_equal(u_state[0], a_state[0]) and np.array_equal(u_state[1], a_state[1]))
        print(json.dumps(dict(case, row="overhead", reps=a.reps, render=spread(u_ms), adaptive=spread(a_ms),
                              adaptive_over_render=round(statistics.median(a_ms) / statistics.median(u_ms), 4),
                              passes=res["passes"], samples=res["samples"], equal_bits=equal)), flush=True)

    if "sweep" in want:
        e = tile_errors()
        tols = [float(t) for t in a.tolerances.split(",")] if a.tolerances else [float(np.quantile(e, q)) for q in QUANTILES]
        uniform(4 * a.spp_max, seed=1234)
        ref = image(spp=4 * a.spp_max)

        def rms(img):
            return float(np.sqrt(np.mean((img - ref) ** 2)))

        ladder = []
        for f in LADDER:
            spp = max(2, int(round(a.spp_max * f)))
            uniform(spp)
            ms = [uniform(spp) for _ in range(a.reps)]
            ladder.append(dict(spp=spp, rms=rms(image(spp=spp)), **spread(ms)))
            print(json.dumps(dict(case, row="sweep", kind="uniform", reps=a.reps, **ladder[-1])), flush=True)
        wins = []
        for tol in tols:
            adaptive(tol)
            runs = [adaptive(tol) for _ in range(a.reps)]
            res = runs[-1]
            err = rms(image(spp_map=r.tile_spp()))
            ms = statistics.median(x["ms"] for x in runs)
            near = min(ladder, key=lambda u: abs(u["ms_median"] - ms))
            wins.append(err < near["rms"])
            print(json.dumps(dict(case, row="sweep", kind="adaptive", reps=a.reps, tolerance=tol, **spread([x["ms"] for x in runs]),
                                  samples_share=round(res["samples"] / (n_pix * a.spp_max), 4), mean_spp=round(res["mean_spp"], 2),
                                  passes=res["passes"], tiles_refined=res["tiles_refined"], tiles_at_max=res["tiles_at_max"],
                                  rms=err, nearest_uniform_spp=near["spp"], nearest_uniform_ms=near["ms_median"],
                                  nearest_uniform_rms=near["rms"], adaptive_rms_over_uniform=round(err / near["rms"], 4))),
                  flush=True)
        print(json.dumps(dict(case, row="sweep", kind="summary", tolerances=len(tols),
                              adaptive_has_lower_rms_than_nearest_uniform=int(sum(wins)))), flush=True)

    if "order" in want:
        tol = float(np.median(tile_errors()))
        kinds = {"by_error": (True, False), "tile_order": (False, False), "tile_order_critical_tiles": (False, True)}
        for _ in range(a.warmup):
            for args in kinds.values():
                adaptive(tol, *args)
        ms = {k: [] for k in kinds}
        states = {}
        for _ in range(a.reps):
            for k, args in kinds.items():
                res = adaptive(tol, *args)
                ms[k].append(res["ms"])
                states[k] = (r.linear().view(np.uint32), r.rng_state(), r.tile_spp())
        equal = all(np.array_equal(x, y) for k in kinds for x, y in zip(states[k], states["tile_order"]))
        med = statistics.median
        print(json.dumps(dict(case, row="order", reps=a.reps, tolerance=tol, passes=res["passes"],
                              samples_share=round(res["samples"] / (n_pix * a.spp_max), 4),
                              **{k: spread(v) for k, v in ms.items()},
                              by_error_over_tile_order=round(med(ms["by_error"]) / med(ms["tile_order"]), 4),
                              critical_tiles_over_tile_order=round(med(ms["tile_order_critical_tiles"]) / med(ms["tile_order"]), 4),
                              equal_bits=bool(equal))), flush=True)


if __name__ == "__main__":
    main()
