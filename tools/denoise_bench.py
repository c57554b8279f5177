"""The denoiser (Renderer.compute_guides / denoise): what it costs and what it buys.

    python tools/denoise_bench.py [--rows timing,quality,adaptive] [--sizes 1280x720,2560x1440] [--reps 7] [--warmup 2]
                                  [--quality-size 1280x720] [--bounces 20]

No pass / fail: JSON lines.  Scene: cornell_bunny, rebuilt 4-wide tree, default options, bench camera, seed 41.

  timing    per size: the guides' time; the filter's launches one by one (Renderer.denoise_iteration_ms: HIP events round
            every launch) for 8 iterations, strides 1 .. 128, through the library's choice of kernel per stride and
            through the direct kernel alone (direct_only=True), the two interleaved after a warm-up of both, medians with
            minimum and maximum; beside them Renderer.render of 1, 16 and 64 spp in the same process, a device-to-device
            copy rate measured in the same process (torch, a 256 MiB buffer: bytes read + bytes written per second) and
            the floor it gives the filter, 56 B per pixel and iteration (12 colour + 32 guides read, 12 written).
  quality   RMS error on linear values against a uniform frame of 4 x the largest spp from seed 1234: raw and denoised
            frames of 4, 16, 64 and 256 spp over a small grid of sigmas, 5 iterations.
  adaptive  the same for one adaptive frame (spp_min 16, spp_max 256) per tolerance of DESIGN.md §20's sweep (the
            quantiles of the spp_min frame's non-zero tile errors), filtered with tile_scale=True.
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

INF = float("inf")
SPPS = (4, 16, 64, 256)
GRID = [(sc, sn, sx) for sc in (1.0, 4.0, 16.0) for sn in (INF, 0.3) for sx in (0.05, 0.2, INF)]
ADAPTIVE_GRID = [(1.0, INF, 0.05), (4.0, INF, 0.05), (16.0, INF, 0.05)]
QUANTILES = (0.95, 0.85, 0.7, 0.5, 0.3, 0.1)          # tools/adaptive_bench.py's


def spread(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def size(text):
    w, h = text.split("x")
    return int(w), int(h)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", default="timing,quality,adaptive")
    ap.add_argument("--sizes", default="1280x720,2560x1440")
    ap.add_argument("--quality-size", default="1280x720")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bounces", type=int, default=20)
    a = ap.parse_args()
    want = set(a.rows.split(","))

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench: no GPU; nothing here can be measured without one")
    import crt_amd
    from crt_amd import assets
    hs = crt_amd.HostScene(assets.scene_files("cornell_bunny"))
    sc = hs.upload(0, bvh="rebuilt", width=4)
    case = {"scene": "cornell_bunny", "bvh": "rebuilt4", "bounces": a.bounces}

    def renderer(w, h):
        r = crt_amd.Renderer(w, h)
        r.set_camera(crt_amd.camera(1))
        return r

    def uniform(r, spp, seed=41):
        r.init_rand(seed)
        r.render(sc, spp, a.bounces)
        r.synchronize()
        return r.last_kernel_ms()

    if "timing" in want:
        # the copy rate first, in this process
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
        rate = 2 * n / (statistics.median(copy_ms) * 1e-3)              # bytes read + written per second
        print(json.dumps(dict(case, row="copy", bytes=n, reps=a.reps, **spread(copy_ms),
                              traffic_gb_per_s=round(rate / 1e9, 1))), flush=True)
        del src, dst
        for w, h in map(size, a.sizes.split(",")):
            r = renderer(w, h)
            frame = dict(case, width=w, height=h)
            for spp in (1, 16, 64):
                uniform(r, spp)
                ms = [uniform(r, spp) for _ in range(a.reps)]
                print(json.dumps(dict(frame, row="render", spp=spp, reps=a.reps, **spread(ms))), flush=True)
            uniform(r, 16)
            scale = crt_amd.pixel_sample_scale(16)
            guides = []
            for k in range(a.warmup + a.reps):
                r.compute_guides(sc)
                s = r.denoise(4.0, INF, 0.05, iterations=1, scale=scale)
                if k >= a.warmup:
                    guides.append(s["guides_ms"])
            print(json.dumps(dict(frame, row="guides", reps=a.reps, pixels_hit=s["pixels_hit"], **spread(guides))), flush=True)
            kinds = {"library": False, "direct": True}
            per = {k: [] for k in kinds}
            total = {k: [] for k in kinds}
            inputs = []
            out = {}
            for k in range(a.warmup + a.reps):
                for kind, direct in kinds.items():
                    s = r.denoise(4.0, INF, 0.05, iterations=8, scale=scale, direct_only=direct)
                    t = r.denoise_iteration_ms()
                    out[kind] = r.denoised().view(np.uint32)
                    if k >= a.warmup:
                        per[kind].append(t["iteration_ms"])
                        total[kind].append(s["filter_ms"])
                        inputs.append(t["input_ms"])
            floor_ms = 56 * w * h / rate * 1e3
            print(json.dumps(dict(frame, row="input_kernel", reps=len(inputs), **spread(inputs))), flush=True)
            for i in range(8):
                row = dict(frame, row="stride", stride=1 << i, reps=a.reps, floor_ms=round(floor_ms, 4))
                for kind in kinds:
                    row[kind] = spread([x[i] for x in per[kind]])
                row["library_over_direct"] = round(row["library"]["ms_median"] / row["direct"]["ms_median"], 4)
                row["direct_over_floor"] = round(row["direct"]["ms_median"] / floor_ms, 2)
                print(json.dumps(row), flush=True)
            five = {}
            for kind, direct in kinds.items():
                ms = []
                for k in range(a.warmup + a.reps):
                    s = r.denoise(4.0, INF, 0.05, iterations=5, scale=scale, direct_only=direct)
                    if k >= a.warmup:
                        ms.append(s["filter_ms"])
                five[kind] = spread(ms)
            print(json.dumps(dict(frame, row="filter", iterations=5, reps=a.reps, floor_ms=round(5 * floor_ms, 4), **five,
                                  eight_iterations={k: spread(v) for k, v in total.items()},
                                  equal_bits=bool(np.array_equal(out["library"], out["direct"])))), flush=True)
            r.close()

    if "quality" in want or "adaptive" in want:
        w, h = size(a.quality_size)
        r = renderer(w, h)
        frame = dict(case, width=w, height=h)
        ref_spp = 4 * max(SPPS)
        uniform(r, ref_spp, seed=1234)
        ref = r.linear().astype(np.float64) / ref_spp
        r.compute_guides(sc)

        def rms(img):
            return float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))

        if "quality" in want:
            for spp in SPPS:
                uniform(r, spp)
                scale = crt_amd.pixel_sample_scale(spp)
                raw = rms(r.linear().astype(np.float64) * scale)
                best = None
                for sig in GRID:
                    s = r.denoise(*sig, iterations=5, scale=scale)
                    err = rms(r.denoised())
                    row = dict(frame, row="quality", spp=spp, sigma_color=sig[0], sigma_normal=sig[1], sigma_position=sig[2],
                               raw_rms=round(raw, 5), denoised_rms=round(err, 5), denoised_over_raw=round(err / raw, 4),
                               filter_ms=round(s["filter_ms"], 4))
                    print(json.dumps(row).replace("Infinity", '"inf"'), flush=True)
                    if best is None or err < best[0]:
                        best = (err, sig)
                print(json.dumps(dict(frame, row="quality_best", spp=spp, raw_rms=round(raw, 5), best_rms=round(best[0], 5),
                                      best_sigmas=[str(v) for v in best[1]],
                                      filter_wins=bool(best[0] < raw))), flush=True)

        if "adaptive" in want:
            r.init_rand(41)
            r.render_adaptive(sc, 16, max(SPPS), INF, a.bounces)
            e = r.tile_error().reshape(-1)
            e = e[e > 0]
            for q in QUANTILES:
                tol = float(np.quantile(e, q))
                r.init_rand(41)
                res = r.render_adaptive(sc, 16, max(SPPS), tol, a.bounces)
                per_pixel = np.repeat(np.repeat(r.tile_spp(), 8, 0), 8, 1)[:h, :w]
                raw = rms(r.linear().astype(np.float64) / per_pixel[..., None])
                for sig in ADAPTIVE_GRID:
                    s = r.denoise(*sig, iterations=5, tile_scale=True)
                    err = rms(r.denoised())
                    row = dict(frame, row="adaptive", tolerance=tol, quantile=q, mean_spp=round(res["mean_spp"], 2),
                               adaptive_ms=round(res["ms"], 3), sigma_color=sig[0], sigma_normal=sig[1], sigma_position=sig[2],
                               raw_rms=round(raw, 5), denoised_rms=round(err, 5), denoised_over_raw=round(err / raw, 4),
                               filter_ms=round(s["filter_ms"], 4))
                    print(json.dumps(row).replace("Infinity", '"inf"'), flush=True)


if __name__ == "__main__":
    main()
