"""Traversal-only rates of the ray queries (Scene.trace / Scene.occluded) on real ray populations.

    python tools/trace_bench.py [--width 2560 --height 1440] [--reps 30] [--warmup 3] [--sets primary,bounce,...]
                                [--modes 1,2] [--thresholds 0] [--seed 7]

No pass / fail: one JSON line per case.  Scene: cornell_bunny, rebuilt 4-wide tree, default options.  The ray sets
are generated on the device with torch, from seeds:

  primary         W x H centre rays of the bench camera (coherent: neighbouring lanes, neighbouring rays)
  bounce          from every primary hit point, a seeded random unit direction in the hemisphere of the surface normal
                  facing the incoming ray, the origin nudged 1e-4 along that normal (incoherent, origins on surfaces)
  bounce_shuffled the same rays in a seeded random order (no screen-space locality left between neighbouring lanes)
  shadow          from every bounce hit point towards the centre of the primary hits on an emitting material, tmax just
                  short of it (the occlusion query; `closest` rows trace the same rays for the closest hit)

Per case: the kernel time of each of `reps` queries from the library's own HIP events (crt_scene_trace_last_stats,
which waits for the query), median and minimum; rays per second from the median; from one extra counting query the
lane fill (step_active_lanes / step_lane_slots; stream kernel only) and the box / triangle tests per ray; and whether
mode 2's records equal mode 1's bit for bit.  mode 1 = one ray per lane (trace4), mode 2 = the stream kernel.
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


def centre_rays(torch, cam, w, h, dev):
    """Camera::getRay through the pixel centres, lens offset 0, float32 (crt_render -aov shoots the same rays)."""
    import crt_amd
    c = torch.from_numpy(crt_amd.camera_floats(cam)).to(dev)
    pos, llc, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    y, x = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    u = ((x.reshape(-1).float() + 0.5) / float(w))[:, None]
    v = ((y.reshape(-1).float() + 0.5) / float(h))[:, None]
    d = ((llc + u * hor) + v * ver) - pos
    return pack(torch, pos.expand(w * h, 3), d, float("inf"))


def pack(torch, o, d, tmax):
    r = torch.zeros((len(o), 8), dtype=torch.float32, device=o.device)
    r[:, 0:3], r[:, 4:7] = o, d
    r[:, 3] = tmax
    return r.contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=2560)
    ap.add_argument("--height", type=int, default=1440)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", default="primary,bounce,bounce_shuffled,shadow")
    ap.add_argument("--modes", default="1,2")
    ap.add_argument("--thresholds", default="0", help="refill thresholds of the stream kernel (0 = the default)")
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trace_bench: no GPU; nothing here can be measured without one")
    import crt_amd
    from crt_amd import assets
    dev = torch.device("cuda:0")
    hs = crt_amd.HostScene(assets.scene_files("cornell_bunny"))
    sc = hs.upload(0, bvh="rebuilt", width=4)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)

    sets = {}
    prim = centre_rays(torch, crt_amd.camera(1), a.width, a.height, dev)
    sets["primary"] = (prim, "closest")
    h0 = sc.trace(prim)
    hit = h0["t"] >= 0

    def leave(rays, h, hit):
        """Hit points nudged off the surface, the facing normal, and a random direction in its hemisphere."""
        o, d = rays[hit][:, 0:3], rays[hit][:, 4:7]
        n = h["normal"][hit] * torch.where(h["front_face"][hit] != 0, 1.0, -1.0)[:, None]
        p = o + h["t"][hit][:, None] * d + 1e-4 * n
        r = torch.randn((len(p), 3), generator=gen, device=dev)
        r = r / r.norm(dim=1, keepdim=True)
        r = torch.where(((r * n).sum(1) < 0)[:, None], -r, r)
        return p, n, r

    p1, _, r1 = leave(prim, h0, hit)
    bounce = pack(torch, p1, r1, float("inf"))
    sets["bounce"] = (bounce, "closest")
    sets["bounce_shuffled"] = (bounce[torch.randperm(len(bounce), generator=gen, device=dev)].contiguous(), "closest")
    h1 = sc.trace(bounce)
    hit1 = h1["t"] >= 0
    p2, _, _ = leave(bounce, h1, hit1)
    mats = hs.loader_arrays()[4]
    lights = torch.tensor([i for i, m in enumerate(mats) if int(m[0]) == 3], device=dev, dtype=torch.int32)
    lit = hit & torch.isin(h0["material"], lights)
    if lit.any():
        target = (prim[lit][:, 0:3] + h0["t"][lit][:, None] * prim[lit][:, 4:7]).mean(0)
        sets["shadow"] = (pack(torch, p2, target[None] - p2, 1.0 - 1e-3), "occluded")

    modes = [int(m) for m in a.modes.split(",")]
    thresholds = [int(t) for t in a.thresholds.split(",")]
    for name in a.sets.split(","):
        if name not in sets:
            print(json.dumps({"set": name, "error": "not available (no primary ray hits an emitting material)"}))
            continue
        rays, query = sets[name]
        for q in ([query, "closest"] if query == "occluded" else [query]):
            run = sc.occluded if q == "occluded" else (lambda r, **kw: sc.trace(r, **kw)["f32"].view(torch.int32))
            base = run(rays, mode=1)
            for mode in modes:
                for thr in (thresholds if mode == 2 else [0]):
                    kw = dict(mode=mode, refill_threshold=thr)
                    for _ in range(a.warmup):
                        out = run(rays, **kw)
                    ms = []
                    for _ in range(a.reps):
                        out = run(rays, **kw)
                        ms.append(sc.trace_stats()["kernel_ms"])
                    run(rays, count_work=True, **kw)
                    st = sc.trace_stats()
                    med = statistics.median(ms)
                    row = {"set": name, "query": q, "n": len(rays), "mode": mode, "refill_threshold": thr,
                           "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms), 4), "reps": a.reps,
                           "grays_per_s": round(len(rays) / med / 1e6, 3),
                           "share_reported": round(float((out != 0).float().mean() if q == "occluded" else
                                                         (out[:, 0] != np.float32(-1).view(np.int32)).float().mean()), 4),
                           "equals_mode1": bool(torch.equal(out, base))}
                    if mode == 2:
                        row["lane_fill"] = round(st["step_active_lanes"] / max(1, st["step_lane_slots"]), 4)
                        row["box_tests_per_ray"] = round(st["box_tests"] / len(rays), 2)
                        row["tri_tests_per_ray"] = round(st["tri_tests"] / len(rays), 2)
                    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
