"""The wavefront drivers (crt_amd.paths.render with torch or device compaction, Renderer.render_wavefront) against
Renderer.render on the same frame, and where their time goes.

    python tools/path_bench.py [--width 1280 --height 720] [--spp 16] [--bounces 20] [--reps 7] [--warmup 1]
                               [--mode 0] [--rows frame,phases,step,queue,advance,queued,finish]

No pass / fail: JSON lines.  Scene: cornell_bunny, rebuilt 4-wide tree, default options, bench camera, seed 41.

  frame   `reps` pairs of frames, interleaved in one process: Renderer.render (the library's own HIP events,
          last_kernel_ms) and paths.render (torch events round the whole call, host work included: the driver waits
          for the device once or twice per iteration to size the next batch); medians, their ratio, and whether the
          two frames' sums, RNG state and ray counts are equal.
  phases  one more wavefront frame with the driver's per-iteration profile: device milliseconds and shares of trace,
          step, camera and the torch work (select = finding the ended paths and their pixels, compact = scattering the
          new rays and boolean indexing); the rest of the frame time is host time between the phases.
  queue    `reps` rounds of four frames, interleaved in one process: Renderer.render, paths.render with
          torch compaction (the parent's code path), paths.render(compact="device") and Renderer.render_wavefront (its
          own HIP events round the loop); medians, ratios to the torch driver, equal bits.
  advance one more compact="device" frame with the per-iteration profile: device milliseconds and shares of trace,
          advance and count (the 4-byte read the host waits for); the advance kernel's entries per second and the bytes
          an entry moves -- ray, hit and path 32 B read each, RNG 24 B read and written, then 64 B written by an entry
          that is appended, and the sum's 12 B read and written plus remaining's 4 B read (and written when a sample is
          taken) by one that ended -- and `advance_entries`, the input entries per reservation of output slots in the
          loaded build.  The reservation sweep is this row from builds with other constants:
              tools/build_profile_lib.sh adv64 -DCRT_ADVANCE_ENTRIES=64        (also 512, 1024; the default is 256)
              CRT_HIP_LIB=raytracer-cuda_amd/lib_exp/adv64/libcrt_hip.so python tools/path_bench.py --rows advance
  queued   `reps` rounds, interleaved in one process, of the queue row's four drivers and
          Renderer.render_wavefront(sync_every=K) for K = 1, 2, 4, 8, 16, 32 and 0 (the library's default): medians, the
          run-to-run spread of the existing library loop (the yardstick), each K's ratio to it, equal bits, rays and
          iterations.
  finish  (only when asked for) `reps` rounds, interleaved in one process after a warm-up of every
          driver: Renderer.render, Renderer.render_wavefront(sync_every=0) (the yardstick, with its spread over the
          runs) and Renderer.render_wavefront(sync_every=0, finish_below=K) for K = 0, 1k, 4k, 16k, 64k, 256k and the
          number of pixels.  One line per driver: median and minimum ms, rays, iterations, equal bits; for a K also its
          ratio to the yardstick, the batch handed over (the bound the host held and the device's count) and the
          finish kernel's own milliseconds, from events round paths.finish in a Python copy of the loop that stops at
          the same hand-off.  A last line names the fastest K and its margin over K = 0 against the yardstick's spread.
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
    ap.add_argument("--rows", default="frame,phases,step,queue,advance,queued", help="the rows to measure, comma-separated")
    a = ap.parse_args()
    want = set(a.rows.split(","))

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

    def wavefront(profile=None, compact="torch"):
        r.init_rand(41)
        r.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = paths.render(sc, r, a.spp, a.bounces, trace_options=opts, profile=profile, compact=compact)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), res

    def state():
        r.synchronize()
        return r.linear().view(np.uint32), r.rng_state()

    def library():
        r.init_rand(41)
        r.synchronize()
        res = r.render_wavefront(sc, a.spp, a.bounces, trace_options=opts)
        return res["ms"], res

    def queued(sync_every):
        r.init_rand(41)
        r.synchronize()
        res = r.render_wavefront(sc, a.spp, a.bounces, trace_options=opts, sync_every=sync_every)
        return res["ms"], res

    if want & {"queue", "advance"}:
        queue_rows(a, want, case, direct, wavefront, library, state)
    if "queued" in want:
        queued_rows(a, case, direct, wavefront, library, queued, state)
    if "finish" in want:
        finish_rows(a, case, sc, r, opts, direct, queued, state)
    if not want & {"frame", "phases", "step"}:
        return
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


def queue_rows(a, want, case, direct, wavefront, library, state):
    import crt_amd
    entries = crt_amd._lib.require("crt_path_advance_entries")()
    med = statistics.median
    if "queue" in want:
        for _ in range(a.warmup):
            direct(), wavefront(), wavefront(compact="device"), library()
        ms = {"render": [], "torch": [], "device": [], "library": []}
        states, res = {}, {}
        for _ in range(a.reps):
            ms["render"].append(direct())
            states["render"] = state()
            for k, run in (("torch", wavefront), ("device", lambda: wavefront(compact="device")), ("library", library)):
                t, res[k] = run()
                ms[k].append(t)
                states[k] = state()
        equal = all(np.array_equal(states[k][0], states["render"][0]) and np.array_equal(states[k][1], states["render"][1])
                    for k in ("torch", "device", "library"))
        equal = equal and len({(res[k]["rays"], res[k]["iterations"]) for k in res}) == 1
        print(json.dumps(dict(case, row="queue", reps=a.reps, advance_entries=entries,
                              **{k + "_ms_median": round(med(v), 3) for k, v in ms.items()},
                              **{k + "_ms_min": round(min(v), 3) for k, v in ms.items()},
                              device_over_torch=round(med(ms["device"]) / med(ms["torch"]), 3),
                              library_over_torch=round(med(ms["library"]) / med(ms["torch"]), 3),
                              library_over_render=round(med(ms["library"]) / med(ms["render"]), 2),
                              rays=res["library"]["rays"], iterations=res["library"]["iterations"], equal_bits=bool(equal))),
              flush=True)
    if "advance" in want:
        wavefront(compact="device")
        t_rows = []
        wavefront(t_rows)                                     # the torch driver's profile: the entries that ended
        ended = sum(row["ended"] for row in t_rows)
        adv_ms, best = [], None
        for _ in range(max(a.reps, 1)):
            rows = []
            total_ms, res = wavefront(rows, compact="device")
            adv_ms.append(sum(row["advance_ms"] for row in rows))
            if best is None or adv_ms[-1] <= min(adv_ms):
                best = (total_ms, rows)
        total_ms, rows = best
        keys = ("trace", "advance", "count")
        ms = {k: sum(row.get(k + "_ms", 0.0) for row in rows) for k in keys}
        n = sum(row["n"] for row in rows)
        appended = n - rows[0]["n"]                           # every batch but the first was appended by an advance
        taken = appended - (n - ended)                        # ended entries that took a new sample
        moved = n * (3 * 32 + 2 * 24) + appended * 64 + ended * (24 + 4) + taken * 4
        big = [row for row in rows if row["n"] >= a.width * a.height // 2]
        n_big, ms_big = sum(row["n"] for row in big), sum(row["advance_ms"] for row in big)
        print(json.dumps(dict(case, row="advance", advance_entries=entries, reps=len(adv_ms), frame_ms=round(total_ms, 3),
                              iterations=len(rows), **{k + "_ms": round(v, 3) for k, v in ms.items()},
                              **{k + "_share": round(v / total_ms, 4) for k, v in ms.items()},
                              host_and_gaps_share=round(1 - sum(ms.values()) / total_ms, 4),
                              advance_ms_median=round(med(adv_ms), 3), advance_ms_min=round(min(adv_ms), 3),
                              entries=n, ended=ended, regenerated=taken,
                              gpaths_per_s=round(n / med(adv_ms) / 1e6, 3), bytes_per_entry=round(moved / n, 1),
                              gbytes_per_s=round(moved / med(adv_ms) / 1e6, 1), large_iterations=len(big),
                              large_gpaths_per_s=round(n_big / ms_big / 1e6, 3) if big else None)), flush=True)


QUEUED_KS = (1, 2, 4, 8, 16, 32, 0)          # 0: the library's default


def queued_rows(a, case, direct, wavefront, library, queued, state):
    med = statistics.median
    runs = [("torch", wavefront), ("device", lambda: wavefront(compact="device")), ("library", library)]
    runs += [(f"queued_{k}", lambda k=k: queued(k)) for k in QUEUED_KS]
    for _ in range(a.warmup):
        direct()
        for _, run in runs:
            run()
    ms = {"render": [], **{k: [] for k, _ in runs}}
    states, res = {}, {}
    for _ in range(a.reps):
        ms["render"].append(direct())
        states["render"] = state()
        for k, run in runs:
            t, res[k] = run()
            ms[k].append(t)
            states[k] = state()
    equal = all(np.array_equal(states[k][0], states["render"][0]) and np.array_equal(states[k][1], states["render"][1])
                for k, _ in runs)
    equal = equal and len({(res[k]["rays"], res[k]["iterations"]) for k in res}) == 1
    lib = ms["library"]
    print(json.dumps(dict(case, row="queued", reps=a.reps, **{k + "_ms_median": round(med(v), 3) for k, v in ms.items()},
                          **{k + "_ms_min": round(min(v), 3) for k, v in ms.items()},
                          library_ms_max=round(max(lib), 3), library_ms_spread=round(max(lib) - min(lib), 3),
                          library_ms_all=[round(v, 3) for v in lib],
                          **{f"queued_{k}_over_library": round(med(ms[f"queued_{k}"]) / med(lib), 3) for k in QUEUED_KS},
                          rays=res["library"]["rays"], iterations=res["library"]["iterations"], equal_bits=bool(equal))),
          flush=True)


FINISH_KS = (0, 1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18)     # and the number of pixels
QUEUE_SYNC_EVERY = 32                                             # the library's block for sync_every = 0


def finish_rows(a, case, sc, r, opts, direct, queued, state):
    import torch
    import crt_amd
    from crt_amd import paths
    med = statistics.median
    n_pix = a.width * a.height
    ks = FINISH_KS + (n_pix,)

    def handoff(k):
        r.init_rand(41)
        r.synchronize()
        res = r.render_wavefront(sc, a.spp, a.bounces, trace_options=opts, sync_every=0, finish_below=k)
        return res["ms"], res

    def kernel(k):
        """The library's loop at sync_every = 0 out of the Python calls, up to the same hand-off: the bound the host
        holds, the device's count and the milliseconds of paths.finish alone."""
        r.init_rand(41)
        r.write_linear(np.zeros((a.height, a.width, 3), np.float32))
        tdev = torch.device("cuda", 0)
        remaining = torch.full((n_pix,), a.spp - 1, dtype=torch.int32, device=tdev)
        batches = [crt_amd.camera_rays(r), (torch.empty((n_pix, 8), dtype=torch.float32, device=tdev),
                                            torch.empty((n_pix, 8), dtype=torch.int32, device=tdev))]
        hits = torch.empty((n_pix, 8), dtype=torch.float32, device=tdev)
        count = torch.full((1,), n_pix, dtype=torch.int32, device=tdev)
        m, cur = n_pix, 0
        while m:
            if m <= k:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                paths.finish(sc, r, batches[cur][0][:m], batches[cur][1][:m], a.bounces, remaining, count_in=count)
                e1.record()
                e1.synchronize()
                return {"handed_bound": m, "handed_entries": int(count), "finish_kernel_ms": round(e0.elapsed_time(e1), 3)}
            for _ in range(QUEUE_SYNC_EVERY):
                rays, pth = batches[cur][0][:m], batches[cur][1][:m]
                sc.trace(rays, count=count, out=hits[:m], **opts)
                _, _, count = paths.advance(sc, r, rays, hits[:m], pth, a.bounces, remaining, out=batches[cur ^ 1],
                                            count_in=count)
                cur ^= 1
            m = min(int(count), m)
        return {"handed_bound": 0, "handed_entries": 0, "finish_kernel_ms": None}

    runs = [("queued_0", lambda: queued(0))] + [(f"finish_{k}", lambda k=k: handoff(k)) for k in ks]
    for _ in range(a.warmup):
        direct()
        for _, run in runs:
            run()
    ms = {"render": [], **{k: [] for k, _ in runs}}
    states, res = {}, {}
    for _ in range(a.reps):
        ms["render"].append(direct())
        states["render"] = state()
        for k, run in runs:
            t, res[k] = run()
            ms[k].append(t)
            states[k] = state()
    equal = {k: bool(np.array_equal(states[k][0], states["render"][0]) and np.array_equal(states[k][1], states["render"][1])
                     and res[k]["rays"] == res["queued_0"]["rays"]) for k, _ in runs}
    yard = ms["queued_0"]
    spread = max(yard) - min(yard)
    print(json.dumps(dict(case, row="finish", driver="render", reps=a.reps, ms_median=round(med(ms["render"]), 3),
                          ms_min=round(min(ms["render"]), 3))), flush=True)
    print(json.dumps(dict(case, row="finish", driver="render_wavefront(sync_every=0)", reps=a.reps,
                          ms_median=round(med(yard), 3), ms_min=round(min(yard), 3), ms_max=round(max(yard), 3),
                          ms_spread=round(spread, 3), ms_all=[round(v, 3) for v in yard], rays=res["queued_0"]["rays"],
                          iterations=res["queued_0"]["iterations"], equal_bits=equal["queued_0"])), flush=True)
    for k in ks:
        v = ms[f"finish_{k}"]
        print(json.dumps(dict(case, row="finish", driver=f"render_wavefront(sync_every=0, finish_below={k})", finish_below=k,
                              reps=a.reps, ms_median=round(med(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3),
                              over_yardstick=round(med(v) / med(yard), 3), rays=res[f"finish_{k}"]["rays"],
                              iterations=res[f"finish_{k}"]["iterations"], equal_bits=equal[f"finish_{k}"], **kernel(k))),
              flush=True)
    best = min(ks, key=lambda k: med(ms[f"finish_{k}"]))
    gain = med(ms["finish_0"]) - med(ms[f"finish_{best}"])
    print(json.dumps(dict(case, row="finish", driver="summary", fastest_finish_below=best,
                          fastest_ms_median=round(med(ms[f"finish_{best}"]), 3), finish_0_ms_median=round(med(ms["finish_0"]), 3),
                          gain_over_finish_0_ms=round(gain, 3), yardstick_spread_ms=round(spread, 3),
                          default_rule_says=best if gain > spread else 0)), flush=True)


if __name__ == "__main__":
    main()
