"""List-schedule model of a variant-8 launch with tail fill.  No GPU.

A variant-8 launch runs one wave per 8x8 tile over a fixed number of wave slots; a slot takes the next block, in block
order, when its wave ends (tools/wave_timeline.py checks this greedy model against a measured launch).  With tail fill
the heads of the first K blocks render all but a fraction `frac` of their samples, and K small blocks, the tail parts,
follow the launch's tiles.  A tail part that is dispatched before its head ended returns at once; the sweep launch that
follows renders those, starting when the main launch has ended.

The model keeps each wave's duration fixed (a wave's time is proportional to its samples); real waves run somewhat
faster when their SIMD holds fewer of them, so the model's gain is an upper bound.

    python tools/tail_fill_model.py durations.json [--slots 7168]     screen K x delta on measured durations
    python tools/tail_fill_model.py --synthetic                       the same on synthetic durations
"""
import argparse
import heapq
import json

import numpy as np

SKIP_MS = 0.002          # a tail part that returns at once: the time its slot is taken


def list_schedule(durations, slots):
    """Greedy span of `durations` in order over `slots` slots, and each item's end."""
    free = [0.0] * slots
    ends = np.empty(len(durations))
    for i, x in enumerate(durations):
        t = free[0]
        ends[i] = t + x
        heapq.heapreplace(free, t + x)
    return max(free) if len(durations) else 0.0, ends


def tail_fill_schedule(durations, slots, k, frac, surcharge=0.0):
    """The launch of `durations` (block order) with the first k blocks holding back `frac` of their samples.
    surcharge: extra cost of a tail part relative to its samples' share.  Returns {"span", "main_span", "swept",
    "in_launch"}: the end of the sweep, the end of the main launch, and the parts each rendered."""
    d = np.asarray(durations, dtype=np.float64)
    k = int(min(k, len(d)))
    head = d.copy()
    head[:k] *= 1.0 - frac
    tail = d[:k] * frac * (1.0 + surcharge)
    free = [0.0] * slots
    head_end = np.empty(len(d))
    for i, x in enumerate(head):
        t = free[0]
        head_end[i] = t + x
        heapq.heapreplace(free, t + x)
    left = []
    for i, x in enumerate(tail):
        t = free[0]
        if t < head_end[i]:            # the head has not ended: the part goes to the sweep
            left.append(x)
            heapq.heapreplace(free, t + SKIP_MS)
        else:
            heapq.heapreplace(free, t + x)
    main_span = max(free)
    span = main_span
    if left:
        span = main_span + list_schedule(left, slots)[0]
    return {"span": span, "main_span": main_span, "swept": len(left), "in_launch": k - len(left)}


def synthetic_durations(n=57600, seed=1):
    """Durations in cost order shaped like config C's measured launch (profiles/r04j): decile medians 165 .. 112 ms,
    a few long tiles up to 582 ms at the front, and a cost probe that ranks with 5 % noise."""
    rng = np.random.default_rng(seed)
    dec = [164.8, 160.7, 139.5, 131, 125.4, 122.2, 119, 116.9, 114.9, 111.8]
    d = np.concatenate([m * np.exp(rng.normal(0, 0.06, n // 10)) for m in dec])
    d[:600] = np.linspace(582, 200, 600)
    d = np.sort(d)[::-1]
    key = d * np.exp(rng.normal(0, 0.05, len(d)))
    return d[np.argsort(-key)]


def screen(durations, slots, surcharge=0.0):
    base = list_schedule(durations, slots)[0]
    rows = [{"k_frac": 0, "delta_frac": 0, "span": round(base, 2), "change": 0.0, "swept": 0,
             "efficiency": round(float(np.sum(durations)) / slots / base, 4)}]
    for kf in (1 / 8, 1 / 4, 1 / 2, 3 / 4):
        for df in (1 / 16, 1 / 8, 1 / 4):
            m = tail_fill_schedule(durations, slots, int(len(durations) * kf), df, surcharge)
            rows.append({"k_frac": kf, "delta_frac": df, "span": round(m["span"], 2),
                         "change": round(m["span"] / base - 1, 4), "swept": m["swept"],
                         "efficiency": round(float(np.sum(durations)) * (1 + 0) / slots / m["span"], 4)})
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("durations", nargs="?", help="JSON list of wave durations in block order (ms)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--slots", type=int, default=7168)
    ap.add_argument("--surcharge", type=float, default=0.0)
    a = ap.parse_args()
    dur = synthetic_durations() if a.synthetic or not a.durations else np.asarray(json.load(open(a.durations)), float)
    for row in screen(dur, a.slots, a.surcharge):
        print(json.dumps(row))
