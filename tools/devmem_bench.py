"""Host-side cost of a renderer's life: the wall time of `--pairs` crt_renderer_create / crt_renderer_destroy pairs.

    python tools/devmem_bench.py [--width 2560 --height 1440 --pairs 100 --label NAME]
    CRT_HIP_LIB=<another build's libcrt_hip.so> CRT_SKIP_ABI_CHECK=1 python tools/devmem_bench.py --label parent

Prints one JSON line.  One pair before the clock starts loads the code object and warms the allocator; every create
ends in a device synchronisation of its own (the uv_div check's read-back), so the host clock measures finished work.
Two builds are compared by alternating processes of this tool in one job.
"""
import argparse
import ctypes as C
import hashlib
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "raytracer-cuda_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=2560)
    ap.add_argument("--height", type=int, default=1440)
    ap.add_argument("--pairs", type=int, default=100)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import crt_amd
    from crt_amd import _lib
    L = _lib.hip()

    def pair():
        h = C.c_void_p()
        crt_amd.check(L.crt_renderer_create(a.width, a.height, 0, C.byref(h)), "crt_renderer_create")
        L.crt_renderer_destroy(h)

    pair()
    t0 = time.perf_counter()
    for _ in range(a.pairs):
        pair()
    ms = (time.perf_counter() - t0) * 1e3
    sha = hashlib.sha256(Path(_lib.HIP_LIB).read_bytes()).hexdigest()[:16]
    print(json.dumps({"label": a.label, "library_sha256": sha, "width": a.width, "height": a.height, "pairs": a.pairs,
                      "ms_total": round(ms, 3), "ms_per_pair": round(ms / a.pairs, 4)}))


if __name__ == "__main__":
    main()
