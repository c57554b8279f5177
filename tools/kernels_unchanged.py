"""Do two builds of csrc/crt_hip.hip hold the same render and trace kernels?  No GPU.

    make -C <tree>/raytracer-cuda_amd isa > <tree>/isa.log 2>&1      (in both trees)
    python tools/kernels_unchanged.py <parent tree> <this tree> [--show 'crt_render_kernel<false, 8, 7>' ...]

Compares, for every crt_render_kernel / crt_trace_kernel / crt_trace_lane_kernel instantiation and the two path-step
kernels (crt_camera_rays_kernel, crt_path_step_kernel), the figures of
-Rpass-analysis=kernel-resource-usage (isa.log) and the assembly text of build/crt_hip.s from the kernel's label to its
.end_amdhsa_kernel: every instruction and the kernel descriptor.  The compiler numbers a function's local labels
`.LBB<f>_<b>` with f = the function's position in the module; a kernel added ahead of the template instantiations
shifts f for all of them without changing an instruction, so f is replaced by a constant before the comparison (b, the
block number inside the function, stays).  Prints the kernels that differ, the totals, the figures of the kernels named
with --show and of every kernel only the second tree has; exit status 1 if any kernel differs.
"""
import argparse
import re
import subprocess
import sys
from pathlib import Path

WANTED = ("crt_render_kernel", "crt_trace_kernel", "crt_trace_lane_kernel", "crt_camera_rays_kernel", "crt_path_step_kernel")
FIGURES = r"(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\])"


def kernels(asm: Path) -> dict:
    out, name, buf = {}, None, []
    for line in asm.read_text().splitlines(keepends=True):
        m = re.match(r"^(_Z\w+):", line)
        if name is None and m and "_kernel" in m.group(1):
            name, buf = m.group(1), []
        if name is not None:
            buf.append(line)
            if ".end_amdhsa_kernel" in line:
                out[name] = re.sub(r"BB\d+_", "BBf_", "".join(buf))
                name = None
    return out


def figures(log: Path) -> dict:
    out, name = {}, None
    for line in log.read_text().splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        m = re.search(r"remark:\s+" + FIGURES + r": (\d+)", line)
        if m and name:
            out[name].append(f"{m.group(1)}: {m.group(2)}")
    return {k: "; ".join(v) for k, v in out.items()}


def demangle(names) -> dict:
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("now")
    ap.add_argument("--show", nargs="*", default=[])
    a = ap.parse_args()
    trees = [Path(a.parent), Path(a.now)]
    asm = [kernels(t / "raytracer-cuda_amd" / "build" / "crt_hip.s") for t in trees]
    fig = [figures(t / "isa.log") for t in trees]
    names = demangle(sorted(set(asm[0]) | set(asm[1])))
    old = [k for k in asm[0] if any(w in k for w in WANTED)]
    differ = [k for k in old if asm[1].get(k) != asm[0][k] or fig[1].get(k) != fig[0][k]]
    for k in differ:
        print("DIFFERS:", names[k])
    n_render = sum("crt_render_kernel" in k for k in old)
    print(f"{len(old)} kernels compared ({n_render} crt_render_kernel, {len(old) - n_render} ray-query and path-step kernels): "
          f"{len(old) - len(differ)} with the same figures and assembly text, {len(differ)} different; "
          f"{sum(asm[0][k].count(chr(10)) for k in old):,} lines in the parent, "
          f"{sum(asm[1][k].count(chr(10)) for k in old if k in asm[1]):,} now")
    for k in old:
        if names[k].replace("void ", "").split("(")[0] in a.show:
            print(names[k])
            print("    parent:", fig[0][k])
            print("    now:   ", fig[1].get(k))
    for k in asm[1]:
        if k not in asm[0]:
            print("new:", names[k])
            print("    ", fig[1].get(k))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
