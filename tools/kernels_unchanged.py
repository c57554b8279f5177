"""Do two builds of csrc/crt_hip.hip hold the same render and trace kernels?  No GPU.

    make -C <tree>/raytracer-cuda_amd isa > <tree>/isa.log 2>&1      (in both trees)
    python tools/kernels_unchanged.py <parent tree> <this tree> [--show 'crt_render_kernel<false, 8, 7>' ...]
                                      [--expect-changed crt_path_step_kernel ...] [--all]

Compares, for every crt_render_kernel / crt_trace_kernel / crt_trace_lane_kernel instantiation, their indirect forms
and the path kernels (crt_camera_rays_kernel, crt_path_step_kernel, crt_path_advance_kernel and its indirect form,
crt_path_finish_kernel), the figures of
-Rpass-analysis=kernel-resource-usage (isa.log) and the assembly text of build/crt_hip.s from the kernel's label to its
.end_amdhsa_kernel: every instruction and the kernel descriptor.  The compiler numbers a function's local labels
`.LBB<f>_<b>` with f = the function's position in the module; a kernel added ahead of the template instantiations
shifts f for all of them without changing an instruction, so f is replaced by a constant before the comparison (b, the
block number inside the function, stays); a label's trailing comment is padded to a fixed column, so when f gains a
digit the padding loses a blank, and the blanks between a label and its comment are made one.  Prints the kernels that differ, the totals, the figures of the kernels named
with --show and of every kernel only the second tree has; exit status 1 if any kernel differs.  A kernel named with
--expect-changed may differ: it is printed with both trees' figures and instruction counts, and sets exit status 1
only if a figure got worse (more VGPRs, any scratch or spill, fewer waves per SIMD, more LDS).  --all compares every
kernel of the parent's build (the self-test, adaptive and denoiser kernels too), not only the families named above.
"""
import argparse
import re
import subprocess
import sys
from pathlib import Path

WANTED = ("crt_render_kernel", "crt_trace_kernel", "crt_trace_lane_kernel", "crt_camera_rays_kernel", "crt_path_step_kernel",
          "crt_path_advance_kernel", "crt_trace_indirect_kernel", "crt_trace_lane_indirect_kernel",
          "crt_path_advance_indirect_kernel", "crt_path_finish_kernel")
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
                out[name] = re.sub(r"(?m)^(\.LBBf_\d+:)[ \t]+;", r"\1 ;", re.sub(r"BB\d+_", "BBf_", "".join(buf)))
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


def worse(parent: str, now: str) -> list:
    """The figures of `now` that are worse than `parent`'s."""
    a, b = (dict((k, int(v)) for k, v in (f.split(": ") for f in s.split("; "))) for s in (parent, now))
    out = [k for k in ("VGPRs", "LDS Size [bytes/block]") if b[k] > a[k]]
    out += [k for k in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill") if b[k] > 0]
    if b["Occupancy [waves/SIMD]"] < a["Occupancy [waves/SIMD]"]:
        out.append("Occupancy [waves/SIMD]")
    return out


def instructions(text: str) -> int:
    """Instruction lines of a kernel's text: from its label to s_endpgm, without labels, directives and comments."""
    body = text.split(".section", 1)[0].split("\n")[1:]
    return sum(1 for line in body if line.startswith("\t") and not line.lstrip().startswith((".", ";")))


def demangle(names) -> dict:
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("now")
    ap.add_argument("--show", nargs="*", default=[])
    ap.add_argument("--expect-changed", nargs="*", default=[], metavar="NAME")
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()
    trees = [Path(a.parent), Path(a.now)]
    asm = [kernels(t / "raytracer-cuda_amd" / "build" / "crt_hip.s") for t in trees]
    fig = [figures(t / "isa.log") for t in trees]
    names = demangle(sorted(set(asm[0]) | set(asm[1])))
    old = [k for k in asm[0] if a.all or any(w in k for w in WANTED)]
    differ = [k for k in old if asm[1].get(k) != asm[0][k] or fig[1].get(k) != fig[0][k]]
    short = {k: names[k].replace("void ", "").split("(")[0] for k in names}
    failed = [k for k in differ if short[k] not in a.expect_changed]
    for k in differ:
        if k in failed:
            print("DIFFERS:", names[k])
            continue
        bad = worse(fig[0][k], fig[1][k]) if k in asm[1] and k in fig[1] else ["missing"]
        print("DIFFERS, as expected:" if not bad else "DIFFERS, and is WORSE in " + ", ".join(bad) + ":", names[k])
        print(f"    parent: {fig[0][k]}; {instructions(asm[0][k])} instructions")
        print(f"    now:    {fig[1].get(k)}; {instructions(asm[1].get(k, ''))} instructions")
        if bad:
            failed.append(k)
    n_render = sum("crt_render_kernel" in k for k in old)
    print(f"{len(old)} kernels compared ({n_render} crt_render_kernel, {len(old) - n_render} {'other' if a.all else 'ray-query and path-step'} kernels): "
          f"{len(old) - len(differ)} with the same figures and assembly text, {len(differ)} different; "
          f"{sum(asm[0][k].count(chr(10)) for k in old):,} lines in the parent, "
          f"{sum(asm[1][k].count(chr(10)) for k in old if k in asm[1]):,} now")
    for k in old:
        if short[k] in a.show:
            print(names[k])
            print("    parent:", fig[0][k])
            print("    now:   ", fig[1].get(k))
    for k in asm[1]:
        if k not in asm[0]:
            print("new:", names[k])
            print("    ", fig[1].get(k))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
