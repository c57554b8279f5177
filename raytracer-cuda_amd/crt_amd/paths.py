"""Path steps over ray batches (crt_hip.h "path steps"): what a path tracer does between two ray
queries, as device calls on torch tensors.

  camera_rays(renderer, pixels)        Camera::getRay for a batch of pixels, each on its own RNG stream
  Scene.path_step(rays, hits, paths,   one bounce: the materials, the sky, the invalid-material re-loop, then the
                  max_bounces, rng,    bounce limit and Russian roulette of the bounce that follows
                  linear)
  advance(scene, renderer, rays,       step, regenerate and compact in one kernel: the survivors and the ended pixels'
          hits, paths, max_bounces,    next camera samples appended to an output batch, their number in a device counter
          remaining)                   
  finish(scene, renderer, rays,        a batch of paths run to their ends in one kernel, one lane per path with the trace
         paths, max_bounces,          in the lane: what a loop of Scene.trace and advance leaves, without the rounds
         remaining)                   
  render(scene, renderer, spp)         the reference driver: a wavefront path tracer out of camera_rays, Scene.trace
                                       and Scene.path_step (compact="torch") or Scene.path_advance (compact="device")
                                       whose sums, RNG state and ray count equal Renderer.render's bit for bit;
                                       on_bounce is the hook of a custom integrator

Everything is torch-only (the purpose is device-resident integrators), enqueued on torch's current stream, without a
host copy.  Tensors: rays float32 [n, 8] (crt_ray rows), hits float32 or int32 [n, 8] (crt_hit rows, Scene.trace's
"f32"), paths int32 or float32 [n, 8] (crt_path rows: throughput.xyz as float bits, bounce, pixel, status, 0, 0),
rng int32 [pixels, 6], linear float32 [pixels * 3] in any shape; or the Renderer itself for its own state and sums.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PATH_ACTIVE, PATH_ENDED, check

# columns of a crt_path row viewed as int32
PATH_BOUNCE, PATH_PIXEL, PATH_STATUS = 3, 4, 5


def _rows(x, name, dtypes):
    """x is a contiguous [n, 8] tensor of one of `dtypes`, or ValueError."""
    import torch
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    if x.dtype not in dtypes or x.dim() != 2 or x.shape[1] != 8 or not x.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [n, 8] tensor of {' or '.join(str(d) for d in dtypes)}")
    return x


def _flat(x, name, dtype, numel=None, multiple=1):
    """x is a contiguous tensor of `dtype` with `numel` elements (or a multiple), or ValueError."""
    import torch
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor or the Renderer")
    if x.dtype != dtype or not x.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor")
    if (numel is not None and x.numel() != numel) or x.numel() % multiple:
        raise ValueError(f"{name} has {x.numel()} elements, expected "
                         f"{numel if numel is not None else 'a multiple of ' + str(multiple)}")
    return x


def _batch(rays, hits, paths, max_bounces) -> int:
    """rays, hits and paths are one batch for a step of at least one bounce, or ValueError; its length."""
    import torch
    _rows(rays, "rays", (torch.float32,))
    _rows(hits, "hits", (torch.float32, torch.int32))
    _rows(paths, "paths", (torch.int32, torch.float32))
    n = rays.shape[0]
    if not (n == hits.shape[0] == paths.shape[0]):
        raise ValueError("rays, hits and paths differ in length")
    if int(max_bounces) < 1:
        raise ValueError("max_bounces must be >= 1")
    return n


def _count(x, name):
    """x is a 1-element int32 tensor (a device count), or ValueError."""
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype != torch.int32 or x.numel() != 1 or x.dim() > 1:
        raise ValueError(f"{name} must be a 1-element int32 tensor")
    return x


def _on_device(device, **tensors):
    """Checked last, so that a tensor wrong in kind is reported as that: every tensor lives on cuda:`device`."""
    for name, x in tensors.items():
        if x is not None and (not x.is_cuda or x.device.index != device):
            raise ValueError(f"{name} must be on cuda:{device}")


def _is_renderer(x) -> bool:
    from . import Renderer
    return isinstance(x, Renderer)


def camera_rays(renderer, pixels=None, rng=None):
    """Camera rays of a batch of pixels (crt_renderer_camera_rays_device): each pixel's next sample, drawn on its own
    RNG stream exactly as the render kernels draw it.  pixels: int32 [n] of y * width + x on the renderer's device, no
    pixel twice (None: every pixel, in order); rng: int32 [width * height, 6] (None: the renderer's own state).
    Returns (rays float32 [n, 8], paths int32 [n, 8]): paths start with throughput (1, 1, 1), bounce 0, ACTIVE."""
    import torch
    dev = renderer.device
    n_pix = renderer.width * renderer.height
    if pixels is not None:
        _flat(pixels, "pixels", torch.int32)
        if pixels.dim() != 1:
            raise ValueError("pixels must be one-dimensional")
    if rng is not None:
        _flat(rng, "rng", torch.int32, numel=6 * n_pix)
    _on_device(dev, pixels=pixels, rng=rng)
    fn = _lib.require("crt_renderer_camera_rays_device")
    n = n_pix if pixels is None else pixels.shape[0]
    tdev = torch.device("cuda", dev)
    rays = torch.empty((n, 8), dtype=torch.float32, device=tdev)
    paths = torch.empty((n, 8), dtype=torch.int32, device=tdev)
    check(fn(renderer.h, None if pixels is None else pixels.data_ptr(), n, None if rng is None else rng.data_ptr(),
             rays.data_ptr(), paths.data_ptr(), torch.cuda.current_stream(tdev).cuda_stream),
          "crt_renderer_camera_rays_device")
    return rays, paths


def path_step(scene, rays, hits, paths, max_bounces, rng, linear):
    """One bounce for every ACTIVE path, in place (crt_scene_path_step_device): rays[k] scattered off hits[k] by the
    hit's material, or ended into linear[3 * pixel ..] (sky, light, absorbed metal, bounce limit, roulette); paths[k]
    gets the new throughput, bounce and status.  hits: Scene.trace(rays)["f32"] of the same rays (tmax = inf).  rng,
    linear: tensors (see the module text), or the Renderer for its own.  No two active paths on the same pixel."""
    import torch
    dev = scene.device
    n = _batch(rays, hits, paths, max_bounces)
    n_pix = None
    for name, x, dtype, per in (("rng", rng, torch.int32, 6), ("linear", linear, torch.float32, 3)):
        if _is_renderer(x):
            if x.device != dev:
                raise ValueError(f"{name}: the renderer is on another device than the scene")
            k = x.width * x.height
        else:
            k = _flat(x, name, dtype, multiple=per).numel() // per
        if n_pix is not None and k != n_pix:
            raise ValueError(f"rng holds {n_pix} pixels, linear {k}")
        n_pix = k
    _on_device(dev, rays=rays, hits=hits, paths=paths, rng=None if _is_renderer(rng) else rng,
               linear=None if _is_renderer(linear) else linear)
    fn = _lib.require("crt_scene_path_step_device")
    d_rng = rng.rng_device_ptr() if _is_renderer(rng) else rng.data_ptr()
    d_linear = linear.linear_device_ptr() if _is_renderer(linear) else linear.data_ptr()
    check(fn(scene.h, rays.data_ptr(), hits.data_ptr(), paths.data_ptr(), n, int(max_bounces), d_rng,
             d_linear, n_pix, torch.cuda.current_stream(rays.device).cuda_stream), "crt_scene_path_step_device")


def _same_memory(a, b) -> bool:
    """The two tensors' bytes overlap."""
    if a.device != b.device or not a.numel() or not b.numel():
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def advance(scene, renderer, rays, hits, paths, max_bounces, remaining, rng=None, linear=None, out=None, count_in=None,
            totals=None):
    """Step, regenerate and compact (crt_scene_path_advance_device): every ACTIVE path of the read-only batch takes one
    bounce as path_step gives it; one that goes on is appended to the output batch; one that ended adds to its pixel's
    sum and, while remaining[pixel] > 0, is replaced by that pixel's next camera sample (remaining[pixel] -= 1), drawn on
    the RNG state of the same lane.  remaining: int32 [pixels] on the device, or None for "never regenerate".  rng,
    linear: tensors as for path_step, or None for the renderer's own.  out: (rays_out float32 [>= n, 8], paths_out int32
    or float32 [>= n, 8]) that overlap no input (None: allocated here).
    Returns (rays_out, paths_out, count): count is a 1-element int32 device tensor, the entries appended; they are rows
    [0, count) of the outputs in no particular order, the other rows are unspecified.  No host copy, no synchronisation;
    enqueued on torch's current stream.

    count_in: a 1-element int32 device tensor, typically the count of the advance before.  The call then advances entries
    [0, min(count_in, n)) of the batch, count_in read by the kernel on the stream and never by the host
    (crt_scene_path_advance_indirect_device): a loop of Scene.trace(count=) and advance(count_in=) on ping-pong
    batches runs without a host read, and since an entry appends at most one entry, the first batch's length serves
    all of them.  totals (with count_in): an int64 [2] device tensor the kernel adds (min(count_in, n), 1 if that is not
    0) to: the rays and the iterations of such a loop."""
    import torch
    dev = scene.device
    n = _batch(rays, hits, paths, max_bounces)
    if count_in is not None:
        _count(count_in, "count_in")
    if totals is not None:
        if count_in is None:
            raise ValueError("totals needs count_in")
        _flat(totals, "totals", torch.int64, numel=2)
    if not _is_renderer(renderer):
        raise ValueError("renderer must be a Renderer")
    if renderer.device != dev:
        raise ValueError("the renderer is on another device than the scene")
    n_pix = renderer.width * renderer.height
    if remaining is not None:
        _flat(remaining, "remaining", torch.int32, numel=n_pix)
    if rng is not None:
        _flat(rng, "rng", torch.int32, numel=6 * n_pix)
    if linear is not None:
        _flat(linear, "linear", torch.float32, numel=3 * n_pix)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("out must be a pair (rays_out, paths_out)")
        rays_out = _rows(out[0], "out rays", (torch.float32,))
        paths_out = _rows(out[1], "out paths", (torch.int32, torch.float32))
        if rays_out.shape[0] < n or paths_out.shape[0] < n:
            raise ValueError("out is shorter than the batch: its length must be at least the rays' length")
        for name, o in (("out rays", rays_out), ("out paths", paths_out)):
            for x in (rays, hits, paths):
                if _same_memory(o, x):
                    raise ValueError(f"{name} aliases an input")
        if _same_memory(rays_out, paths_out):
            raise ValueError("out rays aliases out paths")
    _on_device(dev, rays=rays, hits=hits, paths=paths, remaining=remaining, rng=rng, linear=linear, count_in=count_in,
               totals=totals, **({} if out is None else {"out rays": out[0], "out paths": out[1]}))
    fn = _lib.require("crt_scene_path_advance_device" if count_in is None else "crt_scene_path_advance_indirect_device")
    tdev = torch.device("cuda", dev)
    if out is None:
        rays_out = torch.empty((n, 8), dtype=torch.float32, device=tdev)
        paths_out = torch.empty((n, 8), dtype=torch.int32, device=tdev)
    count = torch.empty((1,), dtype=torch.int32, device=tdev)
    ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    stream = torch.cuda.current_stream(tdev).cuda_stream
    if count_in is None:
        check(fn(scene.h, renderer.h, rays.data_ptr(), hits.data_ptr(), paths.data_ptr(), n, int(max_bounces), ptr(rng),
                 ptr(linear), ptr(remaining), rays_out.data_ptr(), paths_out.data_ptr(), count.data_ptr(), stream),
              "crt_scene_path_advance_device")
    else:
        check(fn(scene.h, renderer.h, rays.data_ptr(), hits.data_ptr(), paths.data_ptr(), count_in.data_ptr(), n,
                 int(max_bounces), ptr(rng), ptr(linear), ptr(remaining), rays_out.data_ptr(), paths_out.data_ptr(),
                 count.data_ptr(), ptr(totals), stream), "crt_scene_path_advance_indirect_device")
    return rays_out, paths_out, count


def finish(scene, renderer, rays, paths, max_bounces, remaining, rng=None, linear=None, count_in=None, totals=None):
    """Run a batch of paths to their ends in one kernel (crt_scene_path_finish_device): every ACTIVE path of the
    read-only batch is traced, scattered and traced again in its own lane until it ends; it then adds to its pixel's
    sum and, while remaining[pixel] > 0, goes on with that pixel's next camera sample.  At the end the pixel's RNG
    state and sum are stored and remaining[pixel] = 0: what Scene.trace and advance leave when they are repeated until
    the count is 0, bit for bit.  The first ray of an entry keeps its row's tmax.  rays float32 [n, 8], paths int32 or
    float32 [n, 8]; no hits.  remaining: int32 [pixels] on the device, or None for "never regenerate" (each path only to
    its own end).  rng, linear: tensors as for advance, or None for the renderer's own.  count_in: a 1-element int32
    device tensor; the kernel then takes entries [0, min(count_in, n)), count_in read on the stream.  totals: an int64
    [2] device tensor the kernel adds (rays traced, 1 if it had an entry) to.  No two active entries on one pixel.
    Returns nothing.  No host copy, no synchronisation; enqueued on torch's current stream.  A lane traces at most
    (remaining[pixel] + 1) * max_bounces rays, and the call takes as long as its longest lane."""
    import torch
    dev = scene.device
    _rows(rays, "rays", (torch.float32,))
    _rows(paths, "paths", (torch.int32, torch.float32))
    n = rays.shape[0]
    if n != paths.shape[0]:
        raise ValueError("rays and paths differ in length")
    if int(max_bounces) < 1:
        raise ValueError("max_bounces must be >= 1")
    if count_in is not None:
        _count(count_in, "count_in")
    if totals is not None:
        _flat(totals, "totals", torch.int64, numel=2)
    if not _is_renderer(renderer):
        raise ValueError("renderer must be a Renderer")
    if renderer.device != dev:
        raise ValueError("the renderer is on another device than the scene")
    n_pix = renderer.width * renderer.height
    if remaining is not None:
        _flat(remaining, "remaining", torch.int32, numel=n_pix)
    if rng is not None:
        _flat(rng, "rng", torch.int32, numel=6 * n_pix)
    if linear is not None:
        _flat(linear, "linear", torch.float32, numel=3 * n_pix)
    _on_device(dev, rays=rays, paths=paths, remaining=remaining, rng=rng, linear=linear, count_in=count_in, totals=totals)
    fn = _lib.require("crt_scene_path_finish_device")
    ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    check(fn(scene.h, renderer.h, rays.data_ptr(), paths.data_ptr(), ptr(count_in), n, int(max_bounces), ptr(rng),
             ptr(linear), ptr(remaining), ptr(totals), torch.cuda.current_stream(torch.device("cuda", dev)).cuda_stream),
          "crt_scene_path_finish_device")


def shade_rows(desc) -> np.ndarray:
    """The per-material rows the step kernel reads (crt_scene_export_shade_rows; host only), float32 [materials, 2, 4]:
    row 0 = (code as int bits, 0, 0, 0), row 1 = the payload."""
    fn = _lib.require("crt_scene_export_shade_rows")
    n = C.c_int64(0)
    check(fn(C.byref(desc), None, C.byref(n)), "crt_scene_export_shade_rows")
    out = np.zeros((n.value, 2, 4), np.float32)
    check(fn(C.byref(desc), out.ctypes.data_as(C.c_void_p), C.byref(n)), "crt_scene_export_shade_rows")
    return out


class _Phases:
    """Device time per phase of the driver's iterations, from torch events recorded on the current stream (only when the
    caller asked for a profile; nothing is recorded or waited for otherwise)."""

    def __init__(self, rows):
        self.rows, self.marks = rows, []

    def mark(self, name, **info):
        if self.rows is not None:
            import torch
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev, info))

    def close(self):
        """One row per iteration: its info and the milliseconds of each phase (the time since the previous mark, the
        device's idle time while the host sizes the next batch included)."""
        if self.rows is None or not self.marks:
            return
        self.marks[-1][1].synchronize()
        row = None
        for (_, e0, _), (name, e1, info) in zip(self.marks, self.marks[1:]):
            if name == "trace":
                row = {}
                self.rows.append(row)
            if row is not None:
                row[name + "_ms"] = row.get(name + "_ms", 0.0) + e0.elapsed_time(e1)
                row.update({k: int(v) for k, v in info.items()})      # device scalars are read only now


def render(scene, renderer, spp, max_bounces=20, regenerate=True, on_bounce=None, trace_options=None,
           profile=None, compact="torch", sync_every=1, finish_below=0) -> dict:
    """The reference driver: spp samples per pixel as a wavefront of camera_rays / Scene.trace / Scene.path_step calls on
    the renderer's own RNG state and (fresh) sums, so renderer.linear(), rng_state() and resolve() work afterwards
    and hold what renderer.render(scene, spp, max_bounces) leaves, bit for bit.

    regenerate=True: a path that ends while its pixel has samples left is replaced by that pixel's next camera ray in
    the same iteration, and the batch is compacted with torch indexing; False: sample by sample, each until its last
    path ends.  on_bounce(rays, hits, paths) runs between the trace and the step of every iteration (the hook of a
    custom integrator; it may edit the tensors in place).  trace_options: keywords of Scene.trace (mode, grid_waves,
    ...).  profile: a list that receives one dict per iteration, its entries (n, ended) and the device milliseconds of
    its phases (trace, step, select, camera, compact; tools/path_bench.py).

    compact="device": the step, the regeneration and the compaction are one advance() call per iteration on two
    preallocated ping-pong batches, and the host waits once per iteration, for the 4-byte count (regenerate=False:
    advance with remaining=None as the compaction).  No torch indexing; the same bits.  on_bounce then sees the batch
    before the advance and may edit it in place; the profile's phases are trace, advance and count, its entries n.

    sync_every (compact="device"): 1 is the loop above.  K > 1 enqueues blocks of K iterations of Scene.trace(count=)
    and advance(count_in=) between two reads of the count: the kernels take the batch size from the device, and the
    last size the host read bounds the batches of the whole block (a batch is never larger than the one before it).
    The same bits, rays and iterations.  on_bounce is then called with a fourth argument, the device count: its first
    three arguments are views of the bound's length, whose rows from the count on are stale, and only rows below the
    count may be edited.  The profile's entries n are then the bounds.

    finish_below (compact="device"): K > 0 hands the batch to finish() as soon as the count the host holds (every pixel
    at the start, then each count it reads) is <= K; finish() runs those paths and their pixels' remaining samples to
    the end in one kernel.  The same bits and rays; the finish counts as one iteration.  on_bounce is called for the
    wavefront rounds only, never for the bounces inside finish(): a hybrid integrator does its own work on the first
    rounds and lets the library complete the frame.  The profile has no row for the finish.  0: never.
    Returns {"rays": rays traced, "iterations": trace / step rounds}."""
    import torch
    spp, max_bounces = int(spp), int(max_bounces)
    if max_bounces < 1:
        raise ValueError("max_bounces must be >= 1")
    if compact not in ("torch", "device"):
        raise ValueError('compact must be "torch" or "device"')
    if sync_every != int(sync_every) or int(sync_every) < 1:
        raise ValueError("sync_every must be an integer >= 1")
    sync_every = int(sync_every)
    if sync_every != 1 and compact != "device":
        raise ValueError('sync_every other than 1 needs compact="device"')
    if finish_below != int(finish_below) or int(finish_below) < 0:
        raise ValueError("finish_below must be an integer >= 0")
    finish_below = int(finish_below)
    if finish_below and compact != "device":
        raise ValueError('finish_below other than 0 needs compact="device"')
    opts = dict(trace_options or {})
    n_pix = renderer.width * renderer.height
    tdev = torch.device("cuda", renderer.device)
    renderer.write_linear(np.zeros((renderer.height, renderer.width, 3), np.float32))   # a render starts from 0
    total = iterations = 0
    phases = _Phases(profile)

    def bounce(rays, paths):
        phases.mark("start")
        hits = scene.trace(rays, **opts)["f32"]
        phases.mark("trace", n=rays.shape[0])
        if on_bounce is not None:
            on_bounce(rays, hits, paths)
        path_step(scene, rays, hits, paths, max_bounces, renderer, renderer)
        phases.mark("step")

    if compact == "device" and spp > 0 and sync_every > 1:
        remaining = torch.full((n_pix,), spp - 1, dtype=torch.int32, device=tdev) if regenerate else None
        pong = (torch.empty((n_pix, 8), dtype=torch.float32, device=tdev),
                torch.empty((n_pix, 8), dtype=torch.int32, device=tdev))
        hits = torch.empty((n_pix, 8), dtype=torch.float32, device=tdev)
        totals = torch.zeros((2,), dtype=torch.int64, device=tdev)
        for _ in range(1 if regenerate else spp):
            phases.mark("start")
            batches, cur = [camera_rays(renderer), pong], 0
            count = torch.full((1,), n_pix, dtype=torch.int32, device=tdev)
            m = n_pix
            while m:
                if m <= finish_below:
                    finish(scene, renderer, batches[cur][0][:m], batches[cur][1][:m], max_bounces, remaining,
                           count_in=count, totals=totals)
                    break
                for _ in range(sync_every):
                    rays, paths = batches[cur][0][:m], batches[cur][1][:m]
                    phases.mark("start")
                    scene.trace(rays, count=count, out=hits[:m], **opts)
                    phases.mark("trace", n=m)
                    if on_bounce is not None:
                        on_bounce(rays, hits[:m], paths, count)
                    _, _, count = advance(scene, renderer, rays, hits[:m], paths, max_bounces, remaining,
                                          out=batches[cur ^ 1], count_in=count, totals=totals)
                    phases.mark("advance")
                    cur ^= 1
                m = min(int(count), m)                        # the block's one wait
                phases.mark("count")
        total, iterations = (int(v) for v in totals.tolist())
    elif compact == "device" and spp > 0:
        remaining = torch.full((n_pix,), spp - 1, dtype=torch.int32, device=tdev) if regenerate else None
        pong = (torch.empty((n_pix, 8), dtype=torch.float32, device=tdev),
                torch.empty((n_pix, 8), dtype=torch.int32, device=tdev))
        for _ in range(1 if regenerate else spp):
            phases.mark("start")
            ping = camera_rays(renderer)
            rays, paths = ping
            while rays.shape[0]:
                if rays.shape[0] <= finish_below:
                    totals = torch.zeros((2,), dtype=torch.int64, device=tdev)
                    finish(scene, renderer, rays, paths, max_bounces, remaining, totals=totals)
                    total += int(totals[0])
                    iterations += 1
                    break
                total += rays.shape[0]
                iterations += 1
                phases.mark("start")
                hits = scene.trace(rays, **opts)["f32"]
                phases.mark("trace", n=rays.shape[0])
                if on_bounce is not None:
                    on_bounce(rays, hits, paths)
                _, _, count = advance(scene, renderer, rays, hits, paths, max_bounces, remaining, out=pong)
                phases.mark("advance")
                m = int(count)                                # the iteration's one wait
                phases.mark("count")
                ping, pong = pong, ping
                rays, paths = ping[0][:m], ping[1][:m]
    elif regenerate and spp > 0:
        remaining = torch.full((n_pix,), spp - 1, dtype=torch.int32, device=tdev)   # samples not yet started
        rays, paths = camera_rays(renderer)
        while rays.shape[0]:
            total += rays.shape[0]
            iterations += 1
            bounce(rays, paths)
            ended = paths[:, PATH_STATUS] == PATH_ENDED
            again = ended & (remaining[paths[:, PATH_PIXEL].long()] > 0)
            idx = again.nonzero().squeeze(1)
            new = None
            if idx.numel():
                pix = paths[idx, PATH_PIXEL].contiguous()
                remaining[pix.long()] -= 1
                phases.mark("select")
                new = camera_rays(renderer, pix)
                phases.mark("camera")
                rays[idx], paths[idx] = new
            keep = ~ended | again
            rays, paths = rays[keep], paths[keep]
            phases.mark("compact", ended=ended.sum() if profile is not None else 0)
    elif spp > 0:
        for _ in range(spp):
            phases.mark("start")
            rays, paths = camera_rays(renderer)
            phases.mark("camera")
            while rays.shape[0]:
                total += rays.shape[0]
                iterations += 1
                bounce(rays, paths)
                keep = paths[:, PATH_STATUS] == PATH_ACTIVE
                n_before = rays.shape[0]
                rays, paths = rays[keep], paths[keep]
                phases.mark("compact", ended=n_before - rays.shape[0])
    phases.close()
    return {"rays": total, "iterations": iterations}
