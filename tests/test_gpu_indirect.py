"""Device-side batch sizes on the GPU: the indirect ray query (Scene.trace / occluded with count=), the
indirect advance (paths.advance with count_in=), chains of the two without a host read, and the loops built on them
(Renderer.render_wavefront(sync_every=K), paths.render(compact="device", sync_every=K)).

Every comparison is bit for bit, on uint32 views; batches are the 2,304-entry 64x36 ones of helpers/wavefront_batches.

1. indirect trace == the direct query of the prefix, the rows from the count on keep the caller's sentinel; counts round
   the wave, the workgroup and the stream kernel's reservation sizes, and counts beyond the capacity.
2. the count is produced on the stream, just before the query.
3. indirect advance == the direct advance of the prefix, keyed by pixel; totals; sentinel beyond the count.
4. chains of indirect trace / advance with nothing read back == the same iterations with int(count) in between.
5. whole frames of both loops == Renderer.render and == Renderer.render_wavefront's rays and iterations, for every K.
6. accumulation, refusals, the shared scratch, sync_every=0.
7. on_bounce with a device count.
8. a side stream without synchronisation; the checked build in a fresh child process.
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib, paths

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import custom_scene  # noqa: E402
import stream_gate  # noqa: E402
import wavefront_batches as wb  # noqa: E402
from wavefront_batches import H, W, bits, same  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
CHECKED = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
F32 = np.float32
UNSUPPORTED = -5                      # CRT_ERR_UNSUPPORTED
RENDER_COUNT_WORK = 2                 # CRT_RENDER_COUNT_WORK
N = W * H                             # 2,304: the capacity of every batch here
# round the wave (64), the lane kernel's and the advance kernel's workgroup (256), the stream kernel's reservations (at
# grid_waves=1: 65 rays take 1 x 64 indices, 1025 take 8 x 64; at grid_waves=2 the granularity is crossed between 255,
# 256 and 257), the whole batch, and two counts beyond the capacity (0xffffffff as its int32 bit pattern)
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1025, 2303, 2304, 2305, -1)
SENTINEL = 0x5EA7BEEF                 # fits int32; no hit row and no ray row holds it
KS = (1, 2, 3, 7, 64, 1000)


def clamped(count):
    return min(count & 0xffffffff, N)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def count_tensor(count):
    import torch
    return torch.tensor([count], dtype=torch.int32, device="cuda:0")


# ------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def worlds(tmp_path_factory, scenes):
    out = custom_scene.synth_worlds(custom_scene.family_files(tmp_path_factory.mktemp("indirect")))
    out["odd_materials"] = wb.odd_materials_world(scenes)
    return out


@pytest.fixture(scope="module")
def batches(worlds):
    return {"odd_materials": wb.traced_batch(worlds["odd_materials"], True), "s9_ground": wb.traced_batch(worlds["s9_ground"], False)}


@pytest.fixture(scope="module")
def bunny_w4(device_scenes):
    return device_scenes["cornell_bunny"][0].upload(0, bvh="rebuilt", width=4)


QUERIES = {"reference lane": None, "w4 lane": dict(mode=1), "w4 stream 1 wave": dict(mode=2, grid_waves=1),
           "w4 stream 2 waves": dict(mode=2, grid_waves=2)}


def _scene(b, bunny_w4, query):
    """The batch's own scene (the reference tree: the lane kernel over threaded nodes) or the rebuilt 4-wide bunny scene."""
    return (b.scene, {}) if QUERIES[query] is None else (bunny_w4, QUERIES[query])


# ------------------------------------------------------------------------------------------ 1. indirect trace
@pytest.mark.parametrize("query", list(QUERIES))
@pytest.mark.parametrize("world", ["odd_materials", "s9_ground"])
def test_indirect_trace(batches, bunny_w4, world, query):
    import torch
    b = batches[world]
    scene, opts = _scene(b, bunny_w4, query)
    rays = dev(b.rays)
    whole = scene.trace(rays, **opts)["i32"]
    assert (whole != SENTINEL).all()
    for count in COUNTS:
        n = clamped(count)
        out = torch.full((N, 8), SENTINEL, dtype=torch.int32, device="cuda:0")
        got = scene.trace(rays, count=count_tensor(count), out=out, **opts)
        assert got["i32"].data_ptr() == out.data_ptr() and got["f32"].shape == (N, 8)
        want = scene.trace(rays[:n], **opts)["i32"] if n else whole[:0]
        assert torch.equal(out[:n], want) and torch.equal(want, whole[:n]), (count, int((out[:n] != want).sum()))
        assert (out[n:] == SENTINEL).all(), (count, "rows from the count on were written")
    assert torch.equal(rays, dev(b.rays))


@pytest.mark.parametrize("query", list(QUERIES))
def test_indirect_occlusion(batches, bunny_w4, query):
    import torch
    b = batches["odd_materials"]
    scene, opts = _scene(b, bunny_w4, query)
    rays = dev(b.rays)
    t = scene.trace(rays, **opts)["t"].cpu().numpy()
    hit = t >= 0
    assert hit.sum() > 1000
    tt = np.where(hit, t, F32(1)).astype(F32)
    for case, tmax in (("t", tt), ("below", np.nextafter(tt, F32(0))), ("above", np.nextafter(tt, F32(np.inf)))):
        r = b.rays.copy()
        r[:, 3] = tmax
        r = dev(r)
        want = torch.from_numpy((hit & (t <= tmax)).astype(np.uint8)).to("cuda:0")
        assert torch.equal(scene.occluded(r, **opts), want), case
        assert bool(want.any()) == (case != "below")
        for count in COUNTS:
            n = clamped(count)
            out = torch.full((N,), 0xA5, dtype=torch.uint8, device="cuda:0")
            got = scene.occluded(r, count=count_tensor(count), out=out, **opts)
            assert got.data_ptr() == out.data_ptr()
            if n:
                assert torch.equal(out[:n], scene.occluded(r[:n], **opts)), (case, count)
            assert torch.equal(out[:n], want[:n]) and (out[n:] == 0xA5).all(), (case, count)


@pytest.mark.parametrize("query", list(QUERIES))
def test_indirect_trace_counts_the_clamped_rays(batches, bunny_w4, query):
    b = batches["s9_ground"]
    scene, opts = _scene(b, bunny_w4, query)
    rays = dev(b.rays)
    for count in (0, 65, 1025, 2304, 2305, -1):
        scene.trace(rays, count=count_tensor(count), count_work=True, **opts)
        assert scene.trace_stats()["rays"] == clamped(count), count


# ------------------------------------------------------------------------------------------ 2. the count comes from the stream
@pytest.mark.parametrize("query", ["reference lane", "w4 stream 2 waves"])
def test_count_is_read_on_the_stream(batches, bunny_w4, query):
    """The count is the result of torch ops enqueued on a side stream just before the query, with no synchronisation in
    between: a host that read the word when it enqueued the query would see the 0 the tensor was created with."""
    import torch
    b = batches["odd_materials"]
    scene, opts = _scene(b, bunny_w4, query)
    rays = dev(b.rays)
    whole = scene.trace(rays, **opts)["i32"]
    flags = torch.zeros((N,), dtype=torch.int32, device="cuda:0")
    flags[:1025] = 1
    torch.cuda.synchronize()
    side = stream_gate.side_stream()
    source, rays = rays, torch.zeros_like(rays)             # what a query on another stream would trace
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        stream_gate.gate(side)
        rays.copy_(source)                                   # the rays arrive on this stream, behind the gate
        count = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
        out = torch.full((N, 8), SENTINEL, dtype=torch.int32, device="cuda:0")
        count += flags.sum().to(torch.int32)
        scene.trace(rays, count=count, out=out, **opts)
    side.synchronize()
    assert int(count) == 1025
    assert torch.equal(out[:1025], whole[:1025]) and (out[1025:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------ 3. indirect advance
def _remaining(pattern, n_pix):
    if pattern == "none":
        return None
    if pattern == "alternating":
        return (np.arange(n_pix) % 2).astype(np.int32)
    return np.full(n_pix, {"zero": 0, "positive": 2}[pattern], np.int32)


def _indirect_advance(b, count, remaining, totals):
    """paths.advance(count_in=) over the whole batch on copies of the state, into a pair filled with the sentinel."""
    import torch
    rays, hits, p, rng, lin, rem = b._device(np.arange(N), None, remaining)
    out = (torch.full((N, 8), float(SENTINEL), dtype=torch.float32, device="cuda:0"),
           torch.full((N, 8), SENTINEL, dtype=torch.int32, device="cuda:0"))
    rays_out, pth_out, c = b.scene.path_advance(b.r, rays, hits, p, 20, rem, rng=rng, linear=lin, out=out,
                                                count_in=count_tensor(count), totals=totals)
    assert rays_out.data_ptr() == out[0].data_ptr() and c.shape == (1,) and c.dtype == torch.int32
    res = b._result(rays_out, pth_out, int(c), rng, lin, rem)
    m = res["count"]
    assert (out[0][m:] == float(SENTINEL)).all() and (out[1][m:] == SENTINEL).all(), "outputs beyond the count were written"
    assert same(rays.cpu().numpy(), b.rays) and same(hits.cpu().numpy(), b.hits) and same(p.cpu().numpy(), b.pth)
    return res


@pytest.mark.parametrize("pattern", ["zero", "positive", "alternating", "none"])
@pytest.mark.parametrize("world", ["odd_materials", "s9_ground"])
def test_indirect_advance(batches, world, pattern):
    import torch
    b = batches[world]
    rem = _remaining(pattern, b.n_pix)
    for count in COUNTS:
        n = clamped(count)
        want = b.advance(np.arange(n), rem)
        totals = torch.tensor([5, 7], dtype=torch.int64, device="cuda:0")
        got = _indirect_advance(b, count, rem, totals)
        wb.assert_equal_results(got, want, f"{world} / {pattern} / count {count}")
        assert got["count"] <= n
        assert totals.tolist() == [5 + n, 7 + (n > 0)], (count, totals.tolist())
        wb.assert_equal_results(_indirect_advance(b, count, rem, totals), want, f"{world} / {pattern} / count {count}, again")
        assert totals.tolist() == [5 + 2 * n, 7 + 2 * (n > 0)], (count, totals.tolist())
    assert _indirect_advance(b, 1025, rem, None)["count"] == b.advance(np.arange(1025), rem)["count"]   # totals are optional


# ------------------------------------------------------------------------------------------ 4. chains without host reads
def _chain(scene, r, rng0, iterations, indirect, opts, gated=False):
    """Camera rays, then `iterations` rounds of trace and advance on ping-pong batches and the caller's own state, 3
    more samples per pixel.  indirect: every size comes from the device and nothing is read back before the end;
    otherwise the direct calls with int(count) between them, which stop when no entry is left.  gated: the current
    stream is held back first (helpers/stream_gate.py), and the state and the first count are made on it behind the gate."""
    import torch
    rng, first_count = dev(rng0.view(np.int32)), count_tensor(N)
    if gated:
        torch.cuda.synchronize()
        stream_gate.gate(torch.cuda.current_stream())
        rng, first_count = rng.clone(), first_count.clone()
    lin = torch.zeros((N, 3), dtype=torch.float32, device="cuda:0")
    rem = torch.full((N,), 3, dtype=torch.int32, device="cuda:0")
    totals = torch.zeros((2,), dtype=torch.int64, device="cuda:0")
    torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())
    batch = [crt_amd.camera_rays(r, rng=rng), (torch.empty((N, 8), dtype=torch.float32, device="cuda:0"),
                                               torch.empty((N, 8), dtype=torch.int32, device="cuda:0"))]
    hits = torch.empty((N, 8), dtype=torch.float32, device="cuda:0")
    count, m, cur, done = first_count, N, 0, 0
    for _ in range(iterations):
        rays, pth = batch[cur]
        if indirect:
            scene.trace(rays, count=count, out=hits, **opts)
            _, _, count = scene.path_advance(r, rays, hits, pth, 20, rem, rng=rng, linear=lin, out=batch[cur ^ 1],
                                             count_in=count, totals=totals)
        else:
            if m == 0:
                break
            h = scene.trace(rays[:m], **opts)["f32"]
            _, _, count = scene.path_advance(r, rays[:m], h, pth[:m], 20, rem, rng=rng, linear=lin, out=batch[cur ^ 1])
            totals += torch.tensor([m, 1], dtype=torch.int64, device="cuda:0")
            m = int(count)
        cur ^= 1
        done += 1
    torch.cuda.current_stream().synchronize()
    m = int(count)
    return {"rows": wb.keyed(batch[cur][0].cpu().numpy(), batch[cur][1].cpu().numpy(), m), "count": m,
            "rng": rng.cpu().numpy().view(np.uint32), "lin": lin.cpu().numpy(), "remaining": rem.cpu().numpy(),
            "totals": totals.tolist(), "done": done}


@pytest.fixture(scope="module")
def chain_state():
    r = wb.renderer(crt_amd.camera(4))
    r.synchronize()
    return r, r.rng_state().reshape(-1, 6)


@pytest.mark.parametrize("query", ["reference lane", "w4 stream 2 waves"])
@pytest.mark.parametrize("iterations", [1, 2, 5, 24, 120])
def test_chain_without_host_reads(device_scenes, bunny_w4, chain_state, iterations, query):
    r, rng0 = chain_state
    scene, opts = (device_scenes["cornell_bunny"][1], {}) if QUERIES[query] is None else (bunny_w4, QUERIES[query])
    want = _chain(scene, r, rng0, iterations, False, opts)
    got = _chain(scene, r, rng0, iterations, True, opts)
    wb.assert_equal_results(got, want, f"{iterations} iterations")
    assert got["totals"] == want["totals"] and got["totals"][0] > 0, (got["totals"], want["totals"])
    assert got["done"] == iterations and got["totals"][1] == want["done"]
    if iterations == 120:
        # 4 samples of at most 20 rays each: the count reached 0 well before the end, and the indirect iterations
        # after that changed nothing
        assert want["done"] < 100 and got["count"] == 0 and (got["remaining"] == 0).all()
    assert same(r.rng_state().reshape(-1, 6), rng0)        # the renderer's own state was not used


# ------------------------------------------------------------------------------------------ 5. whole frames
def _frame(r, spp):
    r.resolve(crt_amd.pixel_sample_scale(max(spp, 1)))
    r.synchronize()
    return {"sum": r.linear(), "rgba": r.rgba8(), "rng": r.rng_state()}


def _assert_frames_equal(got, want, what):
    for k in ("sum", "rgba", "rng"):
        assert same(got[k], want[k]), f"{what}: {k} differs in {int((bits(got[k]) != bits(want[k])).sum())} words"
    assert got["rays"] == want["rays"], (what, got["rays"], want["rays"])


class Frames:
    """The frames of one case, each computed once.  Kinds: "direct" (Renderer.render), "library" (the existing
    Renderer.render_wavefront), ("queued", K) (Renderer.render_wavefront(sync_every=K)) and ("python", K)
    (paths.render(compact="device", sync_every=K))."""

    def __init__(self, device_scenes, worlds, bunny_w4):
        self.scenes = {"bunny_w4": bunny_w4, **{k: v[1] for k, v in device_scenes.items()}}
        self.worlds, self.memo = worlds, {}

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = self.worlds[name].upload(0)
        return self.scenes[name]

    def get(self, kind, scene, spp, bounces, w=W, h=H, query=None, regenerate=True):
        if kind == "direct":
            query = None
        if kind == "direct" or kind[0] != "python":
            regenerate = True
        key = (kind, scene, spp, bounces, w, h, query, regenerate)
        if key not in self.memo:
            sc = self.scene(scene)
            r = wb.renderer(crt_amd.camera(max(spp, 1)), w, h)
            opts = {None: {}, "lane": dict(mode=1), "stream": dict(mode=2, grid_waves=1)}[query]
            if kind == "direct":
                r.render(sc, spp, bounces, count_work=True)
                res = {"rays": r.counters()["rays"]}
            elif kind == "library":
                res = r.render_wavefront(sc, spp, bounces, trace_options=opts)
            elif kind[0] == "queued":
                res = r.render_wavefront(sc, spp, bounces, trace_options=opts, sync_every=kind[1])
            else:
                res = paths.render(sc, r, spp, bounces, regenerate=regenerate, trace_options=opts, compact="device",
                                   sync_every=kind[1])
            self.memo[key] = dict(_frame(r, spp), **res)
        return self.memo[key]

    def check(self, k, scene, spp, bounces, regenerate=None, **kw):
        """Both loops at sync_every = k against Renderer.render's frame and the existing loop's rays and iterations."""
        size = {a: v for a, v in kw.items() if a in ("w", "h")}
        direct, library = self.get("direct", scene, spp, bounces, **size), self.get("library", scene, spp, bounces, **kw)
        out = {}
        for kind, more in ((("queued", k), {}), (("python", k), {} if regenerate is None else {"regenerate": regenerate})):
            got = self.get(kind, scene, spp, bounces, **kw, **more)
            what = f"{kind} {scene} {spp} spp {bounces} bounces {kw} {more}"
            _assert_frames_equal(got, direct, what)
            if more.get("regenerate", True):
                assert (got["rays"], got["iterations"]) == (library["rays"], library["iterations"]), what
            out[kind[0]] = got
        return out


@pytest.fixture(scope="module")
def frames(device_scenes, worlds, bunny_w4):
    return Frames(device_scenes, worlds, bunny_w4)


@pytest.mark.parametrize("k", KS)
def test_golden_frame(frames, k):
    g = np.load(GOLDEN / "cornell_bunny_64x36_16spp.npz")
    for got in frames.check(k, "cornell_bunny", 16, 20).values():
        assert same(got["sum"], g["sum"]) and np.array_equal(got["rgba"], g["rgba"])
    assert frames.get("library", "cornell_bunny", 16, 20)["iterations"] > 64    # K = 64 takes more than one block


@pytest.mark.parametrize("k", KS)
def test_partial_last_wave(frames, k):
    frames.check(k, "cornell_bunny", 16, 20, w=65, h=37)


@pytest.mark.parametrize("bounces", [1, 20])
def test_config_a(frames, bounces):
    got = frames.check(7, "cornell", 16, bounces, w=256, h=256)
    assert bounces != 1 or got["queued"]["rays"] == 16 * 256 * 256


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("query", ["lane", "stream"])
def test_rebuilt_tree(frames, query, k):
    frames.check(k, "bunny_w4", 16, 20, query=query)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["odd_materials", "s0"])
def test_synthetic_worlds(frames, name, k):
    frames.check(k, name, 4, 20)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("spp", [0, 1])
def test_no_and_one_sample(frames, spp, k):
    for got in frames.check(k, "cornell_bunny", spp, 20).values():
        assert (got["rays"] == 0 and got["iterations"] == 0 and not got["sum"].any()) if spp == 0 else got["rays"] > N


@pytest.mark.parametrize("k", KS)
def test_sample_by_sample(frames, k):
    """regenerate=False: every sample runs until its last path ends, so its rounds differ from the library's loop; the
    frame, the rays and the rounds of the sync_every=1 driver stay."""
    got = frames.check(k, "cornell_bunny", 4, 20, regenerate=False)["python"]
    one = frames.get(("python", 1), "cornell_bunny", 4, 20, regenerate=False)
    assert (got["rays"], got["iterations"]) == (one["rays"], one["iterations"])


# ------------------------------------------------------------------------------------------ 6. the entry's other behaviour
def test_queued_accumulates_refuses_and_shares_the_scratch(frames):
    scene = frames.scene("cornell_bunny")
    cam = crt_amd.camera(16)
    a, b = wb.renderer(cam), wb.renderer(cam)
    zero = np.zeros((H, W, 3), F32)
    a.write_linear(zero)
    b.write_linear(zero)
    rays = 0
    for _ in range(2):
        a.render(scene, 8, 20, accumulate=True, count_work=True)
        a.synchronize()
        rays += a.counters()["rays"]
    res = [b.render_wavefront(scene, 8, 20, accumulate=True, sync_every=5) for _ in range(2)]
    got, want = _frame(b, 16), _frame(a, 16)
    _assert_frames_equal(dict(got, rays=res[0]["rays"] + res[1]["rays"]), dict(want, rays=rays), "two accumulating calls")
    assert got["sum"].any()
    # refusals leave the sums and the RNG state as they are
    fn = _lib.hip().crt_renderer_render_wavefront_queued
    st = _lib.WavefrontStats()
    assert fn(b.h, scene.h, 8, 20, RENDER_COUNT_WORK, None, 4, C.byref(st), None) == UNSUPPORTED
    b.set_pixel_shard(1, 2)
    assert fn(b.h, scene.h, 8, 20, 0, None, 4, C.byref(st), None) == UNSUPPORTED
    with pytest.raises(crt_amd.CrtError, match="shard"):
        b.render_wavefront(scene, 8, 20, sync_every=4)
    b.set_pixel_shard(0, 1)
    b.synchronize()
    assert same(b.linear(), got["sum"]) and same(b.rng_state(), got["rng"])
    # the two loops share the handle's scratch: a frame of each, one after the other
    direct, library = frames.get("direct", "cornell_bunny", 16, 20), frames.get("library", "cornell_bunny", 16, 20)
    for sync_every in (None, 4, None, 0):
        b.init_rand(41)
        again = b.render_wavefront(scene, 16, 20, sync_every=sync_every)
        _assert_frames_equal(dict(_frame(b, 16), rays=again["rays"]), direct, f"frame with sync_every={sync_every}")
        assert again["iterations"] == library["iterations"] and again["ms"] > 0
    assert b.render_wavefront(scene, 0, 20, sync_every=4) == {"rays": 0, "iterations": 0, "ms": 0.0}
    assert not b.linear().any()


# ------------------------------------------------------------------------------------------ 7. on_bounce
def test_on_bounce_gets_the_device_count(frames):
    import torch
    seen = torch.zeros((1,), dtype=torch.int64, device="cuda:0")
    bounds = []

    def hook(*args):
        assert len(args) == 4
        rays, hits, pth, count = args
        assert rays.shape == hits.shape == pth.shape and count.shape == (1,) and count.dtype == torch.int32 and count.is_cuda
        bounds.append(rays.shape[0])
        seen.add_(count)                                    # on the device: the hook does not wait either

    r = wb.renderer(crt_amd.camera(4))
    res = paths.render(frames.scene("cornell_bunny"), r, 4, 20, on_bounce=hook, compact="device", sync_every=4)
    direct = frames.get("direct", "cornell_bunny", 4, 20)
    assert int(seen) == res["rays"] == direct["rays"]
    assert len(bounds) % 4 == 0 and res["iterations"] <= len(bounds) < res["iterations"] + 4
    assert bounds == sorted(bounds, reverse=True) and bounds[0] == N and sum(bounds) >= res["rays"]
    _assert_frames_equal(dict(_frame(r, 4), rays=res["rays"]), direct, "with a hook")


def test_on_bounce_edits_rows_below_the_count(frames):
    import torch
    scene = frames.scene("cornell_bunny")

    def hook(rays, hits, pth, count=None):
        """Ends every path that is at bounce 2."""
        at_2 = pth[:, paths.PATH_BOUNCE] == 2
        if count is not None:
            at_2 &= torch.arange(pth.shape[0], device=pth.device) < count
        pth[:, paths.PATH_STATUS] = torch.where(at_2, _lib.PATH_ENDED, pth[:, paths.PATH_STATUS])

    got = {}
    for k in (1, 4):
        r = wb.renderer(crt_amd.camera(4))
        res = paths.render(scene, r, 4, 20, on_bounce=hook, compact="device", sync_every=k)
        got[k] = dict(_frame(r, 4), **res)
    _assert_frames_equal(got[4], got[1], "a hook that ends paths")
    assert got[4]["iterations"] == got[1]["iterations"]
    assert got[1]["rays"] < frames.get("direct", "cornell_bunny", 4, 20)["rays"] and got[1]["sum"].any()


# ------------------------------------------------------------------------------------------ 8. side stream, checked build
def test_side_stream(bunny_w4, chain_state):
    import torch
    r, rng0 = chain_state
    opts = dict(mode=2, grid_waves=8)
    base = _chain(bunny_w4, r, rng0, 6, True, opts)
    torch.cuda.synchronize()
    side = stream_gate.side_stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side and side != torch.cuda.default_stream()
        got = _chain(bunny_w4, r, rng0, 6, True, opts, gated=True)
    wb.assert_equal_results(got, base, "side stream")
    assert got["totals"] == base["totals"] and base["totals"] == [6 * N, 6] and base["lin"].any()
    # the library's loop on a side stream
    a, b = wb.renderer(crt_amd.camera(4)), wb.renderer(crt_amd.camera(4))
    b.init_rand(7)                                          # what a loop on another stream would start from
    torch.cuda.synchronize()
    stream_gate.gate(side)
    b.init_rand(41, stream=side.cuda_stream)                # a's state, made on the side stream behind the gate
    res = [a.render_wavefront(bunny_w4, 4, 20, sync_every=3),
           b.render_wavefront(bunny_w4, 4, 20, sync_every=3, stream=side.cuda_stream)]
    side.synchronize()
    _assert_frames_equal(dict(_frame(b, 4), rays=res[1]["rays"]), dict(_frame(a, 4), rays=res[0]["rays"]), "queued loop on a side stream")


CHILD = r"""
import sys
from pathlib import Path
import numpy as np
repo = Path(sys.argv[1])
sys.path[:0] = [str(repo / "raytracer-cuda_amd"), str(repo / "oracle")]
import crt_amd
from crt_amd import _lib, assets, paths
hs = crt_amd.HostScene(assets.scene_files("cornell_bunny"))
sc = hs.upload(0, bvh="rebuilt", width=4)
out = {"flags": np.array(_lib.hip().crt_build_flags())}
for kind in ("python", "queued"):
    r = crt_amd.Renderer(64, 36)
    r.set_camera(crt_amd.camera(2))
    r.init_rand(41)
    if kind == "python":
        res = paths.render(sc, r, 2, 20, compact="device", sync_every=4, trace_options=dict(mode=2, grid_waves=2))
    else:
        res = r.render_wavefront(sc, 2, 20, sync_every=4)
    r.resolve(crt_amd.pixel_sample_scale(2))
    r.synchronize()                                      # a device error of the checked build raises here
    out.update({kind + "_sum": r.linear(), kind + "_rgba": r.rgba8(), kind + "_rng": r.rng_state(),
                kind + "_rays": np.array(res["rays"]), kind + "_iterations": np.array(res["iterations"])})
np.savez(sys.argv[2], **out)
"""


def test_checked_build_gives_the_same_bits(frames, tmp_path):
    assert CHECKED.exists() and _lib.hip().crt_build_flags() == 0
    res = tmp_path / "checked.npz"
    p = subprocess.run([sys.executable, "-c", CHILD, str(REPO), str(res)], env=dict(os.environ, CRT_HIP_LIB=str(CHECKED)),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(res)
    assert int(got["flags"]) == _lib.BUILD_CHECKED
    want = frames.get("direct", "bunny_w4", 2, 20)
    library = frames.get("library", "bunny_w4", 2, 20)
    for kind in ("python", "queued"):
        _assert_frames_equal({k: got[f"{kind}_{k}"] for k in ("sum", "rgba", "rng")} | {"rays": int(got[f"{kind}_rays"])},
                             want, f"checked build, {kind}")
        assert int(got[f"{kind}_iterations"]) == library["iterations"]
