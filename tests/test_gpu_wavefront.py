"""Path queues on the GPU: the fused step / regenerate / compact kernel (paths.advance), the driver on
it (paths.render(compact="device")) and the whole loop in the library (Renderer.render_wavefront).

Every comparison is bit for bit, on uint32 views; frames are 64x36 unless stated.

1. advance == its composition out of the parent's functions (path_step, camera_rays on the ended pixels with samples
   left, torch compaction), keyed by pixel: rows, count, RNG state, sums, remaining; batch lengths round the wave, the
   workgroup and a workgroup's whole reservation; remaining all 0 / all positive / alternating / None; entries that come
   in ENDED or name no pixel; n = 0; a permuted batch; a caller's own output pair.
2. paths.render(compact="device") == Renderer.render (sums, RGBA8, RNG state, rays) and == compact="torch" (iterations).
3. Renderer.render_wavefront == the same, accumulation, refusals, a second frame on the same handle; the plain, the
   queued and the finish loop refuse alike, word for word.
4. on_bounce under device compaction.
5. a side stream without synchronisation == the default stream.
6. the checked build in a fresh child process gives the same bits.
"""
import ctypes as C
import hashlib
import json
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


# ------------------------------------------------------------------------------------------ 1. advance == composition
@pytest.fixture(scope="module")
def worlds(tmp_path_factory, scenes):
    out = custom_scene.synth_worlds(custom_scene.family_files(tmp_path_factory.mktemp("wf")))
    out["odd_materials"] = wb.odd_materials_world(scenes)
    return out


@pytest.fixture(scope="module")
def batches(worlds):
    """odd_materials: a batch with every kind of entry (misses, the five material codes, the invalid index, glass hit
    from inside, absorbed metal); s9_ground: a batch of a sphere world."""
    return {"odd_materials": wb.traced_batch(worlds["odd_materials"], True), "s9_ground": wb.traced_batch(worlds["s9_ground"], False)}


def _remaining(pattern, n_pix):
    if pattern == "none":
        return None
    if pattern == "alternating":
        return (np.arange(n_pix) % 2).astype(np.int32)
    return np.full(n_pix, {"zero": 0, "positive": 2}[pattern], np.int32)


PATTERNS = ("zero", "positive", "alternating", "none")


def test_batch_holds_every_kind_of_entry(batches):
    b = batches["odd_materials"]
    assert len(b.rays) == W * H and all(v.any() for v in b.cls.values()), {k: int(v.sum()) for k, v in b.cls.items()}
    assert _lib.hip().crt_path_advance_entries() in (64, 256, 512, 768, 1024)


@pytest.mark.parametrize("world", ["odd_materials", "s9_ground"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_whole_batch(batches, world, pattern):
    b = batches[world]
    idx = np.arange(len(b.rays))
    rem = _remaining(pattern, b.n_pix)
    want = b.composed(idx, rem)
    got = b.advance(idx, rem)
    print(f"\n{world} / {pattern}: {got['count']} of {len(idx)} entries appended")
    wb.assert_equal_results(got, want, f"{world} / {pattern}")
    goes_on, ends = int(b.cls["goes on"].sum()), int(b.cls["ends"].sum())
    if pattern in ("zero", "none"):
        assert got["count"] == goes_on
    elif pattern == "positive":
        assert got["count"] == len(idx) and (got["remaining"] == 2 - b.cls["ends"][np.argsort(b.pth[:, paths.PATH_PIXEL])].astype(np.int32)).all()
    else:
        assert goes_on < got["count"] < goes_on + ends
    # the same batch permuted gives the same keyed result
    perm = np.random.default_rng(4).permutation(len(idx))
    wb.assert_equal_results(b.advance(perm, rem), want, f"{world} / {pattern} permuted")


def _lengths():
    """Round the wave, round the workgroup, and one above a workgroup's whole reservation (4 x 256 + 1 at the least)."""
    return [1, 63, 64, 65, 129, 255, 256, 257, 4 * 256 + 1]


@pytest.mark.parametrize("n", _lengths())
def test_batch_lengths(batches, n):
    b = batches["odd_materials"]
    assert n > max(_lib.hip().crt_path_advance_entries(), 1024) or n <= 257
    for idx in (np.arange(n), np.arange(len(b.rays) - n, len(b.rays))):
        for pattern in PATTERNS:
            rem = _remaining(pattern, b.n_pix)
            wb.assert_equal_results(b.advance(idx, rem), b.composed(idx, rem), f"{n} entries from {idx[0]} / {pattern}")


def test_everything_ends_with_no_sample_left(batches):
    b = batches["odd_materials"]
    idx = np.nonzero(b.cls["ends"])[0]
    assert len(idx) > 256
    for rem in (_remaining("zero", b.n_pix), None):
        got = b.advance(idx, rem)
        assert got["count"] == 0 and got["rows"].shape == (0, 16)
        wb.assert_equal_results(got, b.composed(idx, rem), "all ended")
        assert not same(got["lin"], b.lin) and not same(got["rng"], b.rng)     # they did run


def test_ended_and_out_of_frame_entries_are_dropped(batches):
    b = batches["odd_materials"]
    n = len(b.rays)
    pth = b.pth.copy()
    off = np.zeros(n, bool)
    off[::3] = True
    pth[off, paths.PATH_STATUS] = _lib.PATH_ENDED
    outside = [1, 2, 4]                                     # active entries that name no pixel of the frame
    pth[outside, paths.PATH_PIXEL] = [b.n_pix, -1, 2 ** 30]
    gone = off.copy()
    gone[outside] = True
    idx = np.arange(n)
    for pattern in ("positive", "none"):
        rem = _remaining(pattern, b.n_pix)
        got = b.advance(idx, rem, pth)
        wb.assert_equal_results(got, b.composed(idx, rem, pth), f"dropped entries / {pattern}")
        pix_gone = b.pth[gone, paths.PATH_PIXEL]
        assert same(got["rng"][pix_gone], b.rng[pix_gone]) and same(got["lin"][pix_gone], b.lin[pix_gone])
        assert rem is None or (got["remaining"][pix_gone] == 2).all()
        assert not np.isin(got["rows"][:, 8 + paths.PATH_PIXEL].view(np.int32), pix_gone).any()
        assert got["count"] == ((~gone).sum() if rem is not None else (~gone & b.cls["goes on"]).sum())


def test_empty_batch_and_own_output(batches):
    import torch
    b = batches["odd_materials"]
    none = np.arange(0)
    got = b.advance(none, _remaining("positive", b.n_pix))
    assert got["count"] == 0 and same(got["rng"], b.rng) and same(got["lin"], b.lin) and (got["remaining"] == 2).all()
    # a caller's own pair, longer than the batch: rows [0, count) are the result, the rest is not examined
    out = (torch.full((300, 8), 7.0, dtype=torch.float32, device="cuda:0"), torch.full((300, 8), 7, dtype=torch.int32, device="cuda:0"))
    idx = np.arange(257)
    rem = _remaining("alternating", b.n_pix)
    got = b.advance(idx, rem, out=out)
    wb.assert_equal_results(got, b.composed(idx, rem), "own output pair")
    assert (out[1][257:] == 7).all() and (out[0][257:] == 7).all()            # nothing beyond the batch's length


# ------------------------------------------------------------------------------------------ 2. / 3. whole frames
def _frame(r, spp):
    r.resolve(crt_amd.pixel_sample_scale(max(spp, 1)))
    r.synchronize()
    return {"sum": r.linear(), "rgba": r.rgba8(), "rng": r.rng_state()}


def _assert_frames_equal(got, want, what):
    for k in ("sum", "rgba", "rng"):
        assert same(got[k], want[k]), f"{what}: {k} differs in {int((bits(got[k]) != bits(want[k])).sum())} words"
    assert got["rays"] == want["rays"], (what, got["rays"], want["rays"])


class Frames:
    """The frames of one case, each computed once: Renderer.render's, and the drivers'."""

    def __init__(self, device_scenes, worlds):
        self.device_scenes, self.worlds, self.scenes, self.memo = device_scenes, worlds, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            if name == "bunny_w4":
                self.scenes[name] = self.device_scenes["cornell_bunny"][0].upload(0, bvh="rebuilt", width=4)
            elif name in self.device_scenes:
                self.scenes[name] = self.device_scenes[name][1]
            else:
                self.scenes[name] = self.worlds[name].upload(0)
        return self.scenes[name]

    def get(self, kind, scene, spp, bounces, w=W, h=H, query=None, regenerate=True):
        if kind == "direct":
            query, regenerate = None, True
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
            else:
                res = paths.render(sc, r, spp, bounces, regenerate=regenerate, trace_options=opts, compact=kind)
            self.memo[key] = dict(_frame(r, spp), **res)
        return self.memo[key]

    def check(self, kind, scene, spp, bounces, **kw):
        """The frame of driver `kind` against Renderer.render's and the torch driver's iterations."""
        got = self.get(kind, scene, spp, bounces, **kw)
        what = f"{kind} {scene} {spp} spp {bounces} bounces {kw}"
        _assert_frames_equal(got, self.get("direct", scene, spp, bounces, **{k: v for k, v in kw.items() if k in ("w", "h")}), what)
        torch_driver = self.get("torch", scene, spp, bounces, **kw)
        assert got["iterations"] == torch_driver["iterations"] and got["rays"] == torch_driver["rays"], what
        return got


@pytest.fixture(scope="module")
def frames(device_scenes, worlds):
    return Frames(device_scenes, worlds)


@pytest.mark.parametrize("regenerate", [True, False])
def test_golden_frame(frames, regenerate):
    g = np.load(GOLDEN / "cornell_bunny_64x36_16spp.npz")
    want = json.loads((GOLDEN / "frames.json").read_text())["cornell_bunny_64x36_16spp_20b"]
    got = frames.check("device", "cornell_bunny", 16, 20, regenerate=regenerate)
    print(f"\nregenerate={regenerate}: {got['rays']} rays in {got['iterations']} iterations")
    assert same(got["sum"], g["sum"]) and np.array_equal(got["rgba"], g["rgba"]) and got["rays"] == want["rays"]


def test_partial_last_wave(frames):
    frames.check("device", "cornell_bunny", 16, 20, w=65, h=37)


@pytest.mark.parametrize("bounces", [1, 3, 4, 20])
def test_config_a(frames, bounces):
    got = frames.check("device", "cornell", 16, bounces, w=256, h=256)
    assert bounces != 1 or got["rays"] == 16 * 256 * 256
    want = json.loads((GOLDEN / "frames.json").read_text()).get(f"configA_256x256_16spp_{bounces}b")
    assert (want is not None) == (bounces in (4, 20))
    if want:
        sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()   # noqa: E731
        assert got["rays"] == want["rays"]
        assert sha(got["sum"]) == want["sum_sha256"] and sha(got["rgba"]) == want["rgba_sha256"]


@pytest.mark.parametrize("query", ["lane", "stream"])
def test_rebuilt_tree(frames, query):
    frames.check("device", "bunny_w4", 16, 20, query=query)


@pytest.mark.parametrize("name", ["soup", "s0", "s1", "s9_ground", "s40", "odd_materials"])
def test_synthetic_worlds(frames, name):
    for regenerate in (True, False):
        frames.check("device", name, 4, 20, regenerate=regenerate)


@pytest.mark.parametrize("spp", [0, 1])
def test_no_and_one_sample(frames, spp):
    for regenerate in (True, False):
        got = frames.check("device", "cornell_bunny", spp, 20, regenerate=regenerate)
        assert (got["rays"] == 0 and got["iterations"] == 0 and not got["sum"].any()) if spp == 0 else got["rays"] > W * H


# ------------------------------------------------------------------------------------------ 3. Renderer.render_wavefront
@pytest.mark.parametrize("case", ["golden", "65x37", "rebuilt lane", "rebuilt stream", "odd_materials"])
def test_render_wavefront(frames, case):
    scene, spp, kw = {"golden": ("cornell_bunny", 16, {}), "65x37": ("cornell_bunny", 16, dict(w=65, h=37)),
                      "rebuilt lane": ("bunny_w4", 16, dict(query="lane")), "rebuilt stream": ("bunny_w4", 16, dict(query="stream")),
                      "odd_materials": ("odd_materials", 4, {})}[case]
    got = frames.check("library", scene, spp, 20, **kw)
    device = frames.get("device", scene, spp, 20, **kw)
    assert (got["rays"], got["iterations"]) == (device["rays"], device["iterations"]) and got["ms"] > 0
    if case == "golden":
        g = np.load(GOLDEN / "cornell_bunny_64x36_16spp.npz")
        assert same(got["sum"], g["sum"]) and np.array_equal(got["rgba"], g["rgba"])


def test_render_wavefront_accumulates_refuses_and_reuses_its_scratch(frames):
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
    res = [b.render_wavefront(scene, 8, 20, accumulate=True) for _ in range(2)]
    got, want = _frame(b, 16), _frame(a, 16)
    _assert_frames_equal(dict(got, rays=res[0]["rays"] + res[1]["rays"]), dict(want, rays=rays), "two accumulating calls")
    assert got["sum"].any()
    # refusals leave the sums and the RNG state as they are
    fn = _lib.hip().crt_renderer_render_wavefront
    st = _lib.WavefrontStats()
    assert fn(b.h, scene.h, 8, 20, RENDER_COUNT_WORK, None, C.byref(st), None) == UNSUPPORTED
    b.set_pixel_shard(1, 2)
    assert fn(b.h, scene.h, 8, 20, 0, None, C.byref(st), None) == UNSUPPORTED
    with pytest.raises(crt_amd.CrtError, match="shard"):
        b.render_wavefront(scene, 8, 20)
    b.set_pixel_shard(0, 1)
    b.synchronize()
    assert same(b.linear(), got["sum"]) and same(b.rng_state(), got["rng"])
    # a second frame on the same handle, not accumulating: the scratch is reused, the sums start from 0
    b.init_rand(41)
    again = b.render_wavefront(scene, 16, 20)
    _assert_frames_equal(dict(_frame(b, 16), rays=again["rays"]), frames.get("direct", "cornell_bunny", 16, 20), "second frame")
    assert again["iterations"] == frames.get("device", "cornell_bunny", 16, 20)["iterations"]
    # no sample: the sums are cleared, nothing is traced
    assert b.render_wavefront(scene, 0, 20) == {"rays": 0, "iterations": 0, "ms": 0.0}
    assert not b.linear().any()


INVALID = -1                          # CRT_ERR_INVALID_ARGUMENT
RENDER_ACCUMULATE = 1                 # CRT_RENDER_ACCUMULATE
# What the three loops answer to a call they refuse, word for word from the library's source (crt_paths.h), in the order
# the library checks: (status, crt_last_error()).  The camera is looked at before the work-counter flag.
REFUSALS = {
    "negative spp": (INVALID, "render wavefront: negative spp"),
    "no bounce": (INVALID, "render wavefront: max_bounces must be >= 1"),
    "sync_every": (INVALID, "render wavefront: sync_every must be >= 0"),                 # the two queued entries only
    "unknown flag": (INVALID, "render wavefront: unknown flag"),
    "no camera": (INVALID, "render wavefront: camera not set"),
    "count work": (UNSUPPORTED, "render wavefront: work counters are the render kernels' (crt_renderer_render)"),
    "pixel shard": (UNSUPPORTED, "render wavefront: pixel sharding is crt_renderer_render's"),
}
FINISH_BELOW = (INVALID, "render wavefront: finish_below must be >= 0, or -1 for the default")   # the finish entry only


def test_the_three_loops_refuse_alike():
    """crt_renderer_render_wavefront, _queued and _finish through the library's own entries (the Python front-end
    refuses some of these calls itself): the same status and the same text for the same bad input, the library's own
    order of the checks, and the same answer to a frame of no samples.  No frame is rendered."""
    import synth_scenes as synth
    L = _lib.hip()
    scene = custom_scene.CustomScene([], synth.SPHERES_ONLY["only3"], synth.SPHERE_MATS).upload(0)
    r = crt_amd.Renderer(16, 8)
    st = _lib.WavefrontStats()

    def loop(entry, spp=1, bounces=20, flags=0, sync_every=0, finish_below=0):
        """(status, crt_last_error()) of one of the three entries."""
        if entry == "plain":
            rc = L.crt_renderer_render_wavefront(r.h, scene.h, spp, bounces, flags, None, C.byref(st), None)
        elif entry == "queued":
            rc = L.crt_renderer_render_wavefront_queued(r.h, scene.h, spp, bounces, flags, None, sync_every, C.byref(st), None)
        else:
            rc = L.crt_renderer_render_wavefront_finish(r.h, scene.h, spp, bounces, flags, None, sync_every, finish_below,
                                                        C.byref(st), None)
        return rc, L.crt_last_error().decode() if rc else ""

    def refused(what, want, only=("plain", "queued", "finish"), **kw):
        got = {entry: loop(entry, **kw) for entry in only}
        assert all(g == want for g in got.values()), (what, want, got)

    bad = {"negative spp": dict(spp=-1), "no bounce": dict(bounces=0), "unknown flag": dict(flags=4),
           "count work": dict(flags=RENDER_COUNT_WORK)}
    # the renderer has no camera yet: every input that the library looks at before the camera is still named first
    refused("no camera", REFUSALS["no camera"])
    for what in ("negative spp", "no bounce", "unknown flag"):
        refused(what + ", no camera", REFUSALS[what], **bad[what])
    refused("no camera, count work", REFUSALS["no camera"], **bad["count work"])
    r.set_camera(crt_amd.camera(1))
    r.init_rand(41)
    # each input alone
    for what, kw in bad.items():
        refused(what, REFUSALS[what], **kw)
    refused("sync_every", REFUSALS["sync_every"], only=("queued", "finish"), sync_every=-1)
    refused("finish_below", FINISH_BELOW, only=("finish",), finish_below=-2)
    r.set_pixel_shard(0, 2)
    refused("pixel shard", REFUSALS["pixel shard"])
    # together: the first of the checks wins, in all three alike
    refused("all at once", REFUSALS["negative spp"], spp=-1, bounces=0, flags=4 | RENDER_COUNT_WORK, sync_every=-1)
    refused("no bounce first", REFUSALS["no bounce"], bounces=0, flags=4 | RENDER_COUNT_WORK, sync_every=-1)
    refused("sync_every before the flags", REFUSALS["sync_every"], only=("queued", "finish"), flags=4 | RENDER_COUNT_WORK,
            sync_every=-1)
    refused("unknown flag first", REFUSALS["unknown flag"], flags=4 | RENDER_COUNT_WORK)
    refused("count work before the shard", REFUSALS["count work"], flags=RENDER_COUNT_WORK)
    refused("finish_below before everything", FINISH_BELOW, only=("finish",), spp=-1, bounces=0, finish_below=-2)
    r.set_pixel_shard(0, 1)
    # no sample: the sums are cleared unless the call accumulates, nothing is traced
    pattern = (np.arange(8 * 16 * 3, dtype=F32).reshape(8, 16, 3) + F32(0.5))
    for flags in (0, RENDER_ACCUMULATE):
        for entry in ("plain", "queued", "finish"):
            r.write_linear(pattern)
            st.rays, st.iterations = 7, 7
            assert loop(entry, spp=0, flags=flags) == (0, "") and (st.rays, st.iterations) == (0, 0), (entry, flags)
            assert same(r.linear(), pattern if flags else np.zeros_like(pattern)), (entry, flags)


# ------------------------------------------------------------------------------------------ 4. on_bounce
def test_on_bounce_sees_every_ray(frames):
    seen = []

    def hook(rays, hits, pth):
        assert rays.shape == hits.shape == pth.shape and rays.is_cuda
        seen.append(rays.shape[0])

    r = wb.renderer(crt_amd.camera(4))
    rows = []
    res = paths.render(frames.scene("cornell_bunny"), r, 4, 20, on_bounce=hook, compact="device", profile=rows)
    assert sum(seen) == res["rays"] == frames.get("direct", "cornell_bunny", 4, 20)["rays"] and len(seen) == res["iterations"]
    _assert_frames_equal(dict(_frame(r, 4), rays=res["rays"]), frames.get("direct", "cornell_bunny", 4, 20), "with a hook")
    assert len(rows) == res["iterations"] and [row["n"] for row in rows] == seen
    assert all({"trace_ms", "advance_ms", "count_ms"} <= set(row) for row in rows)


def test_on_bounce_can_end_the_frame(frames):
    calls = []

    def hook(rays, hits, pth):
        calls.append(rays.shape[0])
        pth[:, paths.PATH_STATUS] = _lib.PATH_ENDED

    scene = frames.scene("cornell_bunny")
    r = wb.renderer(crt_amd.camera(4))
    before = None
    for regenerate in (True, False):
        r.init_rand(41)
        calls.clear()
        res = paths.render(scene, r, 4, 20, on_bounce=hook, compact="device", regenerate=regenerate)
        r.synchronize()
        if regenerate:
            assert res == {"rays": W * H, "iterations": 1} and calls == [W * H]
            before = r.rng_state()
        else:
            assert res == {"rays": 4 * W * H, "iterations": 4} and calls == [W * H] * 4
        assert not bits(r.linear()).any()                   # only zeros: no entry was stepped, so nothing was added
    fresh = wb.renderer(crt_amd.camera(4))
    crt_amd.camera_rays(fresh)
    fresh.synchronize()
    assert same(before, fresh.rng_state())                  # the camera rays' draws and no other


# ------------------------------------------------------------------------------------------ 5. side stream
def _fixed_rounds(scene, r, rng0, rounds, gated=False):
    """camera rays and `rounds` trace / advance rounds on the current stream, on the caller's own state tensors, without
    any synchronisation: every pixel has more samples left than rounds, so every round's count is the frame's pixels and
    the next batch is the whole output pair.  gated: the current stream is held back first (helpers/stream_gate.py), and
    the state tensors are made on it behind the gate."""
    import torch
    rng = torch.from_numpy(rng0.view(np.int32).copy()).to("cuda:0", non_blocking=False)
    if gated:
        torch.cuda.synchronize()
        stream_gate.gate(torch.cuda.current_stream())
        rng = rng.clone()
    lin = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda:0")
    rem = torch.full((W * H,), rounds + 1, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.default_stream())
    rays, pth = crt_amd.camera_rays(r, rng=rng)
    counts = []
    for _ in range(rounds):
        hits = scene.trace(rays, mode=2, grid_waves=8)["f32"]
        rays, pth, count = scene.path_advance(r, rays, hits, pth, 20, rem, rng=rng, linear=lin)
        counts.append(count)
    return rays, pth, rng, lin, rem, torch.cat(counts)


def test_side_stream(frames):
    import torch
    scene = frames.scene("bunny_w4")
    r = wb.renderer(crt_amd.camera(1))
    r.synchronize()
    rng0 = r.rng_state().reshape(-1, 6)
    base = _fixed_rounds(scene, r, rng0, 6)
    torch.cuda.synchronize()
    side = stream_gate.side_stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side and side != torch.cuda.default_stream()
        got = _fixed_rounds(scene, r, rng0, 6, gated=True)
    side.synchronize()
    assert base[5].tolist() == [W * H] * 6 and got[5].tolist() == [W * H] * 6
    key = lambda t: wb.keyed(t[0].cpu().numpy(), t[1].cpu().numpy(), W * H)   # noqa: E731
    assert np.array_equal(key(got), key(base))
    for a, b, k in zip(got[2:5], base[2:5], ("rng", "sums", "remaining")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert base[3].any() and (base[4] < 7).any()
    assert same(r.rng_state().reshape(-1, 6), rng0)        # the renderer's own state was not used


# ------------------------------------------------------------------------------------------ 6. checked build
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
for kind in ("device", "library"):
    r = crt_amd.Renderer(64, 36)
    r.set_camera(crt_amd.camera(2))
    r.init_rand(41)
    res = paths.render(sc, r, 2, 20, compact="device") if kind == "device" else r.render_wavefront(sc, 2, 20)
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
    fast = frames.get("device", "bunny_w4", 2, 20)
    for kind in ("device", "library"):
        _assert_frames_equal({k: got[f"{kind}_{k}"] for k in ("sum", "rgba", "rng")} | {"rays": int(got[f"{kind}_rays"])},
                             want, f"checked build, {kind}")
        assert int(got[f"{kind}_iterations"]) == fast["iterations"]
    _assert_frames_equal(fast, want, "fast build")
