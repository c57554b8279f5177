"""Path finish on the GPU: paths.finish / Scene.path_finish, the hand-off of
Renderer.render_wavefront(finish_below=K) and of paths.render(compact="device", finish_below=K).

Every comparison is bit for bit, on uint32 views; batches are the 2,304-entry 64x36 ones of helpers/wavefront_batches.

1. one finish == the loop of Scene.trace and paths.advance it replaces: RNG state, sums, remaining, rays; prefixes
   round the wave, a permuted batch, both traversals (trace<> on the reference tree, trace4 on the rebuilt 4-wide one).
2. entries that do nothing: ended, out of frame, at or beyond the count; an empty batch; a count made on the stream.
3. the first ray's tmax just below, at and just above its hit.
4. whole frames of Renderer.render_wavefront(finish_below=K) == Renderer.render, and the iterations the hand-off rule gives.
5. paths.render(compact="device", finish_below=K): the same frames, on_bounce for the wavefront rounds only.
6. the checked build in a fresh child process.
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
import finish_batches as fb  # noqa: E402
import wavefront_batches as wb  # noqa: E402
from wavefront_batches import H, W, bits, same  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
CHECKED = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
F32 = np.float32
UNSUPPORTED = -5                      # CRT_ERR_UNSUPPORTED
RENDER_COUNT_WORK = 2                 # CRT_RENDER_COUNT_WORK
N = W * H                             # 2,304
ENTRIES = (1, 63, 64, 65, 129, N)     # round the kernel's one-wave workgroup, more than one workgroup, the batch
PATTERNS = ("zero", "three", "alternating", "none")
KS = (0, 1, 100, N, 10 ** 9)
SYNC = (1, 3, 0)
QUEUE_SYNC_EVERY = 32                 # the library's block for sync_every = 0


# ------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def worlds(tmp_path_factory, scenes):
    out = custom_scene.synth_worlds(custom_scene.family_files(tmp_path_factory.mktemp("finish")))
    out["odd_materials"] = wb.odd_materials_world(scenes)
    return out


@pytest.fixture(scope="module")
def batches(worlds):
    return {"odd_materials": wb.traced_batch(worlds["odd_materials"], True), "s9_ground": wb.traced_batch(worlds["s9_ground"], False)}


@pytest.fixture(scope="module")
def bunny_w4(device_scenes):
    return device_scenes["cornell_bunny"][0].upload(0, bvh="rebuilt", width=4)


def _tree(b, bunny_w4, tree):
    """The batch's own scene (the reference tree: trace<> in the lane) or the rebuilt 4-wide bunny scene (trace4)."""
    return b.scene if tree == "reference" else bunny_w4


# ------------------------------------------------------------------------------------------ 1. against the loop
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("tree", ["reference", "w4"])
@pytest.mark.parametrize("world", ["odd_materials", "s9_ground"])
def test_finish_equals_the_loop(batches, bunny_w4, world, tree, pattern):
    b = batches[world]
    scene = _tree(b, bunny_w4, tree)
    rem = fb.remaining(pattern, b.n_pix)
    order = np.random.default_rng(7).permutation(N)
    for what, idx in [(f"first {n}", np.arange(n)) for n in ENTRIES] + [("permuted", order), ("permuted 129", order[:129])]:
        what = f"{world} / {tree} / {pattern} / {what}"
        want = fb.loop(b, scene, b.rays[idx], b.pth[idx], rem)
        got = fb.finish(b, scene, b.rays[idx], b.pth[idx], rem, totals=(5, 7))
        print(f"{what}: {want['rays']} rays in {want['rounds']} rounds")
        fb.assert_same_state(got, want, what)
        assert got["totals"] == [5 + want["rays"], 7 + 1], (what, got["totals"], want["rays"])
        assert want["rays"] >= len(idx) and (pattern != "three" or want["rays"] >= 4 * len(idx))
        pix = b.pth[idx, paths.PATH_PIXEL]
        fb.assert_others_untouched(b, got, rem, pix, what)
        assert rem is None or not got["remaining"][pix].any()
        assert len(idx) < N or not same(got["rng"][pix], b.rng[pix])
    # totals are optional (the renderer's own state and sums, rng=None and linear=None, are what the frames below use)
    idx = np.arange(129)
    s = fb.State(b, b.rays[idx], b.pth[idx], rem)
    scene.path_finish(b.r, s.rays, s.pth, fb.BOUNCES, s.rem, rng=s.rng, linear=s.lin)
    fb.assert_same_state(s.result(), fb.loop(b, scene, b.rays[idx], b.pth[idx], rem), "without totals")


# ------------------------------------------------------------------------------------------ 2. entries that do nothing
def _idle_batch(b):
    """The batch with every third entry handed in ENDED and four entries naming pixels outside the frame."""
    pth = b.pth.copy()
    pth[::3, paths.PATH_STATUS] = _lib.PATH_ENDED
    out = np.array([1, 64, 130, N - 1])
    assert not (out % 3 == 0).any()
    pth[out, paths.PATH_PIXEL] = [-1, b.n_pix, b.n_pix + 5, -(1 << 31)]
    return pth, out


@pytest.mark.parametrize("pattern", ["three", "none"])
@pytest.mark.parametrize("tree", ["reference", "w4"])
def test_ended_and_out_of_frame_entries_do_nothing(batches, bunny_w4, tree, pattern):
    b = batches["odd_materials"]
    scene = _tree(b, bunny_w4, tree)
    rem = fb.remaining(pattern, b.n_pix)
    pth, out = _idle_batch(b)
    act = fb.active(pth, b.n_pix)
    assert int((~act).sum()) == N // 3 + len(out)
    want = fb.loop(b, scene, b.rays, pth, rem)
    got = fb.finish(b, scene, b.rays, pth, rem)
    fb.assert_same_state(got, want, "idle entries")
    assert got["totals"] == [want["rays"], 1] and want["rays"] >= int(act.sum())
    fb.assert_others_untouched(b, got, rem, b.pth[act, paths.PATH_PIXEL], "pixels of idle entries")
    # nothing but idle entries: no ray, but the call had entries
    got = fb.finish(b, scene, b.rays[::3], pth[::3], rem, totals=(2, 3))
    assert got["totals"] == [2, 4]
    fb.assert_others_untouched(b, got, rem, [], "only ended entries")


@pytest.mark.parametrize("tree", ["reference", "w4"])
def test_counts(batches, bunny_w4, tree):
    b = batches["s9_ground"]
    scene = _tree(b, bunny_w4, tree)
    rem = fb.remaining("alternating", b.n_pix)
    cap = 1000                                               # a capacity that is no multiple of the wave
    rays, pth = b.rays[:cap], b.pth[:cap]
    for count in (0, 1, 65, cap, cap + 1, -1):               # -1: 0xffffffff
        n = min(count & 0xffffffff, cap)
        want = fb.loop(b, scene, rays[:n], pth[:n], rem)
        got = fb.finish(b, scene, rays, pth, rem, count=count, totals=(1, 1))
        fb.assert_same_state(got, want, f"count {count}")
        assert got["totals"] == [1 + want["rays"], 1 + (n > 0)], (count, got["totals"])
        fb.assert_others_untouched(b, got, rem, pth[:n, paths.PATH_PIXEL], f"entries from the count {count} on")
    # a count produced on a side stream just before the call
    want = fb.loop(b, scene, rays[:65], pth[:65], rem)
    got = fb.finish(b, scene, rays, pth, rem, count=65, stream_count=True)
    fb.assert_same_state(got, want, "count made on the stream")
    assert got["totals"] == [want["rays"], 1]
    # capacity 0: nothing launched, nothing changed, with and without a count
    for count in (None, 5):
        got = fb.finish(b, scene, rays[:0], pth[:0], rem, count=count, totals=(4, 4))
        assert got["totals"] == [4, 4]
        fb.assert_others_untouched(b, got, rem, [], "capacity 0")


# ------------------------------------------------------------------------------------------ 3. tmax
@pytest.mark.parametrize("tree", ["reference", "w4"])
def test_first_ray_keeps_its_tmax(batches, bunny_w4, tree):
    import torch
    b = batches["odd_materials"]
    scene = _tree(b, bunny_w4, tree)
    rem = fb.remaining("three", b.n_pix)
    t = scene.trace(fb.dev(b.rays))["t"].cpu().numpy()
    torch.cuda.synchronize()
    hit = t >= 0
    assert hit.sum() > 1000
    tt = np.where(hit, t, F32(np.inf)).astype(F32)
    res = {}
    for case, tmax in (("at", tt), ("below", np.nextafter(tt, F32(0))), ("above", np.nextafter(tt, F32(np.inf))),
                       ("zero", np.zeros_like(tt)), ("inf", np.full_like(tt, np.inf))):
        rays = b.rays.copy()
        rays[:, 3] = tmax
        want = fb.loop(b, scene, rays, b.pth, rem)
        got = fb.finish(b, scene, rays, b.pth, rem)
        fb.assert_same_state(got, want, f"tmax {case}")
        assert got["totals"] == [want["rays"], 1]
        res[case] = got
    # the filter did something: a ray cut short below its hit sees the sky instead, at or above its hit it does not
    assert same(res["at"]["lin"], res["inf"]["lin"]) and same(res["above"]["rng"], res["inf"]["rng"])
    assert not same(res["below"]["lin"], res["inf"]["lin"]) and same(res["zero"]["lin"], res["below"]["lin"])


# ------------------------------------------------------------------------------------------ 4. whole frames
def _frame(r, spp):
    r.resolve(crt_amd.pixel_sample_scale(max(spp, 1)))
    r.synchronize()
    return {"sum": r.linear(), "rgba": r.rgba8(), "rng": r.rng_state()}


def _assert_frames_equal(got, want, what):
    for k in ("sum", "rgba", "rng"):
        assert same(got[k], want[k]), f"{what}: {k} differs in {int((bits(got[k]) != bits(want[k])).sum())} words"
    assert got["rays"] == want["rays"], (what, got["rays"], want["rays"])


def _handoff(sizes, k, block):
    """The hand-off rule on the batch sizes of the wavefront's rounds: the host holds a size before round 0 and after
    every `block` rounds; the first one it holds that is <= k goes to the finish.  The rounds before it, or None."""
    for j in range(0, len(sizes), block):
        if sizes[j] <= k:
            return j
    return None


def _iterations(sizes, k, block):
    """The rounds, plus one for a finish that got an entry."""
    j = _handoff(sizes, k, block)
    return len(sizes) if j is None else j + 1


class Frames:
    def __init__(self, device_scenes, worlds, bunny_w4):
        self.scenes = {"bunny_w4": bunny_w4, **{k: v[1] for k, v in device_scenes.items()}}
        self.worlds = worlds

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = self.worlds[name].upload(0)
        return self.scenes[name]

    def check(self, name, spp, bounces, w=W, h=H):
        """Every K and sync_every of the new entry against Renderer.render's frame, the queued loop's numbers and the
        hand-off rule on the batch sizes paths.render's profile gives.  Returns the direct frame."""
        sc = self.scene(name)
        mk = lambda: wb.renderer(crt_amd.camera(max(spp, 1)), w, h)   # noqa: E731
        r = mk()
        r.render(sc, spp, bounces, count_work=True)
        direct = dict(_frame(r, spp), rays=r.counters()["rays"])
        rows = []
        paths.render(sc, mk(), spp, bounces, compact="device", profile=rows)
        sizes = [row["n"] for row in rows]
        assert sum(sizes) == direct["rays"] and (not sizes or sizes[0] == w * h)
        for sync in SYNC:
            queued = mk().render_wavefront(sc, spp, bounces, sync_every=sync)
            assert (queued["rays"], queued["iterations"]) == (direct["rays"], len(sizes))
            for k in KS:
                what = f"{name} {w}x{h} {spp} spp {bounces} bounces, finish_below={k}, sync_every={sync}"
                r = mk()
                res = r.render_wavefront(sc, spp, bounces, sync_every=sync, finish_below=k)
                _assert_frames_equal(dict(_frame(r, spp), rays=res["rays"]), direct, what)
                want = _iterations(sizes, k, sync or QUEUE_SYNC_EVERY)
                assert res["iterations"] == want, (what, res["iterations"], want)
                if k == 0:
                    assert res["iterations"] == queued["iterations"], what
                if k >= w * h and spp > 0:
                    assert res["iterations"] == 1, what
                assert spp == 0 or res["ms"] > 0
        print(f"\n{name} {w}x{h} {spp} spp {bounces} bounces: {direct['rays']} rays, {len(sizes)} rounds")
        return direct


@pytest.fixture(scope="module")
def frames(device_scenes, worlds, bunny_w4):
    return Frames(device_scenes, worlds, bunny_w4)


def test_config_a_golden_frame_on_the_reference_tree(frames):
    got = frames.check("cornell", 16, 20, w=256, h=256)
    want = json.loads((GOLDEN / "frames.json").read_text())["configA_256x256_16spp_20b"]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()   # noqa: E731
    assert got["rays"] == want["rays"]
    assert sha(got["sum"]) == want["sum_sha256"] and sha(got["rgba"]) == want["rgba_sha256"]


def test_bunny_golden_frame_on_the_reference_tree(frames):
    g = np.load(GOLDEN / "cornell_bunny_64x36_16spp.npz")
    got = frames.check("cornell_bunny", 16, 20)
    assert same(got["sum"], g["sum"]) and np.array_equal(got["rgba"], g["rgba"])


@pytest.mark.parametrize("spp", [0, 1, 4])
def test_rebuilt_tree(frames, spp):
    got = frames.check("bunny_w4", spp, 20)
    assert (got["rays"] == 0 and not got["sum"].any()) if spp == 0 else got["rays"] >= spp * N


@pytest.mark.parametrize("name", ["odd_materials", "s0"])
def test_synthetic_worlds(frames, name):
    frames.check(name, 4, 20)


def test_partial_last_wave(frames):
    frames.check("cornell_bunny", 4, 20, w=65, h=37)


@pytest.mark.parametrize("scene", ["cornell_bunny", "bunny_w4"])
@pytest.mark.parametrize("bounces", [1, 3])
def test_bounce_limits(frames, scene, bounces):
    got = frames.check(scene, 4, bounces)
    assert bounces != 1 or got["rays"] == 4 * N


def test_finish_entry_accumulates_refuses_and_shares_the_scratch(frames, bunny_w4):
    import torch
    scene = bunny_w4
    cam = crt_amd.camera(8)
    a, b = wb.renderer(cam), wb.renderer(cam)
    zero = np.zeros((H, W, 3), F32)
    a.write_linear(zero)
    b.write_linear(zero)
    rays = 0
    for _ in range(2):
        a.render(scene, 4, 20, accumulate=True, count_work=True)
        a.synchronize()
        rays += a.counters()["rays"]
    res = [b.render_wavefront(scene, 4, 20, accumulate=True, sync_every=2, finish_below=k) for k in (100, N)]
    got, want = _frame(b, 8), _frame(a, 8)
    _assert_frames_equal(dict(got, rays=res[0]["rays"] + res[1]["rays"]), dict(want, rays=rays), "two accumulating calls")
    assert got["sum"].any() and res[1]["iterations"] == 1 < res[0]["iterations"]
    # the two inherited refusals leave the sums and the RNG state as they are
    fn = _lib.hip().crt_renderer_render_wavefront_finish
    st = _lib.WavefrontStats()
    assert fn(b.h, scene.h, 4, 20, RENDER_COUNT_WORK, None, 4, 100, C.byref(st), None) == UNSUPPORTED
    b.set_pixel_shard(1, 2)
    assert fn(b.h, scene.h, 4, 20, 0, None, 4, 100, C.byref(st), None) == UNSUPPORTED
    with pytest.raises(crt_amd.CrtError, match="shard"):
        b.render_wavefront(scene, 4, 20, finish_below=100)
    b.set_pixel_shard(0, 1)
    with pytest.raises(crt_amd.CrtError, match="finish_below"):
        b.render_wavefront(scene, 4, 20, finish_below=-2)
    b.synchronize()
    assert same(b.linear(), got["sum"]) and same(b.rng_state(), got["rng"])
    # further frames on the same handle, the other loops of the shared scratch in between; -1 is the library's default
    r = wb.renderer(crt_amd.camera(4))
    r.render(scene, 4, 20, count_work=True)
    direct = dict(_frame(r, 4), rays=r.counters()["rays"])
    queued = r.render_wavefront(scene, 4, 20, sync_every=0)
    for kw in (dict(finish_below=100), dict(sync_every=4), dict(finish_below=N, sync_every=1), dict(), dict(finish_below=-1),
               dict(finish_below=1, sync_every=5)):
        b.init_rand(41)
        again = b.render_wavefront(scene, 4, 20, **kw)
        _assert_frames_equal(dict(_frame(b, 4), rays=again["rays"]), direct, f"a further frame with {kw}")
        assert again["ms"] > 0 and 1 <= again["iterations"] <= queued["iterations"]
    assert b.render_wavefront(scene, 0, 20, finish_below=100) == {"rays": 0, "iterations": 0, "ms": 0.0}
    assert not b.linear().any()
    # a side stream
    c = wb.renderer(crt_amd.camera(4))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    res = c.render_wavefront(scene, 4, 20, sync_every=3, finish_below=500, stream=side.cuda_stream)
    side.synchronize()
    _assert_frames_equal(dict(_frame(c, 4), rays=res["rays"]), direct, "the finish entry on a side stream")


def test_whole_frame_on_a_scene_that_was_never_traced(device_scenes):
    """Handed over before the first round, the frame runs no ray query at all: nothing of a query's may be assumed."""
    hs = device_scenes["cornell_bunny"][0]
    r = wb.renderer(crt_amd.camera(2))
    r.render(hs.upload(0, bvh="rebuilt", width=4), 2, 20, count_work=True)
    direct = dict(_frame(r, 2), rays=r.counters()["rays"])
    for k in (N, -1):
        fresh = hs.upload(0, bvh="rebuilt", width=4)
        r = wb.renderer(crt_amd.camera(2))
        res = r.render_wavefront(fresh, 2, 20, finish_below=k)
        _assert_frames_equal(dict(_frame(r, 2), rays=res["rays"]), direct, f"a fresh scene, finish_below={k}")
        assert res["iterations"] == 1


# ------------------------------------------------------------------------------------------ 5. the Python driver
@pytest.mark.parametrize("sync", [1, 4])
@pytest.mark.parametrize("name", ["cornell_bunny", "bunny_w4", "odd_materials"])
def test_python_driver_hands_off(frames, name, sync):
    sc = frames.scene(name)
    spp = 4
    mk = lambda: wb.renderer(crt_amd.camera(spp))   # noqa: E731
    r = mk()
    r.render(sc, spp, 20, count_work=True)
    direct = dict(_frame(r, spp), rays=r.counters()["rays"])
    rows = []
    paths.render(sc, mk(), spp, 20, compact="device", profile=rows)
    sizes = [row["n"] for row in rows]
    for k in KS:
        calls = []

        def hook(*args):
            calls.append(args[0].shape[0])

        r = mk()
        res = paths.render(sc, r, spp, 20, compact="device", sync_every=sync, finish_below=k, on_bounce=hook)
        what = f"{name}, finish_below={k}, sync_every={sync}"
        _assert_frames_equal(dict(_frame(r, spp), rays=res["rays"]), direct, what)
        want = _iterations(sizes, k, sync)
        assert res["iterations"] == want, (what, res["iterations"], want)
        # the hook sees the wavefront rounds and nothing of the finish: the rounds enqueued before the hand-off (whole
        # blocks; with no hand-off the last block may run past the end)
        j = _handoff(sizes, k, sync)
        if j is not None:
            assert len(calls) == j, (what, len(calls))
        else:
            assert len(sizes) <= len(calls) < len(sizes) + sync, (what, len(calls))
        assert not calls or calls[0] == N
    # sample by sample (regenerate=False): each sample's batch is finished with remaining=None
    r = mk()
    res = paths.render(sc, r, spp, 20, compact="device", sync_every=sync, finish_below=100, regenerate=False)
    _assert_frames_equal(dict(_frame(r, spp), rays=res["rays"]), direct, f"{name}, sample by sample")


# ------------------------------------------------------------------------------------------ 6. the checked build
CHILD = r"""
import sys
from pathlib import Path
import numpy as np
repo = Path(sys.argv[1])
sys.path[:0] = [str(repo / "raytracer-cuda_amd"), str(repo / "oracle")]
import crt_amd
from crt_amd import _lib, assets
hs = crt_amd.HostScene(assets.scene_files("cornell_bunny"))
sc = hs.upload(0, bvh="rebuilt", width=4)
r = crt_amd.Renderer(64, 36)
r.set_camera(crt_amd.camera(2))
r.init_rand(41)
res = r.render_wavefront(sc, 2, 20, sync_every=4, finish_below=100)
r.resolve(crt_amd.pixel_sample_scale(2))
r.synchronize()                                          # a device error of the checked build raises here
np.savez(sys.argv[2], flags=np.array(_lib.hip().crt_build_flags()), sum=r.linear(), rgba=r.rgba8(), rng=r.rng_state(),
         rays=np.array(res["rays"]), iterations=np.array(res["iterations"]))
"""


def test_checked_build_gives_the_same_bits(bunny_w4, tmp_path):
    assert CHECKED.exists() and _lib.hip().crt_build_flags() == 0
    out = tmp_path / "checked.npz"
    p = subprocess.run([sys.executable, "-c", CHILD, str(REPO), str(out)], env=dict(os.environ, CRT_HIP_LIB=str(CHECKED)),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(out)
    assert int(got["flags"]) == _lib.BUILD_CHECKED
    r = wb.renderer(crt_amd.camera(2))
    r.render(bunny_w4, 2, 20, count_work=True)
    want = dict(_frame(r, 2), rays=r.counters()["rays"])
    here = wb.renderer(crt_amd.camera(2)).render_wavefront(bunny_w4, 2, 20, sync_every=4, finish_below=100)
    _assert_frames_equal({k: got[k] for k in ("sum", "rgba", "rng")} | {"rays": int(got["rays"])}, want, "checked build")
    assert int(got["iterations"]) == here["iterations"] > 1
