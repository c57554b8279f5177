"""Stream ordering of the frame pipeline's entries (crt_hip.h and INTEGRATION.md "Streams", DESIGN.md "Streams").

Every launching entry takes a stream and promises to be ordered with the caller's other work on it.  A test that only
puts work on a side stream and synchronises cannot see a launch that went to stream 0 by mistake: nothing else is in
flight.  Here a stream is held back by a gate (helpers/stream_gate.py: a spin kernel of some tens of milliseconds) while
the calls under test are enqueued:

1. the controls: the rig discriminates on this machine (a gated stream holds its own work back and nobody else's).
2. side-gated chains: a handle that holds a stale frame in every buffer enqueues a whole chain behind a gate on a side
   stream; a launch on another stream, or one that read its inputs when it was enqueued, gives the stale values.  The
   calls that DESIGN.md lists as enqueue-only must return while the gate is still closed.
3. null-gated first use: the default stream is held back while the first call of every state-allocating path runs on a
   side stream; an initialisation left on the null stream would land after the kernels that follow it.
4. two handles over one scene on two gated streams.

Expected values: the same calls on the null stream from a fresh handle, compared as raw bits (the filtered buffers
through denoise_model.canon, as the filter tests compare them).  The entries are called through ctypes with a NULL
stats pointer: the Python front-ends always pass one, and an entry with a stats pointer waits.
"""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import denoise_model as dm  # noqa: E402
import stream_gate as sg  # noqa: E402
from wavefront_batches import same  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
SIZES = [(64, 36), (37, 19)]                     # 37x19: a partial wave and partial tiles
BOUNCES = 20
SEED, STALE_SEED = 41, 977
YAW, STALE_YAW = -90.0, -60.0
SWEEP = (-47.0, -46.0, -45.0)                    # the open front of the box is in view: misses beside hits
TOL, CAP = 0.05, 32.0                            # the reprojection's options, as test_gpu_reproject.py
SIGMAS, MINH = (4.0, INF, 0.05), 4.0             # the filters' options, as test_gpu_denoise.py and test_gpu_variance.py
ADAPT_MIN, ADAPT_MAX = 4, 16
ACCUMULATE = crt_amd.RENDER_ACCUMULATE
CANON = ("denoised", "history", "moments", "variance", "tile_error")      # may hold NaNs


# ------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def scene_of(device_scenes):
    """The rebuilt 4-wide bunny scene and the reference-tree Cornell box."""
    return {"bunny_w4": device_scenes["cornell_bunny"][0].upload(0, bvh="rebuilt", width=4),
            "cornell": device_scenes["cornell"][1]}


@pytest.fixture(scope="module")
def rig():
    """Side streams on which the two controls hold (helpers/stream_gate.pick_side_streams), found once.  Every ordering
    test below takes its streams from _sides(rig), which fails and names the control where none was found."""
    print(f"\ngate: {sg.describe()}; measured {sg.measure():.1f} ms on an idle stream")
    streams, problems = sg.picked()
    return {"streams": streams, "problems": problems}


def _sides(rig, n=1):
    """n side streams that run beside the default stream: the precondition of every ordering test."""
    for control, problems in rig["problems"].items():
        assert not problems, f"precondition: the control '{control}' holds on no side stream of this machine: {problems}"
    assert len(rig["streams"]) >= n
    return rig["streams"][:n]


def _side(rig):
    return _sides(rig)[0]


# ------------------------------------------------------------------------------------------ 1. the controls
def test_control_side_gate(rig):
    """x = 0; gate on side; x.fill_(1) on side; y = x on the default stream: y is all 0 and x all 1."""
    res = sg.control_side_gate(_side(rig))
    assert res["gate open at enqueue"]
    assert bool((res["early copy"] == 0).all()) and bool((res["late value"] == 1).all())


def test_control_null_gate(rig):
    """The same with the roles exchanged; torch's default stream is stream 0 and its side stream is not."""
    res = sg.control_null_gate(_side(rig))
    assert res["default handle"] == 0 and res["side handle"] != 0
    assert res["gate open at enqueue"]
    assert bool((res["early copy"] == 0).all()) and bool((res["late value"] == 1).all())


def test_gate_length():
    ms = sg.measure()
    print(f"\ngate: {sg.describe()}; measured {ms:.1f} ms")
    assert 0.5 * sg.GATE_MS <= ms <= 4 * sg.GATE_MS          # bounded, and some tens of milliseconds


# ------------------------------------------------------------------------------------------ the calls
class Calls:
    """The entries under test on one handle and one stream, through ctypes with NULL stats pointers.

    gate_on: the torch stream that is held back (None: nothing is).  After a call that DESIGN.md lists as enqueue-only
    (enqueue_only=True) the gate must still be closed, where check_open asks for it.  Any other call may have waited for
    the stream; when it has outlasted the gate, a new gate holds back what follows.  An error return raises: nothing is
    enqueued after it."""

    def __init__(self, r, sc, stream=None, gate_on=None, check_open=False):
        self.r, self.sc, self.stream, self.gate_on, self.check_open = r, sc, stream, gate_on, check_open
        self.ev = sg.gate(gate_on) if gate_on is not None else None
        self.t0, self.gates, self.asserted = time.perf_counter(), 1, []

    def _call(self, name, enqueue_only, *args):
        rc = _lib.require("crt_renderer_" + name)(self.r.h, *args, self.stream)
        _lib.check(rc, name)
        if self.ev is None:
            return
        if enqueue_only and self.check_open:
            assert not self.ev.query(), (f"{name} is documented as enqueue-only, but the gate had ended when it returned "
                                         f"({1e3 * (time.perf_counter() - self.t0):.1f} ms after the gate was set)")
            self.asserted.append(name)
        elif self.ev.query():
            self.ev = sg.gate(self.gate_on)
            self.t0, self.gates = time.perf_counter(), self.gates + 1

    # enqueue_only: whether this call, here, is one that only enqueues (DESIGN.md "Streams")
    def init_rand(self, seed, enqueue_only=False):
        self._call("init_rand", enqueue_only, int(seed), 0)

    def render(self, spp, flags=0, enqueue_only=False):
        self._call("render", enqueue_only, self.sc.h, int(spp), BOUNCES, flags)

    def resolve(self, spp):
        self._call("resolve", True, C.c_float(crt_amd.pixel_sample_scale(spp)))

    def render_adaptive(self, tolerance):
        o = _lib.AdaptiveOptions(ADAPT_MIN, ADAPT_MAX, float(tolerance), 0)
        self._call("render_adaptive", False, self.sc.h, C.byref(o), BOUNCES, 0, None)

    def resolve_adaptive(self):
        self._call("resolve_adaptive", True)

    def compute_guides(self, enqueue_only=False):
        self._call("compute_guides", enqueue_only, self.sc.h, None)

    def denoise(self, spp, direct_only=False, enqueue_only=False):
        o = _lib.DenoiseOptions(5, *SIGMAS, _lib.DENOISE_DIRECT_ONLY if direct_only else 0, 0)
        self._call("denoise", enqueue_only, C.byref(o), C.c_float(crt_amd.pixel_sample_scale(spp)), None)

    def resolve_denoised(self):
        self._call("resolve_denoised", True)

    def reproject(self, moments=False, enqueue_only=False):
        o = _lib.ReprojectOptions(TOL, -INF, CAP, 0, 0)
        self._call("reproject_moments" if moments else "reproject", enqueue_only, C.byref(o), C.c_float(1.0), None)

    def denoise_history(self, enqueue_only=False):
        o = _lib.DenoiseOptions(5, *SIGMAS, 0, 0)
        self._call("denoise_history", enqueue_only, C.byref(o), None)

    def denoise_history_variance(self, enqueue_only=False):
        o = _lib.DenoiseVarianceOptions(5, *SIGMAS, MINH, 0, 0)
        self._call("denoise_history_variance", enqueue_only, C.byref(o), None)

    def resolve_history(self):
        self._call("resolve_history", True)


def _begin(c, yaw=YAW, variant=-1, probe=False, temporal=False):
    """The host-only settings a chain starts from, the same on a fresh and on a used handle."""
    r = c.r
    r.set_kernel_variant(variant)
    r.set_schedule(probe_spp=2, min_spp=0) if probe else r.set_schedule()
    r.set_temporal_order(temporal)
    r.set_camera(crt_amd.camera(1, yaw=yaw))
    r.reset_history()


def _read(r, extras=()):
    r.synchronize()                                   # the error word: a render that reported one raises here
    out = {"sum": r.linear(), "rgba": r.rgba8(), "rng": r.rng_state()}
    for k in extras:
        out[k] = getattr(r, k)()
    return out


def _equal(k, a, b):
    return np.array_equal(dm.canon(a), dm.canon(b)) if k in CANON else (
        same(a, b) if a.dtype.itemsize == 4 else np.array_equal(a, b))


def _assert_equal(got, want, what):
    for k in want:
        if not _equal(k, got[k], want[k]):
            diff = (dm.canon(got[k]) != dm.canon(want[k])) if got[k].dtype == np.float32 else (got[k] != want[k])
            raise AssertionError(f"{what}: {k} differs from the null-stream frame in {int(diff.sum())} of {diff.size} "
                                 f"words, first at {np.argwhere(diff)[:4].tolist()}")


def _stale_handle(sc, w, h):
    """A handle that has completed another frame on the null stream: another seed, another camera, its own adaptive
    state, guides, history, moments, variance and denoised frame.  Every entry has run once, so every first-use
    allocation is done.  (Every chain begins with reset_history, a host flag: its first reprojection starts over, as a
    fresh handle's does.)"""
    r = crt_amd.Renderer(w, h)
    c = Calls(r, sc)
    _begin(c, yaw=STALE_YAW)
    c.init_rand(STALE_SEED)
    c.render_adaptive(-1.0)                           # every tile refined to the maximum
    c.resolve_adaptive()
    c.render(2)
    c.render(1, ACCUMULATE)
    c.compute_guides()
    c.denoise(3)
    c.reproject(moments=True)
    c.denoise_history_variance()
    c.resolve_denoised()
    r.synchronize()
    return r


EXTRAS_ALL = ("tile_spp", "tile_error", "guides", "denoised", "history", "moments", "variance")


def _reference(sc, w, h, chain, extras):
    """The chain on the null stream from a fresh handle."""
    r = crt_amd.Renderer(w, h)
    chain(Calls(r, sc))
    return _read(r, extras)


def _run_side_gated(rig, sc, w, h, chain, extras=(), what=""):
    import torch
    side = _side(rig)
    want = _reference(sc, w, h, chain, extras)
    r = _stale_handle(sc, w, h)
    stale = _read(r, extras)
    for k in want:                                    # plausible but wrong: no buffer already holds the answer
        assert not _equal(k, stale[k], want[k]), f"{what}: the stale {k} already equals the expected one"
    torch.cuda.synchronize()
    c = Calls(r, sc, side.cuda_stream, gate_on=side, check_open=True)
    chain(c)
    enqueued_ms = 1e3 * (time.perf_counter() - c.t0)
    side.synchronize()
    print(f"\n{what} {w}x{h}: {c.gates} gate(s), {enqueued_ms:.2f} ms of enqueueing after the last; still closed "
          f"after {len(c.asserted)} calls: {' '.join(sorted(set(c.asserted)))}")
    _assert_equal(_read(r, extras), want, what)
    c.want = want
    return c


# ------------------------------------------------------------------------------------------ 2a. init_rand, render, resolve
def _chain_probe(c):
    """The automatic choice with the probe: variant 8, whose occupancy decision reads the probe's statistics."""
    _begin(c, probe=True)
    c.init_rand(SEED, enqueue_only=True)
    c.render(4)                                       # waits: the probe's occupancy decision
    c.resolve(4)


def _chain_v7(c):
    """The interactive path: variant 7 at 1 spp, no probe."""
    _begin(c, variant=7)
    c.init_rand(SEED, enqueue_only=True)
    c.render(1, enqueue_only=True)
    c.resolve(1)


def _chain_v7_temporal(c):
    """Variant 7 over two frames with the temporal order: the second frame's launch is ordered by the first's rays."""
    _begin(c, variant=7, temporal=True)
    c.init_rand(SEED, enqueue_only=True)
    c.render(1)                                       # first use of the temporal order allocates
    c.render(1, ACCUMULATE, enqueue_only=True)
    c.resolve(2)


def _chain_v4(c):
    _begin(c, variant=4)
    c.init_rand(SEED, enqueue_only=True)
    c.render(3, enqueue_only=True)
    c.resolve(3)


def _chain_v10(c):
    _begin(c, variant=10, probe=True)
    c.init_rand(SEED, enqueue_only=True)
    c.render(2)                                       # first use of the tile variants allocates the tile keys
    c.render(2, ACCUMULATE, enqueue_only=True)
    c.resolve(4)


def _chain_v3(c):
    _begin(c, variant=3)
    c.init_rand(SEED, enqueue_only=True)
    c.render(2, enqueue_only=True)
    c.resolve(2)


def _chain_accumulate(c):
    _begin(c)
    c.init_rand(SEED, enqueue_only=True)
    c.render(2, enqueue_only=True)
    c.render(2, ACCUMULATE, enqueue_only=True)
    c.resolve(4)


def _chain_rand_cache(c):
    """The same seed twice: the second init_rand copies the cached state back."""
    _begin(c)
    c.init_rand(SEED, enqueue_only=True)
    c.render(1, enqueue_only=True)
    c.init_rand(SEED, enqueue_only=True)
    c.render(1, ACCUMULATE, enqueue_only=True)
    c.resolve(2)


RENDER_CHAINS = {"probe v8": ("bunny_w4", _chain_probe), "v7": ("bunny_w4", _chain_v7),
                 "v7 temporal": ("bunny_w4", _chain_v7_temporal), "v4": ("bunny_w4", _chain_v4),
                 "v10": ("cornell", _chain_v10), "v3": ("cornell", _chain_v3),
                 "accumulate w4": ("bunny_w4", _chain_accumulate), "accumulate reference": ("cornell", _chain_accumulate),
                 "rand cache": ("bunny_w4", _chain_rand_cache)}


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", list(RENDER_CHAINS))
def test_render_chain_behind_a_side_gate(rig, scene_of, name, w, h):
    scene, chain = RENDER_CHAINS[name]
    c = _run_side_gated(rig, scene_of[scene], w, h, chain, what=name)
    assert "resolve" in c.asserted and "init_rand" in c.asserted


def test_the_variants_ran_the_kernels_they_name(scene_of):
    """The chains above pick their kernels through the public settings: what they pick, on the null stream."""
    for name, kernel in (("probe v8", "crt_render_kernel<false, 8,"), ("v7", "crt_render_kernel<false, 7,"),
                         ("v4", "crt_render_kernel<false, 4,"), ("v10", "crt_render_kernel<false, 10,"),
                         ("v3", "crt_render_kernel<false, 3,"), ("accumulate w4", "crt_render_kernel<false, 7,"),
                         ("accumulate reference", "crt_render_kernel<false, 3,")):
        scene, chain = RENDER_CHAINS[name]
        r = crt_amd.Renderer(64, 36)
        chain(Calls(r, scene_of[scene]))
        r.synchronize()
        assert r.last_kernel_name().startswith(kernel), (name, r.last_kernel_name())


# ------------------------------------------------------------------------------------------ 2b. adaptive
@pytest.fixture(scope="module")
def median_tolerance(scene_of):
    """Per scene and size, the median of the non-zero tile errors of the spp_min frame (as test_gpu_adaptive.py)."""
    out = {}
    for name, sc in scene_of.items():
        for w, h in SIZES:
            r = crt_amd.Renderer(w, h)
            c = Calls(r, sc)
            _begin(c)
            c.init_rand(SEED)
            c.render_adaptive(INF)
            e = r.tile_error().reshape(-1)
            out[name, w, h] = float(np.median(e[e > 0]))
    return out


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_adaptive_chain_behind_a_side_gate(rig, scene_of, median_tolerance, name, w, h):
    tol = median_tolerance[name, w, h]

    def chain(c):
        _begin(c)
        c.init_rand(SEED, enqueue_only=True)
        c.render_adaptive(tol)                        # waits: the pass count is read on the host
        c.resolve_adaptive()

    c = _run_side_gated(rig, scene_of[name], w, h, chain, ("tile_spp", "tile_error"), f"adaptive {name}")
    assert "resolve_adaptive" in c.asserted
    spp = c.want["tile_spp"].reshape(-1)
    assert spp.min() == ADAPT_MIN and spp.max() > ADAPT_MIN          # both outcomes occur: a condition on the input


# ------------------------------------------------------------------------------------------ 2c. guides, filter
@pytest.mark.parametrize("direct_only", [False, True], ids=["tiled", "direct"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_denoise_chain_behind_a_side_gate(rig, scene_of, name, w, h, direct_only):
    def chain(c):
        _begin(c)
        c.init_rand(SEED, enqueue_only=True)
        c.render(4, enqueue_only=True)
        c.compute_guides(enqueue_only=True)
        c.denoise(4, direct_only, enqueue_only=True)
        c.resolve_denoised()

    c = _run_side_gated(rig, scene_of[name], w, h, chain, ("guides", "denoised"), f"denoise {name}")
    assert c.gates == 1 and c.asserted == ["init_rand", "render", "compute_guides", "denoise", "resolve_denoised"]


# ------------------------------------------------------------------------------------------ 2d. a camera sweep
def _sweep(kind):
    def chain(c):
        _begin(c)
        for k, yaw in enumerate(SWEEP):
            c.r.set_camera(crt_amd.camera(1, yaw=yaw))
            c.init_rand(SEED + k, enqueue_only=True)
            c.render(1, enqueue_only=True)
            c.compute_guides(enqueue_only=True)
            c.reproject(moments=kind == "variance", enqueue_only=True)
            if kind == "history":
                c.resolve_history()
            else:
                c.denoise_history_variance(enqueue_only=True) if kind == "variance" else c.denoise_history(enqueue_only=True)
                c.resolve_denoised()
    return chain


SWEEP_EXTRAS = {"denoise": ("guides", "history", "denoised"), "history": ("guides", "history"),
                "variance": ("guides", "history", "moments", "variance", "denoised")}


@pytest.mark.parametrize("kind", list(SWEEP_EXTRAS))
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_camera_sweep_behind_a_side_gate(rig, scene_of, name, w, h, kind):
    c = _run_side_gated(rig, scene_of[name], w, h, _sweep(kind), SWEEP_EXTRAS[kind], f"sweep {kind} {name}")
    assert c.gates == 1 and len(c.asserted) == len(SWEEP) * (5 if kind == "history" else 6)


def test_the_sweep_reprojects(scene_of):
    """A condition on the input of the sweeps: their later frames take most pixels from the history."""
    r = crt_amd.Renderer(64, 36)
    _sweep("variance")(Calls(r, scene_of["bunny_w4"]))
    length = r.history()[..., 3]
    assert (length > len(SWEEP) - 1).any() and (length == 1).any()


# ------------------------------------------------------------------------------------------ 2e. a torch consumer
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_torch_consumer_on_the_same_stream(rig, scene_of, name, w, h):
    """attach_linear to a torch tensor, render on the side stream, clone on the side stream, no host wait in between."""
    import torch
    side = _side(rig)
    sc = scene_of[name]

    def chain(c):
        _begin(c)
        c.init_rand(SEED, enqueue_only=True)
        c.render(2, enqueue_only=True)

    want = _reference(sc, w, h, chain, ())["sum"]
    r = _stale_handle(sc, w, h)
    t = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    r.attach_linear(t.data_ptr())
    try:
        c = Calls(r, sc)
        c.render(1)                                   # a stale frame in the tensor, on the null stream
        r.synchronize()
        assert t.any() and not same(t.cpu().numpy(), want)
        torch.cuda.synchronize()
        c = Calls(r, sc, side.cuda_stream, gate_on=side, check_open=True)
        chain(c)
        with torch.cuda.stream(side):
            clone = t.clone()
        assert not c.ev.query(), "the clone was enqueued after the gate had ended"
        side.synchronize()
        assert same(clone.cpu().numpy(), want), "the clone on the same stream is not the null-stream frame"
        assert same(t.cpu().numpy(), want)
    finally:
        r.attach_linear(None)


# ------------------------------------------------------------------------------------------ 3. null-gated first use
def _first_uses(c):
    """The first call of every state-allocating path, in this order."""
    _begin(c)
    c.init_rand(SEED)
    c.render(2)                                       # order buffers, the overflow stack where the scene needs it
    c.render_adaptive(1e-3)
    c.resolve_adaptive()
    c.compute_guides()
    c.denoise(ADAPT_MIN)
    c.reproject()
    c.reproject(moments=True)
    c.denoise_history_variance()
    c.resolve_denoised()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_first_use_on_a_side_stream_while_the_null_stream_is_held_back(rig, scene_of, name, w, h):
    import torch
    side = _side(rig)
    sc = scene_of[name]
    want = _reference(sc, w, h, _first_uses, EXTRAS_ALL)
    r = crt_amd.Renderer(w, h)                        # the handle and the scene exist before the gate
    torch.cuda.synchronize()
    c = Calls(r, sc, side.cuda_stream, gate_on=torch.cuda.default_stream())
    _first_uses(c)
    held = not c.ev.query()
    side.synchronize()
    torch.cuda.synchronize()
    print(f"\nfirst use {name} {w}x{h}: {c.gates} gate(s) on the null stream, the last still closed at the end: {held}")
    _assert_equal(_read(r, EXTRAS_ALL), want, f"first use {name}")


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_a_handle_created_while_the_null_stream_is_held_back(rig, scene_of, name, w, h):
    import torch
    side = _side(rig)
    sc = scene_of[name]

    def chain(c):
        _begin(c)
        c.init_rand(SEED)
        c.render(2)
        c.resolve(2)

    want = _reference(sc, w, h, chain, ())
    torch.cuda.synchronize()
    ev = sg.gate(torch.cuda.default_stream())
    r = crt_amd.Renderer(w, h)                        # returns after its own initialisation has completed
    chain(Calls(r, sc, side.cuda_stream))             # and is used on another stream at once
    side.synchronize()
    torch.cuda.synchronize()
    assert ev.query()
    _assert_equal(_read(r), want, f"create {name}")


# ------------------------------------------------------------------------------------------ 4. two handles, two streams
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_two_handles_on_two_gated_streams(rig, scene_of, name, w, h):
    """Two renderers with different seeds render one scene at the same time (a render uses none of the scene's own
    scratch: that is the trace queries', which one scene serves one at a time)."""
    import torch
    sides = _sides(rig, 2)
    sc = scene_of[name]

    def chain_of(seed):
        def chain(c):
            _begin(c)
            c.init_rand(seed, enqueue_only=True)
            c.render(3, enqueue_only=True)
            c.resolve(3)
        return chain

    chains = [chain_of(SEED), chain_of(SEED + 1)]
    want = [_reference(sc, w, h, ch, ()) for ch in chains]
    assert not same(want[0]["sum"], want[1]["sum"])
    handles = [_stale_handle(sc, w, h) for _ in chains]
    torch.cuda.synchronize()
    calls = [Calls(r, sc, s.cuda_stream, gate_on=s, check_open=True) for r, s in zip(handles, sides)]   # both gated
    for c, ch in zip(calls, chains):
        ch(c)
    assert not calls[0].ev.query() and not calls[1].ev.query()       # released together: both chains are enqueued
    for s in sides:
        s.synchronize()
    for k, r in enumerate(handles):
        _assert_equal(_read(r), want[k], f"two handles {name}, handle {k}")
