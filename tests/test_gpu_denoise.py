"""The denoiser on the GPU: Renderer.compute_guides, denoise, resolve_denoised and the filter self-test.

Every comparison is bit for bit, on uint32 views (NaNs, whose sign and payload IEEE 754 leaves open, mapped to one
pattern first: helpers/denoise_model.canon).

1. the filter on crafted buffers against the numpy model, through the tiled and the direct kernel.
2. the guides against Scene.trace of the numpy pixel-centre rays.
3. whole pipelines: render / render_adaptive, compute_guides, denoise, resolve_denoised.
4. the refusals that need a real handle.
5. the checked build in a fresh child process.
6. crt_render -denoise.
"""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import adaptive_model as am  # noqa: E402
import denoise_model as dm  # noqa: E402
from wavefront_batches import bits, same  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
CHECKED = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
CLI = REPO / "raytracer-cuda_amd" / "bin" / "crt_render"
F32 = np.float32
INF = float("inf")
INVALID, UNSUPPORTED = -1, -5
W, H = 64, 36
SIGMAS = (4.0, INF, 0.05)


# ------------------------------------------------------------------------------------------ 1. the filter, crafted
# one pixel; one partial workgroup; 8x8; odd sizes; 64x36; narrower than every halo; more than one workgroup in x and
# several row groups; several workgroups both ways with ragged edges and a stride of 16 that crosses tiles
FRAMES = [(1, 1), (7, 5), (8, 8), (37, 19), (64, 36), (3, 70), (136, 136), (264, 260)]
SIGMA_SETS = {"all": (4.0, 0.7, 0.5), "color": (4.0, INF, INF), "normal": (INF, 0.7, INF), "position": (INF, INF, 0.5),
              "off": (INF, INF, INF)}
STEPS = (1, 5, 8)


def _crafted(w, h, seed):
    """Seeded random colours in (-1, 4), a few of them infinite or NaN; unit normals; positions in the unit cube; key
    regions in blocks of 5 x 3 pixels over 4 keys (one of them negative); a twentieth of the pixels are misses."""
    g = np.random.default_rng(seed)
    c = (g.random((h, w, 3)) * 5 - 1).astype(F32)
    special = g.random((h, w)) < 0.02
    c[special, g.integers(0, 3, int(special.sum()))] = g.choice(np.array([np.inf, -np.inf, np.nan], F32), int(special.sum()))
    n = g.normal(size=(h, w, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F32)
    pos = g.random((h, w, 3)).astype(F32)
    blocks = g.integers(0, 4, ((h + 2) // 3, (w + 4) // 5)).astype(np.int32)
    key = np.repeat(np.repeat(blocks, 3, axis=0), 5, axis=1)[:h, :w] - 1
    t = (g.random((h, w)) * 3 + 0.1).astype(F32)
    guides = dm.pack_guides(n, t, pos, np.ascontiguousarray(key))
    guides[g.random((h, w)) < 0.05] = dm.miss_record()
    return c, guides


@pytest.mark.parametrize("sigmas", list(SIGMA_SETS))
@pytest.mark.parametrize("w,h", FRAMES)
def test_filter_on_crafted_buffers_equals_the_model(w, h, sigmas):
    sig = SIGMA_SETS[sigmas]
    r = crt_amd.Renderer(w, h)
    c, guides = _crafted(w, h, 1000 + 31 * w + h)
    want = dm.denoise_steps(c, guides, *sig, STEPS)
    for it in STEPS:
        tiled = r.selftest_denoise(c, guides, *sig, iterations=it)
        direct = r.selftest_denoise(c, guides, *sig, iterations=it, direct_only=True)
        assert np.array_equal(bits(tiled), bits(direct)), (w, h, sigmas, it, "the two kernels differ")
        diff = dm.canon(tiled) != dm.canon(want[it])
        assert not diff.any(), (w, h, sigmas, it, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert same(r.guides(), guides) and np.array_equal(dm.canon(r.linear()), dm.canon(c))
    if sig[0] != INF:       # with the colour term on a NaN or infinite neighbour has X = NaN or inf: it never spread
        bad_in = ~np.isfinite(c).all(axis=-1)
        bad_out = ~np.isfinite(want[8]).all(axis=-1)
        assert (bad_in.any() or w * h < 500) and not (bad_out & ~bad_in).any()


def test_a_second_call_on_the_first_calls_output():
    w, h = 37, 19
    r = crt_amd.Renderer(w, h)
    c, guides = _crafted(w, h, 77)
    sig = SIGMA_SETS["all"]
    first = r.selftest_denoise(c, guides, *sig, iterations=2)
    second = r.selftest_denoise(first, guides, *sig, iterations=3)
    want = dm.denoise(dm.denoise(c, guides, *sig, 2), guides, *sig, 3)
    assert np.array_equal(dm.canon(second), dm.canon(want))
    assert same(r.denoised(), second)


# ------------------------------------------------------------------------------------------ 2. the guides
@pytest.fixture(scope="module")
def bunny_w4(device_scenes):
    return device_scenes["cornell_bunny"][0].upload(0, bvh="rebuilt", width=4)


@pytest.fixture(scope="module")
def scene_of(device_scenes, bunny_w4):
    """The rebuilt 4-wide bunny scene and the reference-tree Cornell box."""
    return {"bunny_w4": bunny_w4, "cornell": device_scenes["cornell"][1]}


def _renderer(w=W, h=H, seed=41, cam=None):
    r = crt_amd.Renderer(w, h)
    r.set_camera(cam if cam is not None else crt_amd.camera(1))
    r.init_rand(seed)
    return r


def _state(r):
    r.synchronize()
    return {"sum": r.linear(), "rgba": r.rgba8(), "rng": r.rng_state()}


@pytest.mark.parametrize("yaw", [-90.0, -40.0])                 # the second camera sees past the box: misses
@pytest.mark.parametrize("w,h", [(64, 36), (37, 19)])
@pytest.mark.parametrize("name", ["bunny_w4", "cornell"])
def test_guides_equal_the_ray_query_of_the_centre_rays(scene_of, name, w, h, yaw):
    sc = scene_of[name]
    cam = crt_amd.camera(1, yaw=yaw)
    r = _renderer(w, h, cam=cam)
    r.render(sc, 2, 20)
    before = _state(r)
    r.compute_guides(sc)
    g = r.guides()
    after = _state(r)
    for k in before:
        assert same(before[k], after[k]), k                      # no RNG state consumed, no sum touched
    o, d = dm.centre_rays(crt_amd.camera_floats(cam), w, h)
    hits = sc.trace(o, d)
    hit = hits["t"] >= 0
    assert hit.any() and (yaw == -90.0 or (~hit).any())
    g2, gi = g.reshape(-1, 8), g.view(np.int32).reshape(-1, 8)
    assert same(g2[hit, 3], hits["t"][hit]) and same(g2[hit, 0:3], hits["normal"][hit])
    assert np.array_equal(gi[hit, 7], hits["object"][hit])
    pos = (o + (hits["t"][:, None] * d).astype(F32)).astype(F32)
    assert same(g2[hit, 4:7], pos[hit])
    assert (bits(g2[~hit]) == bits(dm.miss_record())).all()
    assert (hits["t"][~hit] == -1).all()


# ------------------------------------------------------------------------------------------ 3. whole pipelines
@pytest.fixture(scope="module")
def reference_512(bunny_w4):
    """The 512-spp frame from seed 1234, linear, computed once."""
    r = _renderer(seed=1234)
    r.render(bunny_w4, 512, 20)
    r.synchronize()
    out = (r.linear().astype(np.float64) / 512)
    out.setflags(write=False)
    return out


def _rms(a, ref):
    return float(np.sqrt(np.mean((a.astype(np.float64) - ref) ** 2)))


def test_render_guides_denoise_resolve(bunny_w4, reference_512):
    spp = 16
    scale = crt_amd.pixel_sample_scale(spp)
    r = _renderer()
    r.render(bunny_w4, spp, 20)
    r.resolve(scale)
    before = _state(r)
    r.compute_guides(bunny_w4)
    stats = r.denoise(*SIGMAS, scale=scale)
    after = _state(r)
    for k in before:
        assert same(before[k], after[k]), k
    g = r.guides()
    raw = (F32(scale) * before["sum"]).astype(F32)
    want = dm.denoise(raw, g, *SIGMAS, 5)
    got = r.denoised()
    assert np.array_equal(dm.canon(got), dm.canon(want))
    assert stats["iterations"] == 5 and stats["pixels_hit"] == int((g[..., 3] >= 0).sum()) > 0
    assert stats["filter_ms"] > 0 and stats["guides_ms"] > 0
    per = r.denoise_iteration_ms()
    assert len(per["iteration_ms"]) == 5 and per["input_ms"] > 0 and all(v > 0 for v in per["iteration_ms"])
    assert per["input_ms"] + sum(per["iteration_ms"]) <= stats["filter_ms"] * 1.001 + 1e-3     # the parts lie inside the whole
    assert r.denoised_device_ptr() != 0
    # the direct kernel alone, fewer iterations, and the trace options: the same model
    r.denoise(*SIGMAS, scale=scale, direct_only=True)
    assert same(r.denoised(), got)
    r.compute_guides(bunny_w4, mode=2)
    assert same(r.guides(), g)
    s3 = r.denoise(1.0, 0.5, 0.1, iterations=3, scale=scale)
    assert s3["iterations"] == 3 and np.array_equal(dm.canon(r.denoised()), dm.canon(dm.denoise(raw, g, 1.0, 0.5, 0.1, 3)))
    # the resolved bytes are those of the denoised frame written as sums and resolved with scale 1
    r.denoise(*SIGMAS, scale=scale)
    r.resolve_denoised()
    r.synchronize()
    r2 = crt_amd.Renderer(W, H)
    r2.write_linear(got)
    r2.resolve(1.0)
    r2.synchronize()
    assert np.array_equal(r.rgba8(), r2.rgba8()) and not np.array_equal(r.rgba8(), before["rgba"])
    assert same(r.linear(), before["sum"]) and same(r.rng_state(), before["rng"])
    # the filter lowers the error: a condition on the frame, not a tuned threshold
    raw_rms, den_rms = _rms(raw, reference_512), _rms(got, reference_512)
    print(f"raw RMS {raw_rms:.4f}, denoised RMS {den_rms:.4f}")
    assert den_rms < raw_rms


def test_tile_scale_after_an_adaptive_render(bunny_w4):
    r = _renderer()
    r.render_adaptive(bunny_w4, 4, 32, INF)
    e = r.tile_error().reshape(-1)
    tol = float(np.median(e[e > 0]))
    r = _renderer()
    r.render_adaptive(bunny_w4, 4, 32, tol)
    spp = r.tile_spp().reshape(-1)
    assert len(np.unique(spp)) > 1
    before = _state(r)
    r.compute_guides(bunny_w4)
    stats = r.denoise(*SIGMAS, tile_scale=True)
    scale = (F32(1) / am.expand(spp, W, H).astype(F32)).astype(F32)
    raw = (scale[..., None] * before["sum"]).astype(F32)
    assert np.array_equal(dm.canon(r.denoised()), dm.canon(dm.denoise(raw, r.guides(), *SIGMAS, 5)))
    assert stats["iterations"] == 5
    after = _state(r)
    for k in before:
        assert same(before[k], after[k]), k
    assert np.array_equal(r.tile_spp().reshape(-1), spp)


# ------------------------------------------------------------------------------------------ 4. refusals on a real handle
def _nothing_allocated(r):
    assert r.denoised_device_ptr() == 0
    with pytest.raises(crt_amd.CrtError, match="no guides"):
        r.guides()
    with pytest.raises(crt_amd.CrtError, match="no denoised"):
        r.denoised()


def test_refusals_on_a_real_handle(bunny_w4):
    r = _renderer()
    r.render(bunny_w4, 2, 20)
    before = _state(r)
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*no guides"):
        r.denoise(*SIGMAS, scale=0.5)
    _nothing_allocated(r)
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*adaptive"):
        r.denoise(*SIGMAS, tile_scale=True)
    _nothing_allocated(r)
    r.set_pixel_shard(1, 2)
    with pytest.raises(crt_amd.CrtError, match=r"status -5.*pixel shard"):
        r.compute_guides(bunny_w4)
    with pytest.raises(crt_amd.CrtError, match=r"status -5.*pixel shard"):
        r.denoise(*SIGMAS, scale=0.5)
    _nothing_allocated(r)
    r.set_pixel_shard(0, 1)
    fn = _lib.hip().crt_renderer_denoise
    for o, word in ((_lib.DenoiseOptions(9, 4.0, INF, 0.05, 0, 0), "iterations"),
                    (_lib.DenoiseOptions(5, -4.0, INF, 0.05, 0, 0), "sigma_color"),
                    (_lib.DenoiseOptions(5, 4.0, float("nan"), 0.05, 0, 0), "sigma_normal"),
                    (_lib.DenoiseOptions(5, 4.0, INF, 2.0 ** 51, 0, 0), "sigma_position")):
        assert fn(r.h, C.byref(o), C.c_float(0.5), None, None) == INVALID
        assert word in _lib.hip().crt_last_error().decode()
        _nothing_allocated(r)
    no_camera = crt_amd.Renderer(W, H)
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*camera"):
        no_camera.compute_guides(bunny_w4)
    _nothing_allocated(no_camera)
    after = _state(r)
    for k in before:
        assert same(before[k], after[k]), k
    # the same handle then works, with and without a stats pointer
    r.compute_guides(bunny_w4)
    # with guides, the bad options are still refused and leave no denoised frame
    o = _lib.DenoiseOptions(9, 4.0, INF, 0.05, 0, 0)
    assert fn(r.h, C.byref(o), C.c_float(0.5), None, None) == INVALID
    with pytest.raises(crt_amd.CrtError, match="no denoised"):
        r.denoised()
    with pytest.raises(crt_amd.CrtError, match=r"status -1.*adaptive"):
        r.denoise(*SIGMAS, tile_scale=True)
    o = _lib.DenoiseOptions(0, 4.0, INF, 0.05, 0, 0)              # 0 iterations = 5
    assert fn(r.h, C.byref(o), C.c_float(0.5), None, None) == 0
    r.synchronize()
    with pytest.raises(crt_amd.CrtError, match="stats pointer"):          # that call recorded no per-launch events
        r.denoise_iteration_ms()
    raw = (F32(0.5) * before["sum"]).astype(F32)
    assert np.array_equal(dm.canon(r.denoised()), dm.canon(dm.denoise(raw, r.guides(), *SIGMAS, 5)))


# ------------------------------------------------------------------------------------------ 5. the checked build
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
r.set_camera(crt_amd.camera(1))
r.init_rand(41)
r.render(sc, 16, 20)
r.compute_guides(sc)
stats = r.denoise(4.0, float("inf"), 0.05, scale=crt_amd.pixel_sample_scale(16))
r.resolve_denoised()
r.synchronize()                                          # a device error of the checked build raises here
np.savez(sys.argv[2], flags=np.array(_lib.hip().crt_build_flags()), guides=r.guides(), denoised=r.denoised(),
         rgba=r.rgba8(), sum=r.linear(), hit=np.array(stats["pixels_hit"]))
"""


def test_checked_build_gives_the_same_bits(bunny_w4, tmp_path):
    assert CHECKED.exists() and _lib.hip().crt_build_flags() == 0
    out = tmp_path / "checked.npz"
    p = subprocess.run([sys.executable, "-c", CHILD, str(REPO), str(out)],
                       env=dict(os.environ, CRT_HIP_LIB=str(CHECKED)), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(out)
    assert int(got["flags"]) == _lib.BUILD_CHECKED
    r = _renderer()
    r.render(bunny_w4, 16, 20)
    r.compute_guides(bunny_w4)
    stats = r.denoise(*SIGMAS, scale=crt_amd.pixel_sample_scale(16))
    r.resolve_denoised()
    r.synchronize()
    assert same(got["sum"], r.linear()) and same(got["guides"], r.guides())
    assert np.array_equal(dm.canon(got["denoised"]), dm.canon(r.denoised()))
    assert np.array_equal(got["rgba"], r.rgba8()) and int(got["hit"]) == stats["pixels_hit"]


# ------------------------------------------------------------------------------------------ 6. the CLI
def _read_ppm(path):
    data = path.read_bytes()
    fields, pos = [], 0
    while len(fields) < 4:
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        fields.append(data[pos:end])
        pos = end + 1
    assert fields[0] == b"P6" and fields[3] == b"255"
    w, h = int(fields[1]), int(fields[2])
    return np.frombuffer(data[pos:pos + w * h * 3], np.uint8).reshape(h, w, 3)


def test_cli_denoise(device_scenes, scenes, tmp_path):
    sc = device_scenes["cornell_bunny"][1]                 # the CLI's default tree is the reference's
    spp = 16
    r = _renderer()
    r.render(sc, spp, 20)
    r.compute_guides(sc)
    r.denoise(*SIGMAS, iterations=4, scale=crt_amd.pixel_sample_scale(spp))
    r.resolve_denoised()
    want = _state(r)
    out = tmp_path / "denoised.ppm"
    p = subprocess.run([str(CLI), "-w", str(W), "-h", str(H), "-spp", str(spp), "-denoise", "4:inf:0.05", "-denoise-iters", "4",
                        "-o", str(out), *map(str, scenes["cornell_bunny"])], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(info) == {"width", "height", "spp", "rays", "setup_s", "frame_s", "kernel_ms", "mrays_per_s", "guides_ms",
                         "filter_ms", "out"}
    assert info["guides_ms"] > 0 and info["filter_ms"] > 0
    assert np.array_equal(_read_ppm(out), want["rgba"][::-1, :, :3])     # the file holds the top row first
    # with -adaptive the filter takes the tiles' own scales
    r = _renderer()
    r.render_adaptive(sc, 4, 32, 0.05)
    r.compute_guides(sc)
    r.denoise(*SIGMAS, tile_scale=True)
    r.resolve_denoised()
    want = _state(r)
    p = subprocess.run([str(CLI), "-w", str(W), "-h", str(H), "-spp", "32", "-spp-min", "4", "-adaptive", "0.05", "-denoise",
                        "4:inf:0.05", "-o", str(out), *map(str, scenes["cornell_bunny"])], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert info["guides_ms"] > 0 and info["filter_ms"] > 0 and info["passes"] >= 0
    assert np.array_equal(_read_ppm(out), want["rgba"][::-1, :, :3])
    # a malformed value is a usage error, and without the flag the program prints what it printed before
    p = subprocess.run([str(CLI), "-denoise", "4:inf", *map(str, scenes["cornell_bunny"])], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 2 and "-denoise" in p.stderr
    p = subprocess.run([str(CLI), "-w", str(W), "-h", str(H), "-spp", "2", "-o", str(tmp_path / "plain.ppm"),
                        *map(str, scenes["cornell_bunny"])], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(info) == {"width", "height", "spp", "rays", "setup_s", "frame_s", "kernel_ms", "mrays_per_s", "out"}
