"""Path steps on the GPU (crt_amd.paths: camera_rays, Scene.path_step, the wavefront driver paths.render): DESIGN.md §16.

Every comparison is bit for bit; frames are 64x36 unless stated.

1. camera rays and the RNG state after them == pyoracle.kat_get_ray over every pixel (64x36, and 65x37 with its
   partial last wave), bench and wide-aperture cameras, a second call, permuted and partial pixel lists, n = 0.
2. paths.render on cornell_bunny == the committed golden frame (sums, RGBA8, ray count), RNG == Renderer.render's.
3. bounce limit and roulette: config A at 4 and 20 bounces against frames.json; 1 and 3 bounces against Renderer.render.
4. the rebuilt 4-wide tree, lane and stream queries, against Renderer.render (automatic variant and variant 4).
5. the soup family, sphere worlds and a world with an out-of-range and an unknown-type material against Renderer.render.
6. a path's result depends only on its own entry: permutation, prefixes around the wave size, single entries, entries
   that come in ENDED.
7. hand-built hit records against a float32 restatement of what draws nothing.
8. the calls on a side stream without synchronisation == the default stream.
9. the checked build gives the same bits.
"""
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
import synth_scenes as synth  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
CHECKED = REPO / "raytracer-cuda_amd" / "lib" / "checked" / "libcrt_hip.so"
F32 = np.float32
W, H = 64, 36
INVALID = 5          # the step kernel's code of a material index outside the scene's materials


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _renderer(cam, w=W, h=H, seed=41):
    r = crt_amd.Renderer(w, h)
    r.set_camera(cam)
    r.init_rand(seed)
    return r


def _frame(r, spp):
    r.resolve(crt_amd.pixel_sample_scale(spp))
    r.synchronize()
    return {"sum": r.linear(), "rgba": r.rgba8(), "rng": r.rng_state()}


def _direct(scene, cam, spp, bounces, w=W, h=H, variant=None):
    """Renderer.render's frame and its ray count."""
    r = _renderer(cam, w, h)
    if variant is not None:
        r.set_kernel_variant(variant)
    r.render(scene, spp, bounces, count_work=True)
    out = _frame(r, spp)
    out["rays"] = r.counters()["rays"]
    return out


def _wavefront(scene, cam, spp, bounces, w=W, h=H, **kw):
    r = _renderer(cam, w, h)
    res = paths.render(scene, r, spp, bounces, **kw)
    out = _frame(r, spp)
    out["rays"], out["iterations"] = res["rays"], res["iterations"]
    return out


def _assert_frames_equal(got, want, what):
    for k in ("sum", "rgba", "rng"):
        assert _same(got[k], want[k]), f"{what}: {k} differs in {int((_bits(got[k]) != _bits(want[k])).sum())} words"
    assert got["rays"] == want["rays"], (what, got["rays"], want["rays"])


# ------------------------------------------------------------------------------------------ 1. camera rays
def _oracle_rays(cam, w, h, state):
    xy = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2).astype(np.int32)
    import pyoracle
    return pyoracle.kat_get_ray(crt_amd.camera_floats(cam), w, h, xy, state)     # continues `state` in place


@pytest.fixture(scope="module")
def init_states():
    import pyoracle
    n = 65 * 37
    st = np.stack([pyoracle.rng_init(41, i) for i in range(n)])
    st.setflags(write=False)
    return st


def _check_camera_batch(rays, pth, want, pixels):
    rays, pth = rays.cpu().numpy(), pth.cpu().numpy()
    n = len(pixels)
    assert rays.shape == (n, 8) and pth.shape == (n, 8) and pth.dtype == np.int32
    assert _same(rays[:, :3], want[pixels, :3]) and _same(rays[:, 4:7], want[pixels, 3:])
    assert np.isposinf(rays[:, 3]).all() and not _bits(rays[:, 7]).any()
    assert _same(pth[:, :3].view(F32), np.ones((n, 3), F32)) and not pth[:, 3].any()
    assert np.array_equal(pth[:, paths.PATH_PIXEL], pixels) and not pth[:, 5:].any()


@pytest.mark.parametrize("size", [(64, 36), (65, 37)])
@pytest.mark.parametrize("lens", ["bench", "wide"])
def test_camera_rays_equal_the_oracle(init_states, size, lens):
    import torch
    w, h = size
    n = w * h
    cam = crt_amd.camera(1) if lens == "bench" else crt_amd.camera(1, aperture=0.2, focus=0.5)
    assert lens == "bench" or cam.lens_radius > 0.05
    state = init_states[:n].copy()
    r = _renderer(cam, w, h)
    assert _same(r.rng_state().reshape(n, 6), state)
    every = np.arange(n)
    first = _oracle_rays(cam, w, h, state)
    after_first = state.copy()
    _check_camera_batch(*crt_amd.camera_rays(r), first, every)
    assert _same(r.rng_state().reshape(n, 6), after_first)
    second = _oracle_rays(cam, w, h, state)                     # a second call continues the streams
    assert not _same(first, second)
    _check_camera_batch(*crt_amd.camera_rays(r), second, every)
    assert _same(r.rng_state().reshape(n, 6), state)
    # pixel lists: a permutation, subsets around the wave size, none; pixels not named keep their state
    perm = np.random.default_rng(3).permutation(n).astype(np.int32)
    for pixels in [perm] + [perm[:k] for k in (1, 63, 64, 65, 129, 0)]:
        r.init_rand(41)
        t = torch.from_numpy(pixels.copy()).to("cuda:0")
        _check_camera_batch(*crt_amd.camera_rays(r, t), first, pixels)
        want = init_states[:n].copy()
        want[pixels] = after_first[pixels]
        assert _same(r.rng_state().reshape(n, 6), want), len(pixels)
    # a caller's own state tensor: the renderer's is left alone
    r.init_rand(41)
    own = torch.from_numpy(init_states[:n].view(np.int32).copy()).to("cuda:0")
    _check_camera_batch(*crt_amd.camera_rays(r, rng=own), first, every)
    assert _same(own.cpu().numpy(), after_first) and _same(r.rng_state().reshape(n, 6), init_states[:n])
    # a pixel outside the frame draws nothing and comes back ended
    t = torch.tensor([5, n, -1, 7], dtype=torch.int32, device="cuda:0")
    rays, pth = crt_amd.camera_rays(r, t)
    assert pth[:, paths.PATH_STATUS].tolist() == [0, 1, 1, 0] and pth[:, paths.PATH_PIXEL].tolist() == [5, n, -1, 7]
    _check_camera_batch(rays[[0, 3]], pth[[0, 3]], first, np.array([5, 7]))


# ------------------------------------------------------------------------------------------ 2. the golden frame
@pytest.mark.parametrize("regenerate", [True, False])
def test_golden_frame(device_scenes, regenerate):
    g = np.load(GOLDEN / "cornell_bunny_64x36_16spp.npz")
    frames = json.loads((GOLDEN / "frames.json").read_text())
    _, scene = device_scenes["cornell_bunny"]
    cam = crt_amd.camera(16)
    got = _wavefront(scene, cam, 16, 20, regenerate=regenerate)
    print(f"\nregenerate={regenerate}: {got['rays']} rays in {got['iterations']} iterations")
    assert _same(got["sum"], g["sum"]) and np.array_equal(got["rgba"], g["rgba"])
    assert got["rays"] == frames["cornell_bunny_64x36_16spp_20b"]["rays"]
    want = _direct(scene, cam, 16, 20)
    _assert_frames_equal(got, want, "golden frame")


# ------------------------------------------------------------------------------------------ 3. bounce limit, roulette
@pytest.mark.parametrize("bounces", [4, 20])
def test_config_a(device_scenes, bounces):
    want = json.loads((GOLDEN / "frames.json").read_text())[f"configA_256x256_16spp_{bounces}b"]
    _, scene = device_scenes["cornell"]
    got = _wavefront(scene, crt_amd.camera(16), 16, bounces, 256, 256)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()   # noqa: E731
    print(f"\nconfig A, {bounces} bounces: {got['rays']} rays in {got['iterations']} iterations")
    assert got["rays"] == want["rays"]
    assert sha(got["sum"]) == want["sum_sha256"] and sha(got["rgba"]) == want["rgba_sha256"]


@pytest.mark.parametrize("regenerate", [True, False])
@pytest.mark.parametrize("bounces", [1, 3])
def test_short_paths(device_scenes, bounces, regenerate):
    _, scene = device_scenes["cornell_bunny"]
    cam = crt_amd.camera(16)
    got = _wavefront(scene, cam, 16, bounces, regenerate=regenerate)
    _assert_frames_equal(got, _direct(scene, cam, 16, bounces), f"{bounces} bounces")
    assert bounces != 1 or got["rays"] == 16 * W * H


# ------------------------------------------------------------------------------------------ 4. rebuilt tree
@pytest.fixture(scope="module")
def bunny_w4(device_scenes):
    hs, _ = device_scenes["cornell_bunny"]
    return hs.upload(0, bvh="rebuilt", width=4)


@pytest.mark.parametrize("query", ["lane", "stream"])
def test_rebuilt_tree(bunny_w4, query):
    cam = crt_amd.camera(16)
    opts = dict(mode=1) if query == "lane" else dict(mode=2, grid_waves=1)
    got = _wavefront(bunny_w4, cam, 16, 20, trace_options=opts)
    for variant in (None, 4):
        _assert_frames_equal(got, _direct(bunny_w4, cam, 16, 20, variant=variant), f"{query} / variant {variant}")


# ------------------------------------------------------------------------------------------ 5. materials, spheres
def _odd_materials_world(scenes):
    """40 spheres cycling through the five sphere materials, one whose material index is outside the scene's materials
    (the reference's same-ray bounce), one of an unknown material type (emits nothing) and one of metal with fuzz 1,
    which absorbs many of its hits, in the Cornell box."""
    k = len(synth.SPHERE_MATS)
    spheres = synth.random_spheres(40) + [((0.1, -0.1, 0.1), 0.06, 99), ((-0.1, -0.12, 0.12), 0.06, k),
                                          ((0.0, 0.12, 0.1), 0.06, k + 1)]
    mats = synth.SPHERE_MATS + [custom_scene.mat_row(7, (0.3, 0.3, 0.3), (2, 2, 2)),
                                custom_scene.mat_row(1, (0.9, 0.9, 0.9), roughness=1.0)]
    return custom_scene.CustomScene(scenes["cornell"], spheres, mats)


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, scenes):
    out = custom_scene.synth_worlds(custom_scene.family_files(tmp_path_factory.mktemp("ps")))
    out["odd_materials"] = _odd_materials_world(scenes)
    return out


@pytest.mark.parametrize("name", ["soup", "s0", "s1", "s9_ground", "s40", "odd_materials"])
def test_synthetic_worlds(worlds, name):
    cs = worlds[name]
    scene = cs.upload(0)
    cam = crt_amd.camera(4)
    want = _direct(scene, cam, 4, 20)
    for regenerate in (True, False):
        _assert_frames_equal(_wavefront(scene, cam, 4, 20, regenerate=regenerate), want, f"{name} regenerate={regenerate}")
    if name == "soup":
        assert set(paths.shade_rows(cs.desc)[:, 0, 0].view(np.int32).tolist()) >= {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------ 6. own entry only
class Batch:
    """One traced batch of the odd-materials world and everything a step of it reads, on the host."""

    def __init__(self, scene, rows, rays, hits, pth, rng, lin):
        self.scene, self.rows = scene, rows
        self.rays, self.hits, self.pth, self.rng, self.lin = rays, hits, pth, rng, lin
        for a in (rays, hits, pth, rng, lin):
            a.setflags(write=False)

    def step(self, idx, pth=None):
        """The step over entries idx (in that order) on copies of the state: rays, paths, RNG words and sums after."""
        import torch
        dev = "cuda:0"
        rays = torch.from_numpy(self.rays[idx].copy()).to(dev)
        hits = torch.from_numpy(self.hits[idx].copy()).to(dev)
        p = torch.from_numpy((self.pth if pth is None else pth)[idx].copy()).to(dev)
        rng = torch.from_numpy(self.rng.view(np.int32).copy()).to(dev)
        lin = torch.from_numpy(self.lin.copy()).to(dev)
        self.scene.path_step(rays, hits, p, 20, rng, lin)
        torch.cuda.synchronize()
        return rays.cpu().numpy(), p.cpu().numpy(), rng.cpu().numpy().view(np.uint32), lin.cpu().numpy()

    def code(self):
        """Per entry: the step kernel's material code, -1 for a miss."""
        mat = self.hits[:, 3].view(np.int32)
        codes = self.rows[:, 0, 0].view(np.int32)
        ok = (mat >= 0) & (mat < len(codes))
        c = np.where(ok, codes[np.clip(mat, 0, len(codes) - 1)], INVALID)
        return np.where(self.hits[:, 0] < 0, -1, c)


def _classes(b, after_pth):
    code = b.code()
    front = b.hits[:, 7].view(np.int32) != 0
    ended = after_pth[:, paths.PATH_STATUS] == _lib.PATH_ENDED
    same_bounce = after_pth[:, paths.PATH_BOUNCE] == b.pth[:, paths.PATH_BOUNCE]
    return {"miss": code == -1, "lambertian": code == 0, "metal": code == 1, "glass": code == 2, "light": code == 3,
            "unknown type": code == 4, "invalid index": code == INVALID, "glass from inside": (code == 2) & ~front,
            "metal absorbed": (code == 1) & ended & same_bounce}


@pytest.fixture(scope="module")
def batch(worlds):
    """The wavefront of the odd-materials world, one path per pixel with regeneration (2,304 entries in every
    iteration); the first of its first 24 iterations' batches that holds every class of entry."""
    import torch
    cs = worlds["odd_materials"]
    scene = cs.upload(0)
    rows = paths.shade_rows(cs.desc)
    r = _renderer(crt_amd.camera(64))
    r.write_linear(np.zeros((H, W, 3), F32))
    rays, pth = crt_amd.camera_rays(r)
    seen = {}
    for it in range(24):
        hits = scene.trace(rays)["f32"]
        r.synchronize()
        b = Batch(scene, rows, rays.cpu().numpy(), hits.cpu().numpy(), pth.cpu().numpy(),
                  r.rng_state().reshape(-1, 6), r.linear().reshape(-1, 3))
        assert len(b.rays) == W * H and len(np.unique(b.pth[:, paths.PATH_PIXEL])) == W * H
        after = b.step(np.arange(W * H))
        seen = {k: int(v.sum()) for k, v in _classes(b, after[1]).items()}
        if all(seen.values()):
            print(f"\nbatch of iteration {it}: {seen}")
            b.after = after
            return b
        scene.path_step(rays, hits, pth, 20, r, r)
        ended = (pth[:, paths.PATH_STATUS] == _lib.PATH_ENDED).nonzero().squeeze(1)
        if ended.numel():                       # every ended path's pixel starts its next sample
            rays[ended], pth[ended] = crt_amd.camera_rays(r, pth[ended, paths.PATH_PIXEL].contiguous())
    raise AssertionError(f"no batch with every class of entry in 24 iterations; the last one: {seen}")


def _assert_entries(b, idx, got, what):
    """`got` = step over entries idx: each entry's ray, path, RNG words and sum equal the full batch's; every pixel
    that no entry of idx names keeps its RNG words and sum."""
    rays, pth, rng, lin = got
    f_rays, f_pth, f_rng, f_lin = b.after
    pix = b.pth[idx, paths.PATH_PIXEL]
    assert _same(rays, f_rays[idx]) and _same(pth, f_pth[idx]), what
    assert _same(rng[pix], f_rng[pix]) and _same(lin[pix], f_lin[pix]), what
    rest = np.setdiff1d(np.arange(len(b.rng)), pix)
    assert _same(rng[rest], b.rng[rest]) and _same(lin[rest], b.lin[rest]), what


def test_batch_holds_every_class(batch):
    n = W * H
    cls = _classes(batch, batch.after[1])
    assert len(batch.rays) >= 2304 and all(v.any() for v in cls.values()), {k: int(v.sum()) for k, v in cls.items()}
    rays, pth, rng, lin = batch.after
    ended = pth[:, paths.PATH_STATUS] == _lib.PATH_ENDED
    # what ends: every miss, light and unknown type; a ray that ended is left as it was, a path that goes on moved on
    for k in ("miss", "light", "unknown type"):
        assert ended[cls[k]].all(), k
    assert _same(rays[ended], batch.rays[ended])
    go = ~ended
    assert (pth[go, paths.PATH_BOUNCE] == batch.pth[go, paths.PATH_BOUNCE] + 1).all() and np.isposinf(rays[go, 3]).all()
    inv = cls["invalid index"] & go
    assert inv.any() and _same(rays[inv], batch.rays[inv])
    early = inv & (pth[:, paths.PATH_BOUNCE] < 3)          # no roulette yet: the throughput is as it was
    assert _same(pth[early, :3], batch.pth[early, :3])
    assert np.array_equal(pth[:, paths.PATH_PIXEL], batch.pth[:, paths.PATH_PIXEL]) and n == len(pth)
    # a sum moves only where a path ended; an unknown type and an absorbed metal add exactly nothing
    assert _same(lin[batch.pth[go, paths.PATH_PIXEL]], batch.lin[batch.pth[go, paths.PATH_PIXEL]])
    for k in ("unknown type", "metal absorbed"):
        p = batch.pth[cls[k], paths.PATH_PIXEL]
        assert np.array_equal(lin[p], batch.lin[p]), k
    # glass from inside with total internal reflection: the scattered ray stays inside (it leaves along the normal's side)
    assert cls["glass from inside"].sum() >= 1


def test_permutation(batch):
    perm = np.random.default_rng(4).permutation(len(batch.rays))
    _assert_entries(batch, perm, batch.step(perm), "permuted")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_prefixes_around_the_wave_size(batch, n):
    _assert_entries(batch, np.arange(n), batch.step(np.arange(n)), f"first {n}")
    tail = np.arange(len(batch.rays) - n, len(batch.rays))
    _assert_entries(batch, tail, batch.step(tail), f"last {n}")


def test_single_entries_of_every_class(batch):
    for k, mask in _classes(batch, batch.after[1]).items():
        for i in np.nonzero(mask)[0][:2]:
            _assert_entries(batch, np.array([i]), batch.step(np.array([i])), f"{k}, entry {i}")


def test_ended_entries_are_left_alone(batch):
    n = len(batch.rays)
    pth = batch.pth.copy()
    off = np.zeros(n, bool)
    off[::3] = True
    off[np.random.default_rng(6).integers(0, n, 200)] = True
    pth[off, paths.PATH_STATUS] = _lib.PATH_ENDED
    rays, p, rng, lin = batch.step(np.arange(n), pth)
    on = np.nonzero(~off)[0]
    f_rays, f_pth, f_rng, f_lin = batch.after
    assert _same(rays[on], f_rays[on]) and _same(p[on], f_pth[on])
    pix_on, pix_off = batch.pth[on, paths.PATH_PIXEL], batch.pth[off, paths.PATH_PIXEL]
    assert _same(rng[pix_on], f_rng[pix_on]) and _same(lin[pix_on], f_lin[pix_on])
    assert _same(rays[off], batch.rays[off]) and _same(p[off], pth[off])
    assert _same(rng[pix_off], batch.rng[pix_off]) and _same(lin[pix_off], batch.lin[pix_off])


# ------------------------------------------------------------------------------------------ 7. hand-built hits
def _sky_f32(d):
    """sky(d) of CRTUtility.cuh:34-38 in float32 operation order, d one direction."""
    l2 = F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))
    uy = F32(F32(F32(1) / F32(np.sqrt(l2))) * d[1])
    t = F32(F32(0.5) * F32(uy + F32(1)))
    white = F32(F32(1) - t)
    return np.array([F32(white + F32(t * F32(c))) for c in (0.5, 0.7, 1.0)], F32)


def test_hand_built_hits(device_scenes):
    import torch
    hs, scene = device_scenes["cornell"]
    rows = paths.shade_rows(hs.desc())
    codes = rows[:, 0, 0].view(np.int32)
    light, diffuse = int(np.argmax(codes == 3)), int(np.argmax(codes == 0))
    assert codes[light] == 3 and codes[diffuse] == 0
    n_pix = 16
    rng0 = np.random.default_rng(8).integers(1, 2 ** 32, (n_pix, 6), dtype=np.uint64).astype(np.uint32)
    lin0 = np.random.default_rng(9).uniform(0, 4, (n_pix, 3)).astype(F32)
    o = np.random.default_rng(10).uniform(-0.2, 0.2, (7, 3)).astype(F32)
    d = np.random.default_rng(11).normal(size=(7, 3)).astype(F32)
    thr = np.array([0.5, 0.25, 1.0], F32)
    rays = crt_amd.pack_rays(o, d)
    hits = np.zeros(7, crt_amd.HIT_DTYPE)
    pth = np.zeros((7, 8), np.int32)
    pth[:, :3] = thr.view(np.int32)
    pth[:, paths.PATH_BOUNCE] = 1
    pth[:, paths.PATH_PIXEL] = [3, 0, 9, 15, 7, 12, 5]
    hits["t"] = [-1, 0.75, 1.5, 0.5, 0.25, 2.0, 0.5]
    hits["material"] = [0, light, diffuse, len(codes), -1, diffuse, len(codes) + 7]
    hits["normal"] = [(0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 1, 0)]
    hits["front_face"] = [0, 1, 0, 1, 0, 1, 1]
    pth[6, paths.PATH_BOUNCE] = 19                       # the invalid-material bounce reaches the limit of 20
    pth[5, paths.PATH_STATUS] = _lib.PATH_ENDED         # comes in ended
    dev = "cuda:0"
    t_rays, t_pth = torch.from_numpy(rays.copy()).to(dev), torch.from_numpy(pth.copy()).to(dev)
    t_hits = torch.from_numpy(hits.view(F32).reshape(7, 8).copy()).to(dev)
    t_rng, t_lin = torch.from_numpy(rng0.view(np.int32).copy()).to(dev), torch.from_numpy(lin0.copy()).to(dev)
    scene.path_step(t_rays, t_hits, t_pth, 20, t_rng, t_lin)
    torch.cuda.synchronize()
    g_rays, g_pth = t_rays.cpu().numpy(), t_pth.cpu().numpy()
    g_rng, g_lin = t_rng.cpu().numpy().view(np.uint32), t_lin.cpu().numpy()
    pix = pth[:, paths.PATH_PIXEL]
    want_lin, want_rng = lin0.copy(), rng0.copy()
    # 0: a miss -- sum += throughput * sky(d), nothing drawn
    want_lin[3] = lin0[3] + (thr * _sky_f32(d[0])).astype(F32)
    # 1: a light -- sum += the emission itself (rayColor returns emit() raw), nothing drawn
    want_lin[0] = lin0[0] + rows[light, 1, :3]
    # 6: invalid material at bounce 19 -> 20 = the limit: ends with + (0, 0, 0), nothing drawn
    for k in (0, 1, 6):
        assert g_pth[k, paths.PATH_STATUS] == _lib.PATH_ENDED and _same(g_rays[k], rays[k]), k
        assert _same(g_rng[pix[k]], rng0[pix[k]]), k
    assert g_pth[6, paths.PATH_BOUNCE] == 20 and g_pth[0, paths.PATH_BOUNCE] == 1
    # 3, 4: material index past the end / negative -- the same ray again, ++bounce, throughput kept, nothing drawn
    for k in (3, 4):
        assert g_pth[k].tolist() == [*thr.view(np.int32).tolist(), 2, pix[k], _lib.PATH_ACTIVE, 0, 0], k
        assert _same(g_rays[k, :3], rays[k, :3]) and _same(g_rays[k, 4:7], rays[k, 4:7]) and np.isposinf(g_rays[k, 3])
        assert _same(g_rng[pix[k]], rng0[pix[k]]), k
    # 2: a diffuse hit on the back face -- leaves from o + t * d with throughput * albedo, on the flipped normal's side
    hp = (o[2] + (F32(1.5) * d[2]).astype(F32)).astype(F32)
    assert g_pth[2, paths.PATH_STATUS] == _lib.PATH_ACTIVE and g_pth[2, paths.PATH_BOUNCE] == 2
    assert _same(g_rays[2, :3], hp) and np.isposinf(g_rays[2, 3]) and g_rays[2, 7] == 0
    assert _same(g_pth[2, :3].view(F32), (thr * rows[diffuse, 1, :3]).astype(F32))
    assert g_rays[2, 6] < 0, "scattered about -normal = (0, 0, -1): n + unit vector has z <= 0"
    assert not _same(g_rng[9], rng0[9])                  # the unit-sphere draws
    want_rng[9] = g_rng[9]
    # 5: came in ended -- untouched
    assert _same(g_rays[5], rays[5]) and _same(g_pth[5], pth[5])
    assert _same(g_lin, want_lin) and _same(g_rng, want_rng)


# ------------------------------------------------------------------------------------------ 8. side stream
def _fixed_rounds(scene, r, rng0, rounds, gated=False):
    """camera rays and `rounds` trace / step rounds on the current stream, on the caller's own state tensors, without
    compaction (ended entries stay in the batch and are skipped) and without any synchronisation.  gated: the current
    stream is held back first (helpers/stream_gate.py), and the state tensors are made on it behind the gate."""
    import torch
    rng = torch.from_numpy(rng0.view(np.int32).copy()).to("cuda:0", non_blocking=False)
    if gated:
        torch.cuda.synchronize()
        stream_gate.gate(torch.cuda.current_stream())
        rng = rng.clone()
    lin = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.default_stream())
    rays, pth = crt_amd.camera_rays(r, rng=rng)
    for _ in range(rounds):
        hits = scene.trace(rays, mode=2, grid_waves=8)["f32"]
        scene.path_step(rays, hits, pth, 20, rng, lin)
    return rays, pth, rng, lin


def test_side_stream(bunny_w4):
    import torch
    r = _renderer(crt_amd.camera(1))
    r.synchronize()
    rng0 = r.rng_state().reshape(-1, 6)
    base = _fixed_rounds(bunny_w4, r, rng0, 6)
    torch.cuda.synchronize()
    side = stream_gate.side_stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side and side != torch.cuda.default_stream()
        got = _fixed_rounds(bunny_w4, r, rng0, 6, gated=True)
    side.synchronize()
    for a, b, k in zip(got, base, ("rays", "paths", "rng", "sums")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    status = base[1][:, paths.PATH_STATUS]
    assert (status == _lib.PATH_ENDED).any() and (status == _lib.PATH_ACTIVE).any() and base[3].any()
    assert _same(r.rng_state().reshape(-1, 6), rng0)       # the renderer's own state was not used


# ------------------------------------------------------------------------------------------ 9. checked build
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
r = crt_amd.Renderer(64, 36)
r.set_camera(crt_amd.camera(2))
r.init_rand(41)
res = paths.render(sc, r, 2, 20)
r.resolve(crt_amd.pixel_sample_scale(2))
r.synchronize()                                      # a device error of the checked build raises here
np.savez(sys.argv[2], flags=np.array(_lib.hip().crt_build_flags()), sum=r.linear(), rgba=r.rgba8(), rng=r.rng_state(),
         rays=np.array(res["rays"]))
"""


def test_checked_build_gives_the_same_bits(bunny_w4, tmp_path):
    assert CHECKED.exists() and _lib.hip().crt_build_flags() == 0
    res = tmp_path / "checked.npz"
    p = subprocess.run([sys.executable, "-c", CHILD, str(REPO), str(res)], env=dict(os.environ, CRT_HIP_LIB=str(CHECKED)),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = np.load(res)
    assert int(got["flags"]) == _lib.BUILD_CHECKED
    want = _wavefront(bunny_w4, crt_amd.camera(2), 2, 20)
    _assert_frames_equal({k: got[k] for k in ("sum", "rgba", "rng")} | {"rays": int(got["rays"])}, want, "checked build")
    _assert_frames_equal(want, _direct(bunny_w4, crt_amd.camera(2), 2, 20), "fast build against Renderer.render")
