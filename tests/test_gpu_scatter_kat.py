"""The scatter step on the GPU against the known answers of tests/golden/scatter_kat.npz ("Known answers
of the scatter step"; the CPU half is tests/test_scatter_kat.py).

Every record of the fixture is one hand-made hit with chosen draws: general position, the glass test's f64 band, the
Schlick draw on either side of equality, Lambert's degenerate sum, metal at dot = 0, the roulette at u == p and with
1 / p by IEEE division, the bounce limit, directions of extreme length, NaNs, invalid materials.  Stage B of the
oracle is what the device must leave, bit for bit (NaNs canonicalised):

a. Scene.path_step over the whole fixture, one pixel per record;
b. the same records in other wave compositions: sorted by class, permuted, every slow-sequence record as lane 0, 31
   and 63 of a wave of general-position records, and single records;
c. Scene.path_advance with remaining=None, direct and with count_in: the count, the appended rows, the sums, the RNG;
d. crt_selftest_shade: shade_rec() + next_ray(), the render kernels' twin of scatter_step(), on the same records.

A record whose bounce limit is not the call's comes in ENDED and must be left alone, so every call also checks that.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

from crt_amd import _lib, paths

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import custom_scene  # noqa: E402
import scatter_kat as sk  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
F32, U32 = np.float32, np.uint32
LIMITS = (20, 1)                      # the bounce limits of the fixture's records


class Rig:
    def __init__(self, fx, scene, base):
        self.fx, self.scene, self.base = fx, scene, base
        self.label = fx["label"]

    def step(self, idx, max_bounces):
        """Scene.path_step over batch(idx): rays, paths, RNG words, sums after."""
        import torch
        rays, hits, pth, rng, lin = sk.batch(self.fx, idx, self.base, max_bounces)
        dev = "cuda:0"
        t = [torch.from_numpy(a).to(dev) for a in (rays, hits, pth, rng.view(np.int32), lin)]
        self.scene.path_step(t[0], t[1], t[2], max_bounces, t[3], t[4])
        torch.cuda.synchronize()
        return t[0].cpu().numpy(), t[2].cpu().numpy(), t[3].cpu().numpy().view(U32), t[4].cpu().numpy()

    def differing(self, idx, got, want):
        """The entries of which any word differs, as 'entry (record, class): arrays'."""
        bad = {}
        for name, g, w in zip(("rays", "paths", "rng", "sums"), got, want):
            assert g.shape == w.shape, name
            for j in np.nonzero((sk.canon(g) != sk.canon(w)).any(1))[0]:
                bad.setdefault(int(j), []).append(name)
        return [f"{j} (record {idx[j]}, {self.label[idx[j]].decode()}): {', '.join(v)}" for j, v in sorted(bad.items())]

    def check(self, idx, what):
        idx = np.asarray(idx)
        limits = [m for m in LIMITS if (self.fx["rec"][idx, sk.MAXB] == m).any()]
        for m in limits:
            bad = self.differing(idx, self.step(idx, m), sk.expected(self.fx, idx, self.base, m))
            assert not bad, f"{what}, max_bounces {m}: {len(bad)} entries differ from the oracle's stage B: {bad[:12]}"


@pytest.fixture(scope="module")
def rig(scenes):
    fx = sk.load(GOLDEN / "scatter_kat.npz")
    for a in fx.values():
        a.setflags(write=False)
    mats = fx["mats"].view(F32)
    cs = custom_scene.CustomScene(scenes["cornell"], [((0.0, 0.0, 0.0), 0.05, 0)], [list(map(float, m)) for m in mats])
    rows = paths.shade_rows(cs.desc)
    assert np.array_equal(sk.canon(rows[-len(mats):]), sk.canon(fx["rows"])), "the scene's rows are not the fixture's"
    assert set(fx["rec"][:, sk.MAXB].tolist()) == set(LIMITS)
    return Rig(fx, cs.upload(0), len(rows) - len(mats))


def _census(rig):
    got = sk.census(rig.fx)
    print("\ncensus: " + ", ".join(f"{k} {v}" for k, v in got.items()))
    assert not sk.census_missing(rig.fx)
    return got


# ------------------------------------------------------------------------------------------ a. the whole fixture
def test_path_step_over_the_fixture(rig):
    _census(rig)
    fx = rig.fx
    n = len(fx["rec"])
    idx = np.arange(n)
    rig.check(idx, "fixture order")
    # said once more without the helper: an entry that ends keeps its ray, one that goes on keeps its sum
    rays0, _, pth0, _, lin0 = sk.batch(fx, idx, rig.base, 20)
    rays, pth, rng, lin = rig.step(idx, 20)
    ran = pth0[:, paths.PATH_STATUS] == _lib.PATH_ACTIVE
    ended = pth[:, paths.PATH_STATUS] == _lib.PATH_ENDED
    assert (ran & ended).sum() > 100 and (ran & ~ended).sum() > 100
    # the comparison is not an empty one: the step moved every entry it ran (its bounce or its status) and no other
    moved = (pth != pth0).any(1)
    assert np.array_equal(moved, ran), np.nonzero(moved != ran)[0][:10]
    assert len(rig.differing(idx, (rays, pth, rng, lin), (rays0, pth0, fx["rec"][:, sk.RNG], lin0))) >= ran.sum()
    assert np.array_equal(sk.canon(rays[ended]), sk.canon(rays0[ended]))
    assert np.array_equal(sk.canon(lin[~ended]), sk.canon(lin0[~ended]))
    assert np.isposinf(rays[ran & ~ended, 3]).all() and not rays[ran & ~ended, 7].view(U32).any()
    assert np.array_equal(pth[:, paths.PATH_PIXEL], idx)


# ------------------------------------------------------------------------------------------ b. wave composition
def test_sorted_by_class(rig):
    _census(rig)
    order = np.argsort(rig.label, kind="stable")
    assert (rig.label[order[:-1]] <= rig.label[order[1:]]).all()
    rig.check(order, "sorted by class")


def test_permuted(rig):
    _census(rig)
    rig.check(np.random.default_rng(12).permutation(len(rig.label)), "permuted")


@pytest.mark.parametrize("lane", [0, 31, 63])
def test_slow_record_among_general_lanes(rig, lane):
    """Every record that takes a slow sequence behind a wave ballot, alone among 63 general-position records."""
    got = _census(rig)
    slow = sk.records_of(rig.fx, *sk.SLOW)
    assert len(slow) == sum(got[k] for k in sk.SLOW) and len(slow) >= 30
    general = sk.records_of(rig.fx, "general")
    g = np.random.default_rng(100 + lane)
    waves = []
    for s in slow:
        w = g.choice(general, 64, replace=False)
        w[lane] = s
        waves.append(w)
    idx = np.concatenate(waves)
    assert len(idx) == 64 * len(slow) and (idx[lane::64] == slow).all()
    rig.check(idx, f"slow records as lane {lane}")


def test_single_records(rig):
    _census(rig)
    for k in sk.CLASSES:
        for i in sk.records_of(rig.fx, k)[:2]:
            rig.check(np.array([i]), f"{k}, record {i} alone")


# ------------------------------------------------------------------------------------------ c. path_advance
@pytest.mark.parametrize("indirect", [False, True])
def test_path_advance(rig, indirect):
    import torch
    import crt_amd
    _census(rig)
    fx = rig.fx
    W, H = 64, 16
    n, n_pix = len(fx["rec"]), W * H
    assert n <= n_pix
    r = crt_amd.Renderer(W, H)
    r.set_camera(crt_amd.camera(1))
    idx = np.arange(n)
    dev = "cuda:0"
    for m in LIMITS:
        rays, hits, pth, rng, lin = sk.batch(fx, idx, rig.base, m)
        rng_all = np.zeros((n_pix, 6), U32)
        lin_all = np.zeros((n_pix, 3), F32)
        rng_all[:n], lin_all[:n] = rng, lin
        t_rng = torch.from_numpy(rng_all.view(np.int32)).to(dev)
        t_lin = torch.from_numpy(lin_all).to(dev)
        count_in = torch.tensor([n], dtype=torch.int32, device=dev) if indirect else None
        rays_out, pth_out, count = rig.scene.path_advance(
            r, torch.from_numpy(rays).to(dev), torch.from_numpy(hits).to(dev), torch.from_numpy(pth).to(dev), m, None,
            rng=t_rng, linear=t_lin, count_in=count_in)
        torch.cuda.synchronize()
        w_rays, w_pth, w_rng, w_lin = sk.expected(fx, idx, rig.base, m)
        ran = pth[:, paths.PATH_STATUS] == _lib.PATH_ACTIVE
        alive = np.nonzero(ran & (w_pth[:, paths.PATH_STATUS] == _lib.PATH_ACTIVE))[0]
        k = int(count.item())
        assert k == len(alive), (m, k, len(alive))
        g_rays, g_pth = rays_out.cpu().numpy()[:k], pth_out.cpu().numpy()[:k]
        pix = g_pth[:, paths.PATH_PIXEL]
        assert np.array_equal(np.sort(pix), alive), "the appended rows name the survivors' pixels, each once"
        assert np.array_equal(sk.canon(g_rays), sk.canon(w_rays[pix])), m
        assert np.array_equal(sk.canon(g_pth), sk.canon(w_pth[pix])), m
        # the sums and the RNG are path_step's; the pixels beyond the batch are untouched
        g_rng, g_lin = t_rng.cpu().numpy().view(U32), t_lin.cpu().numpy()
        assert np.array_equal(g_rng[:n], w_rng) and not g_rng[n:].any(), m
        assert np.array_equal(sk.canon(g_lin[:n]), sk.canon(w_lin)) and not g_lin[n:].any(), m
    r.close()


# ------------------------------------------------------------------------------------------ d. the render kernels' twin
def _shade(rec):
    rec = np.ascontiguousarray(rec, U32)
    out = np.zeros((len(rec), 20), U32)
    crt_check(_lib.require("crt_selftest_shade")(rec.ctypes.data_as(C.c_void_p), len(rec), out.ctypes.data_as(C.c_void_p)))
    return out


def crt_check(rc):
    import crt_amd
    crt_amd.check(rc, "crt_selftest_shade")


@pytest.mark.parametrize("arrangement", ["sorted", "permuted"])
def test_shade_rec_and_next_ray(rig, arrangement):
    """shade_rec() takes the face from dot(d, normal) < 0, not from the record: the records whose stored flag says
    otherwise (the contradicting-flag class and a NaN normal) are not comparable and left out, nothing else is."""
    _census(rig)
    fx = rig.fx
    n = len(fx["rec"])
    order = (np.argsort(rig.label, kind="stable") if arrangement == "sorted"
             else np.random.default_rng(13).permutation(n))
    hit = ~(fx["rec"][order, sk.T].view(F32) < 0)
    same_face = (sk.geometric_front(fx, order) == (fx["rec"][order, sk.FRONT] != 0)) | ~hit
    left_out = set(rig.label[order[~same_face]].tolist())
    assert left_out <= {b"misc_front_flip", b"glass_nan_normal"} and (~same_face).sum() <= 10, left_out
    idx = order[same_face]
    got = _shade(sk.shade_records(fx, idx))
    want = fx["out"][idx, 1]
    bad = np.nonzero((sk.canon(got) != sk.canon(want)).any(1))[0]
    assert not len(bad), (f"{len(bad)} records differ from the oracle's stage B: "
                          + ", ".join(f"{idx[j]} ({rig.label[idx[j]].decode()})" for j in bad[:12]))
