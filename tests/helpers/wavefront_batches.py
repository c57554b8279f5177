"""Helpers of tests/test_gpu_wavefront.py: traced batches on the host, the advance call and its composition out of the
path steps (Scene.path_step, then crt_amd.camera_rays on the ended pixels that have samples left, then compaction
with torch indexing), both as rows keyed by pixel, since the order of an advance's output is not part of its interface."""
import numpy as np

import crt_amd
from crt_amd import _lib, paths

import custom_scene
import synth_scenes as synth

F32 = np.float32
W, H = 64, 36
INVALID = 5          # the step kernels' code of a material index outside the scene's materials


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def renderer(cam, w=W, h=H, seed=41):
    r = crt_amd.Renderer(w, h)
    r.set_camera(cam)
    r.init_rand(seed)
    return r


def odd_materials_world(scenes):
    """40 spheres cycling through the five sphere materials, one whose material index is outside the scene's materials,
    one of an unknown material type and one of metal with fuzz 1 (absorbs many of its hits), in the Cornell box."""
    k = len(synth.SPHERE_MATS)
    spheres = synth.random_spheres(40) + [((0.1, -0.1, 0.1), 0.06, 99), ((-0.1, -0.12, 0.12), 0.06, k),
                                          ((0.0, 0.12, 0.1), 0.06, k + 1)]
    mats = synth.SPHERE_MATS + [custom_scene.mat_row(7, (0.3, 0.3, 0.3), (2, 2, 2)),
                                custom_scene.mat_row(1, (0.9, 0.9, 0.9), roughness=1.0)]
    return custom_scene.CustomScene(scenes["cornell"], spheres, mats)


def keyed(rays, pth, count):
    """Rows [0, count) of an output batch as uint32 [count, 16], sorted by pixel; no pixel twice."""
    rows = np.concatenate([bits(rays[:count]), bits(pth[:count])], axis=1)
    pix = rows[:, 8 + paths.PATH_PIXEL]
    assert len(np.unique(pix)) == count, "a pixel appears twice in the output batch"
    return rows[np.argsort(pix, kind="stable")]


class TracedBatch:
    """One traced batch of a wavefront and everything an advance of it reads, on the host and read-only."""

    def __init__(self, scene, rows, r, rays, hits, pth, rng, lin):
        self.scene, self.rows, self.r = scene, rows, r
        self.rays, self.hits, self.pth, self.rng, self.lin = rays, hits, pth, rng, lin
        self.n_pix = len(rng)
        for a in (rays, hits, pth, rng, lin):
            a.setflags(write=False)

    def _device(self, idx, pth, remaining):
        import torch
        dev = "cuda:0"
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)   # noqa: E731
        return (t(self.rays[idx]), t(self.hits[idx]), t((self.pth if pth is None else pth)[idx]),
                t(self.rng.view(np.int32)), t(self.lin), None if remaining is None else t(remaining.astype(np.int32)))

    @staticmethod
    def _result(rays_out, pth_out, count, rng, lin, remaining):
        import torch
        torch.cuda.synchronize()
        return {"rows": keyed(rays_out.cpu().numpy(), pth_out.cpu().numpy(), count), "count": count,
                "rng": rng.cpu().numpy().view(np.uint32), "lin": lin.cpu().numpy(),
                "remaining": None if remaining is None else remaining.cpu().numpy()}

    def advance(self, idx, remaining, pth=None, out=None):
        """paths.advance over entries idx (in that order) on copies of the state."""
        rays, hits, p, rng, lin, rem = self._device(idx, pth, remaining)
        rays_out, pth_out, count = self.scene.path_advance(self.r, rays, hits, p, 20, rem, rng=rng, linear=lin, out=out)
        assert count.dtype.is_floating_point is False and count.shape == (1,) and count.is_cuda
        res = self._result(rays_out, pth_out, int(count), rng, lin, rem)
        # the inputs are read only
        assert same(rays.cpu().numpy(), self.rays[idx]) and same(hits.cpu().numpy(), self.hits[idx])
        assert same(p.cpu().numpy(), (self.pth if pth is None else pth)[idx])
        return res

    def composed(self, idx, remaining, pth=None):
        """The same out of the parent's functions: path_step, camera_rays on the ended pixels with samples left,
        compaction with torch indexing."""
        import torch
        rays, hits, p, rng, lin, rem = self._device(idx, pth, remaining)
        before = p.clone()
        self.scene.path_step(rays, hits, p, 20, rng, lin)
        pix = before[:, paths.PATH_PIXEL].long()
        valid = (before[:, paths.PATH_STATUS] == _lib.PATH_ACTIVE) & (pix >= 0) & (pix < self.n_pix)
        ended = valid & (p[:, paths.PATH_STATUS] == _lib.PATH_ENDED)
        keep = valid & ~ended
        rays_out, pth_out = rays[keep], p[keep]
        if rem is not None:
            again = ended.clone()
            again[ended] = rem[pix[ended]] > 0
            sel = again.nonzero().squeeze(1)
            if sel.numel():
                new_pix = before[sel, paths.PATH_PIXEL].contiguous()
                rem[new_pix.long()] -= 1
                new_rays, new_pth = crt_amd.camera_rays(self.r, new_pix, rng=rng)
                rays_out, pth_out = torch.cat([rays_out, new_rays]), torch.cat([pth_out, new_pth])
        return self._result(rays_out, pth_out, rays_out.shape[0], rng, lin, rem)

    def code(self):
        """Per entry: the step kernels' material code, -1 for a miss."""
        mat = self.hits[:, 3].view(np.int32)
        codes = self.rows[:, 0, 0].view(np.int32)
        ok = (mat >= 0) & (mat < len(codes))
        c = np.where(ok, codes[np.clip(mat, 0, len(codes) - 1)], INVALID)
        return np.where(self.hits[:, 0] < 0, -1, c)

    def classes(self):
        """Masks of the kinds of entry, from a plain step of the whole batch."""
        import torch
        rays, hits, p, rng, lin, _ = self._device(np.arange(len(self.rays)), None, None)
        self.scene.path_step(rays, hits, p, 20, rng, lin)
        torch.cuda.synchronize()
        after = p.cpu().numpy()
        code = self.code()
        front = self.hits[:, 7].view(np.int32) != 0
        ended = after[:, paths.PATH_STATUS] == _lib.PATH_ENDED
        same_bounce = after[:, paths.PATH_BOUNCE] == self.pth[:, paths.PATH_BOUNCE]
        return {"miss": code == -1, "lambertian": code == 0, "metal": code == 1, "glass": code == 2, "light": code == 3,
                "unknown type": code == 4, "invalid index": code == INVALID, "glass from inside": (code == 2) & ~front,
                "metal absorbed": (code == 1) & ended & same_bounce, "goes on": ~ended, "ends": ended}


def traced_batch(cs, every_class, rounds=24):
    """The wavefront of world `cs` at 64x36, one path per pixel with regeneration (2,304 entries in every iteration): the
    first batch of its first `rounds` iterations that holds every class of entry (every_class), else the fourth."""
    scene = cs.upload(0)
    rows = paths.shade_rows(cs.desc)
    r = renderer(crt_amd.camera(64))
    r.write_linear(np.zeros((H, W, 3), F32))
    rays, pth = crt_amd.camera_rays(r)
    seen = {}
    for it in range(rounds):
        hits = scene.trace(rays)["f32"]
        r.synchronize()
        b = TracedBatch(scene, rows, r, rays.cpu().numpy(), hits.cpu().numpy(), pth.cpu().numpy(),
                        r.rng_state().reshape(-1, 6), r.linear().reshape(-1, 3))
        assert len(b.rays) == W * H and len(np.unique(b.pth[:, paths.PATH_PIXEL])) == W * H
        b.cls = b.classes()
        seen = {k: int(v.sum()) for k, v in b.cls.items()}
        if all(seen.values()) if every_class else it == 3:
            print(f"\nbatch of iteration {it}: {seen}")
            return b
        scene.path_step(rays, hits, pth, 20, r, r)
        ended = (pth[:, paths.PATH_STATUS] == _lib.PATH_ENDED).nonzero().squeeze(1)
        if ended.numel():                       # every ended path's pixel starts its next sample
            rays[ended], pth[ended] = crt_amd.camera_rays(r, pth[ended, paths.PATH_PIXEL].contiguous())
    raise AssertionError(f"no batch with every class of entry in {rounds} iterations; the last one: {seen}")


def assert_equal_results(got, want, what):
    assert got["count"] == want["count"], (what, got["count"], want["count"])
    for k in ("rows", "rng", "lin", "remaining"):
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert same(got[k], want[k]), f"{what}: {k} differs in {int((bits(got[k]) != bits(want[k])).sum())} words"
