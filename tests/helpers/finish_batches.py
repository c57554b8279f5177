"""Helpers of tests/test_gpu_path_finish.py: a batch of paths brought to its end in two ways on copies of one state, by
the loop of Scene.trace and paths.advance that runs until the count is 0, and by one paths.finish call."""
import numpy as np

import stream_gate
import wavefront_batches as wb
from crt_amd import _lib, paths

BOUNCES = 20


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def remaining(pattern, n_pix):
    """The per-pixel sample counts of a named pattern; None for "never regenerate"."""
    if pattern == "none":
        return None
    if pattern == "alternating":
        return np.where(np.arange(n_pix) % 2 == 0, 0, 2).astype(np.int32)
    return np.full(n_pix, {"zero": 0, "three": 3}[pattern], np.int32)


class State:
    """Copies of a traced batch's rays, paths and per-pixel state on the device."""

    def __init__(self, b, rays, pth, rem):
        self.rays, self.pth = dev(rays), dev(pth)
        self.rng, self.lin = dev(b.rng.view(np.int32)), dev(b.lin)
        self.rem = None if rem is None else dev(rem.astype(np.int32))

    def result(self, **more):
        import torch
        torch.cuda.synchronize()
        return dict(rng=self.rng.cpu().numpy().view(np.uint32), lin=self.lin.cpu().numpy(),
                    remaining=None if self.rem is None else self.rem.cpu().numpy(), **more)


def active(pth, n_pix):
    """The entries a step does anything for."""
    pix = pth[:, paths.PATH_PIXEL]
    return (pth[:, paths.PATH_STATUS] == _lib.PATH_ACTIVE) & (pix >= 0) & (pix < n_pix)


def loop(b, scene, rays, pth, rem, max_bounces=BOUNCES, **opts):
    """Scene.trace and paths.advance until no entry is left.  rays: the sum of the batch sizes without the first
    batch's entries that are not active (the query traces those too; nothing else reads their records)."""
    s = State(b, rays, pth, rem)
    r, p, m = s.rays, s.pth, len(rays)
    sizes = []
    while m:
        sizes.append(m)
        hits = scene.trace(r[:m], **opts)["f32"]
        r, p, count = scene.path_advance(b.r, r[:m], hits, p[:m], max_bounces, s.rem, rng=s.rng, linear=s.lin)
        m = int(count)
    idle = int((~active(np.ascontiguousarray(pth).view(np.int32), b.n_pix)).sum())
    return s.result(rays=sum(sizes) - idle, rounds=len(sizes))


def finish(b, scene, rays, pth, rem, count=None, totals=(0, 0), max_bounces=BOUNCES, stream_count=False):
    """One paths.finish.  count: the value of count_in as an int32 (None: no count_in); stream_count: the count is produced by a
    kernel on a side stream just before the call, which then runs on that stream; the stream is held back first
    (stream_gate), and the batch is copied on it behind the gate."""
    import torch
    s = State(b, rays, pth, rem)
    t = torch.tensor(list(totals), dtype=torch.int64, device="cuda:0")
    if stream_count:
        side = stream_gate.side_stream()
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            stream_gate.gate(side)
            s.rays, s.pth = s.rays.clone(), s.pth.clone()
            c = torch.zeros((1,), dtype=torch.int32, device="cuda:0") + count
            res = scene.path_finish(b.r, s.rays, s.pth, max_bounces, s.rem, rng=s.rng, linear=s.lin, count_in=c, totals=t)
        side.synchronize()
    else:
        c = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda:0")
        res = scene.path_finish(b.r, s.rays, s.pth, max_bounces, s.rem, rng=s.rng, linear=s.lin, count_in=c, totals=t)
    assert res is None
    out = s.result(totals=t.tolist())
    # the inputs are read only
    assert wb.same(s.rays.cpu().numpy(), np.ascontiguousarray(rays)) and wb.same(s.pth.cpu().numpy(), np.ascontiguousarray(pth))
    if c is not None:
        assert int(c) == count
    return out


def assert_same_state(got, want, what):
    for k in ("rng", "lin", "remaining"):
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert wb.same(got[k], want[k]), f"{what}: {k} differs in {int((wb.bits(got[k]) != wb.bits(want[k])).sum())} words"


def assert_others_untouched(b, got, rem, touched, what):
    """Every pixel outside `touched` keeps its RNG state, its sum and its remaining samples."""
    other = np.ones(b.n_pix, bool)
    other[touched] = False
    assert wb.same(got["rng"][other], b.rng[other]) and wb.same(got["lin"][other], b.lin[other]), what
    if rem is not None:
        assert np.array_equal(got["remaining"][other], rem[other]), what
