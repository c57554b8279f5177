"""numpy model of the variance-guided filtering of the history (include/crt_hip.h "variance-guided filtering", DESIGN.md
§24), operation for operation in float32, so the GPU's moments, variances and frames are compared bit for bit.  No GPU, no
library.

As in denoise_model.py, every numpy expression below is one IEEE-754 float32 operation per element (numpy's float32
sqrt is correctly rounded, as the build's is).
"""
import numpy as np

from denoise_model import F32, H5, MISS_KEY, canon, dist2, exp_neg, split_guides, tap_walk  # noqa: F401
from reproject_model import dot, frame_moments, host_constants, lum, project  # noqa: F401
import reproject_model as rm

INF = float("inf")
ONE, ZERO = F32(1), F32(0)
HG = (F32(0.25), F32(0.5), F32(0.25))
EPS_DEN = F32(2.0 ** -20)


def reproject_moments(c, guides, prev_guides, prev_history, prev_moments, prev_cam, position_tolerance, normal_min,
                      max_history):
    """One crt_renderer_reproject_moments.  As reproject_model.reproject, with prev_moments [H, W, 2] (None together with
    prev_history: the state is not valid).  Returns (history [H, W, 4], moments [H, W, 2], taken [H, W])."""
    if prev_history is None:
        out, taken = rm.reproject(c, guides, prev_guides, None, prev_cam, position_tolerance, normal_min, max_history)
        return out, frame_moments(np.ascontiguousarray(c, F32)), taken
    return rm.reproject(c, guides, prev_guides, prev_history, prev_cam, position_tolerance, normal_min, max_history,
                        prev_moments)


def estimate(history, moments, key, min_history):
    """The estimate kernel's v [H, W] from history rows [H, W, 4], moments [H, W, 2] and keys [H, W]."""
    hist = np.ascontiguousarray(history, F32)
    mom = np.ascontiguousarray(moments, F32)
    h, w, _ = hist.shape
    mh = F32(min_history)
    length = hist[..., 3]
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        v_long = np.fmax(ZERO, (mom[..., 1] - (mom[..., 0] * mom[..., 0]).astype(F32)).astype(F32)).astype(F32)
        s1, s2, n = np.zeros((h, w), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                qy, qx = ys + dy, xs + dx
                take = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                m = mom[qy, qx]
                take &= (key[qy, qx] == key) & np.isfinite(m).all(axis=-1)
                s1 = np.where(take, (s1 + m[..., 0]).astype(F32), s1)
                s2 = np.where(take, (s2 + m[..., 1]).astype(F32), s2)
                n = np.where(take, (n + ONE).astype(F32), n)
        some = n != 0
        div = np.where(some, n, ONE)
        M1, M2 = (s1 / div).astype(F32), (s2 / div).astype(F32)
        spatial = np.fmax(ZERO, (M2 - (M1 * M1).astype(F32)).astype(F32)).astype(F32)
        v_short = (spatial * (mh / length).astype(F32)).astype(F32)
        v_short = np.where(some, v_short, ZERO)
        return np.where(length >= mh, v_long, v_short).astype(F32)


def prefilter(v, key):
    """g [H, W]: the 3 x 3 Gaussian over v at +-1 pixel, same key, inside the frame."""
    h, w = v.shape
    ys, xs = np.mgrid[0:h, 0:w]
    gs, gw = np.zeros((h, w), F32), np.zeros((h, w), F32)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                kg = F32(HG[dy + 1] * HG[dx + 1])
                qy, qx = ys + dy, xs + dx
                take = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                take &= key[qy, qx] == key
                gs = np.where(take, (gs + (kg * v[qy, qx]).astype(F32)).astype(F32), gs)
                gw = np.where(take, (gw + kg).astype(F32), gw)
        return (gs / gw).astype(F32)


def iteration(c, v, normal, position, key, stride, sigma_l, inv_n, inv_x):
    """(c_i [H, W, 3], v_i [H, W]) -> (c_{i+1}, v_{i+1}).  sigma_l None: the luminance term is off."""
    term = None
    if sigma_l is not None:
        with np.errstate(all="ignore"):
            g = prefilter(v, key)
            den = ((F32(sigma_l) * np.sqrt(g).astype(F32)).astype(F32) + EPS_DEN).astype(F32)
            inv_den = (ONE / den).astype(F32)
            lc = lum(c)

        def term(at):                                     # at(lc): lum(qc)
            return (np.abs((lc - at(lc)).astype(F32)) * inv_den).astype(F32)
    return tap_walk(c, v, normal, position, key, stride, term, inv_n, inv_x)


def filter_steps(c0, v0, guides, sigma_luminance, sigma_normal, sigma_position, steps):
    """{n: (c_n, v_n)} for every n in steps, from c_0 [H, W, 3] and v_0 [H, W]."""
    c, v = np.ascontiguousarray(c0, F32), np.ascontiguousarray(v0, F32)
    normal, position, key = split_guides(guides)
    sl = None if F32(sigma_luminance) == INF else F32(sigma_luminance)
    inv = []
    for s in (sigma_normal, sigma_position):
        s = F32(s)
        inv.append(None if s == INF else F32(ONE / F32(s * s)))
    out = {}
    for i in range(max(steps)):
        c, v = iteration(c, v, normal, position, key, 1 << i, sl, inv[0], inv[1])
        if i + 1 in steps:
            out[i + 1] = (c, v)
    return out


def denoise_variance_steps(history, moments, guides, sigma_luminance, sigma_normal, sigma_position, min_history, steps):
    """The estimate, then the filter: ({n: the frame after n iterations}, the estimate's v)."""
    hist = np.ascontiguousarray(history, F32)
    _, _, key = split_guides(guides)
    v0 = estimate(hist, moments, key, min_history)
    res = filter_steps(hist[..., 0:3], v0, guides, sigma_luminance, sigma_normal, sigma_position, steps)
    return {n: cv[0] for n, cv in res.items()}, v0


def denoise_variance(history, moments, guides, sigma_luminance, sigma_normal, sigma_position, min_history, iterations=5):
    out, v0 = denoise_variance_steps(history, moments, guides, sigma_luminance, sigma_normal, sigma_position, min_history,
                                     (iterations,))
    return out[iterations], v0


class HistoryState:
    """The handle's history state and its validity rules: `valid` (a previous frame exists) and `moments_valid` (the
    moments belong to it).  reproject() is the plain entry, reproject_moments() the new one, reset() is
    crt_renderer_reset_history."""

    def __init__(self):
        self.history = self.moments = self.prev_guides = self.prev_cam = None
        self.valid = self.moments_valid = False

    def _after(self, guides, cam):
        self.prev_guides, self.prev_cam, self.valid = guides, cam, True

    def reproject(self, c, guides, cam, tol, nmin, cap):
        self.history, taken = rm.reproject(c, guides, self.prev_guides, self.history if self.valid else None,
                                           self.prev_cam, tol, nmin, cap)
        self.moments_valid = False
        self._after(guides, cam)
        return taken

    def reproject_moments(self, c, guides, cam, tol, nmin, cap):
        use = self.valid and self.moments_valid          # a history without moments starts over as a whole
        self.history, self.moments, taken = reproject_moments(
            c, guides, self.prev_guides, self.history if use else None, self.moments if use else None, self.prev_cam,
            tol, nmin, cap)
        self.moments_valid = True
        self._after(guides, cam)
        return taken

    def reset(self):
        self.valid = self.moments_valid = False
