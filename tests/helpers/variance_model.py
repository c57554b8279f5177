"""numpy model of the variance-guided filtering of the history (include/crt_hip.h "variance-guided filtering", DESIGN.md
§24), operation for operation in float32, so the GPU's moments, variances and frames are compared bit for bit.  No GPU, no
library.

As in denoise_model.py, every numpy expression below is one IEEE-754 float32 operation per element (numpy's float32
sqrt is correctly rounded, as the build's is).
"""
import numpy as np

from denoise_model import F32, H5, MISS_KEY, canon, dist2, exp_neg, split_guides  # noqa: F401
from reproject_model import dot, host_constants, project
import reproject_model as rm

INF = float("inf")
ONE, ZERO = F32(1), F32(0)
LR, LG, LB = F32(0.2126), F32(0.7152), F32(0.0722)
HG = (F32(0.25), F32(0.5), F32(0.25))
EPS_DEN = F32(2.0 ** -20)


def lum(c):
    """(0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z over the last axis."""
    c = np.asarray(c, F32)
    with np.errstate(all="ignore"):
        a = ((LR * c[..., 0]).astype(F32) + (LG * c[..., 1]).astype(F32)).astype(F32)
        return (a + (LB * c[..., 2]).astype(F32)).astype(F32)


def frame_moments(c):
    """(l, l * l) of a frame [H, W, 3]."""
    with np.errstate(all="ignore"):
        l = lum(c)
        return np.stack([l, (l * l).astype(F32)], axis=-1)


def reproject_moments(c, guides, prev_guides, prev_history, prev_moments, prev_cam, position_tolerance, normal_min,
                      max_history):
    """One crt_renderer_reproject_moments.  As reproject_model.reproject, with prev_moments [H, W, 2] (None together with
    prev_history: the state is not valid).  Returns (history [H, W, 4], moments [H, W, 2], taken [H, W])."""
    c = np.ascontiguousarray(c, F32)
    h, w, _ = c.shape
    new_m = frame_moments(c)
    out = np.concatenate([c, np.ones((h, w, 1), F32)], axis=-1)
    taken = np.zeros((h, w), bool)
    if prev_history is None:
        return out, new_m, taken
    ph = np.ascontiguousarray(prev_history, F32)
    pm = np.ascontiguousarray(prev_moments, F32)
    n, pos, key = split_guides(guides)
    pn, ppos, pkey = split_guides(prev_guides)
    o, L, N, hor, ver, LN, hh, vv, tol2 = host_constants(prev_cam, position_tolerance)
    nmin = F32(normal_min)
    on_n = nmin != -INF
    cap = F32(max_history)
    with np.errstate(all="ignore"):
        cand = (key != MISS_KEY) & np.isfinite(c).all(axis=-1)
        s, fx, fy = project(pos, prev_cam, w, h)
        cand &= (s > 0) & (fx > F32(-1)) & (fx < F32(w)) & (fy > F32(-1)) & (fy < F32(h))     # a NaN fails
        fx, fy = np.where(cand, fx, ZERO), np.where(cand, fy, ZERO)
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = (fx - x0f).astype(F32), (fy - y0f).astype(F32)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        if tol2 is not None:
            d = (pos - o).astype(F32)
            lim = (tol2 * dot(d, d)).astype(F32)
        acc = np.zeros((h, w, 4), F32)
        am = np.zeros((h, w, 2), F32)
        sw = np.zeros((h, w), F32)
        for j in (0, 1):
            for i in (0, 1):
                wx = ax if i else (ONE - ax).astype(F32)
                wy = ay if j else (ONE - ay).astype(F32)
                wgt = (wx * wy).astype(F32)
                tx, ty = x0 + i, y0 + j
                ok = cand & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h) & (wgt > 0)
                tx, ty = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
                ok &= pkey[ty, tx] == key
                if tol2 is not None:
                    ok &= dist2(pos, ppos[ty, tx]) <= lim
                if on_n:
                    ok &= dot(n, pn[ty, tx]) >= nmin
                row, mrow = ph[ty, tx], pm[ty, tx]
                ok &= np.isfinite(row[..., 0:3]).all(axis=-1)
                acc = np.where(ok[..., None], (acc + (wgt[..., None] * row).astype(F32)).astype(F32), acc)
                am = np.where(ok[..., None], (am + (wgt[..., None] * mrow).astype(F32)).astype(F32), am)
                sw = np.where(ok, (sw + wgt).astype(F32), sw)
        taken = sw > 0
        div = np.where(taken, sw, ONE)[..., None]
        hist = (acc / div).astype(F32)
        m = np.fmin((hist[..., 3] + ONE).astype(F32), cap).astype(F32)
        a = (ONE / m).astype(F32)
        col = (hist[..., 0:3] + ((c - hist[..., 0:3]).astype(F32) * a[..., None]).astype(F32)).astype(F32)
        hm = (am / div).astype(F32)
        mom = (hm + ((new_m - hm).astype(F32) * a[..., None]).astype(F32)).astype(F32)
        out = np.where(taken[..., None], np.concatenate([col, m[..., None]], axis=-1), out).astype(F32)
        mom = np.where(taken[..., None], mom, new_m).astype(F32)
    return out, mom, taken


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
    h, w, _ = c.shape
    acc = np.zeros((h, w, 3), F32)
    av = np.zeros((h, w), F32)
    sw = np.zeros((h, w), F32)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        if sigma_l is not None:
            g = prefilter(v, key)
            den = ((F32(sigma_l) * np.sqrt(g).astype(F32)).astype(F32) + EPS_DEN).astype(F32)
            inv_den = (ONE / den).astype(F32)
        lc = lum(c)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = F32(H5[dy + 2] * H5[dx + 2])
                if dy == 0 and dx == 0:
                    acc = (acc + (k * c).astype(F32)).astype(F32)
                    av = (av + (F32(k * k) * v).astype(F32)).astype(F32)
                    sw = (sw + k).astype(F32)
                    continue
                qy, qx = ys + dy * stride, xs + dx * stride
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)

                def at(a):                                # a at the tap; where the tap is outside, anything (masked)
                    return np.roll(a, (-dy * stride, -dx * stride), axis=(0, 1))

                qc, qv = at(c), at(v)
                take = inside & (at(key) == key)
                zero = np.zeros((h, w), F32)
                xc = zero if sigma_l is None else (np.abs((lc - at(lc)).astype(F32)) * inv_den).astype(F32)   # lum(qc)
                xn = zero if inv_n is None else (dist2(normal, at(normal)) * inv_n).astype(F32)
                xx = zero if inv_x is None else (dist2(position, at(position)) * inv_x).astype(F32)
                X = ((xc + xn).astype(F32) + xx).astype(F32)
                take &= X < F32(80)                       # a NaN compares false: skipped
                kw = (k * exp_neg(np.where(take, X, ZERO))).astype(F32)
                acc = np.where(take[..., None], (acc + (kw[..., None] * qc).astype(F32)).astype(F32), acc)
                av = np.where(take, (av + ((kw * kw).astype(F32) * qv).astype(F32)).astype(F32), av)
                sw = np.where(take, (sw + kw).astype(F32), sw)
        return (acc / sw[..., None]).astype(F32), (av / (sw * sw).astype(F32)).astype(F32)


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
