"""numpy model of the reprojection (include/crt_hip.h "reprojection"), operation for operation in float32,
so the GPU's histories are compared bit for bit.  No GPU, no library.

As in denoise_model.py, every numpy expression below is one IEEE-754 float32 operation per element.
"""
import numpy as np

from denoise_model import F32, MISS_KEY, canon, centre_rays, dist2, pack_guides, split_guides  # noqa: F401

INF = float("inf")
ONE, HALF = F32(1), F32(0.5)
LR, LG, LB = F32(0.2126), F32(0.7152), F32(0.0722)


def dot(a, b):
    """(a.x * b.x + a.y * b.y) + a.z * b.z over the last axis."""
    with np.errstate(all="ignore"):
        p = (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32)
        return ((p[..., 0] + p[..., 1]).astype(F32) + p[..., 2]).astype(F32)


def host_constants(cam, position_tolerance):
    """What the host forms once per call from the previous guide camera (its floats: origin, lower_left, horizontal,
    vertical first): (o, L, N, hor, ver, LN, hh, vv, tol2); tol2 None with the position term off."""
    cam = np.asarray(cam, F32)
    o, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    with np.errstate(all="ignore"):
        L = (ll - o).astype(F32)
        N = np.zeros(3, F32)
        for a in range(3):
            b, d = (a + 1) % 3, (a + 2) % 3
            N[a] = F32(F32(hor[b] * ver[d]) - F32(hor[d] * ver[b]))
        tol = F32(position_tolerance)
        tol2 = None if tol == INF else F32(tol * tol)
        return o, L, N, hor, ver, dot(L, N), dot(hor, hor), dot(ver, ver), tol2


def scaled(sums, scale):
    """c = scale * sum per channel."""
    with np.errstate(all="ignore"):
        return (F32(scale) * np.ascontiguousarray(sums, F32)).astype(F32)


def project(pos, cam, w, h):
    """(s, fx, fy) of the positions [..., 3] in the camera `cam` over a w x h frame."""
    o, L, N, hor, ver, LN, hh, vv, _ = host_constants(cam, INF)
    with np.errstate(all="ignore"):
        d = (np.asarray(pos, F32) - o).astype(F32)
        s = (LN / dot(d, N)).astype(F32)
        q = ((s[..., None] * d).astype(F32) - L).astype(F32)
        u = (dot(q, hor) / hh).astype(F32)
        v = (dot(q, ver) / vv).astype(F32)
        fx = ((u * F32(w)).astype(F32) - HALF).astype(F32)
        fy = ((v * F32(h)).astype(F32) - HALF).astype(F32)
    return s, fx, fy


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


def reproject(c, guides, prev_guides, prev_history, prev_cam, position_tolerance, normal_min, max_history,
              prev_moments=None):
    """One call.  c [H, W, 3] = scale * sum; guides, prev_guides [H, W, 8]; prev_history [H, W, 4] or None (the state is
    not valid).  Returns (history [H, W, 4], taken [H, W] bool: the pixels with sw > 0).  With prev_moments [H, W, 2]
    (crt_renderer_reproject_moments: they take the history's taps, weights, sum and blend factor) it returns
    (history, moments [H, W, 2], taken)."""
    c = np.ascontiguousarray(c, F32)
    h, w, _ = c.shape
    out = np.concatenate([c, np.ones((h, w, 1), F32)], axis=-1)
    taken = np.zeros((h, w), bool)
    if prev_history is None:
        return out, taken
    ph = np.ascontiguousarray(prev_history, F32)
    pm = None if prev_moments is None else np.ascontiguousarray(prev_moments, F32)
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
        fx, fy = np.where(cand, fx, F32(0)), np.where(cand, fy, F32(0))
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
                row = ph[ty, tx]
                ok &= np.isfinite(row[..., 0:3]).all(axis=-1)
                acc = np.where(ok[..., None], (acc + (wgt[..., None] * row).astype(F32)).astype(F32), acc)
                if pm is not None:
                    am = np.where(ok[..., None], (am + (wgt[..., None] * pm[ty, tx]).astype(F32)).astype(F32), am)
                sw = np.where(ok, (sw + wgt).astype(F32), sw)
        taken = sw > 0
        div = np.where(taken, sw, ONE)[..., None]
        hist = (acc / div).astype(F32)
        m = np.fmin((hist[..., 3] + ONE).astype(F32), cap).astype(F32)
        a = (ONE / m).astype(F32)
        col = (hist[..., 0:3] + ((c - hist[..., 0:3]).astype(F32) * a[..., None]).astype(F32)).astype(F32)
        blended = np.concatenate([col, m[..., None]], axis=-1)
        out = np.where(taken[..., None], blended, out).astype(F32)
        if pm is not None:
            new_m, hm = frame_moments(c), (am / div).astype(F32)
            mom = (hm + ((new_m - hm).astype(F32) * a[..., None]).astype(F32)).astype(F32)
            return out, np.where(taken[..., None], mom, new_m).astype(F32), taken
    return out, taken


def camera_guides(cam, w, h, t, normal, key):
    """Guides of a frame whose pixel-centre rays (centre_rays of `cam`) hit at parameters t [h, w] (t < 0: a miss):
    position = o + t * d as the pack kernel forms it."""
    ro, rd = centre_rays(cam, w, h)
    t = np.asarray(t, F32)
    with np.errstate(all="ignore"):
        pos = (ro + (t.reshape(-1, 1) * rd).astype(F32)).astype(F32).reshape(h, w, 3)
    hit = t >= 0
    key = np.where(hit, key, MISS_KEY).astype(np.int32)
    pos = np.where(hit[..., None], pos, F32(0))
    nrm = np.where(hit[..., None], np.broadcast_to(np.asarray(normal, F32), (h, w, 3)), F32(0))
    return pack_guides(nrm, np.where(hit, t, F32(-1)), pos, key)
