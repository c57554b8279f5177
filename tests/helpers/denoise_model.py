"""numpy model of the edge-avoiding a-trous filter (include/crt_hip.h "denoiser"), operation for operation
in float32, so the GPU's frames are compared bit for bit.  No GPU, no library.

Every numpy expression below is one IEEE-754 float32 operation per element (add, subtract, multiply, divide, rint): numpy
rounds each correctly and contracts nothing, which is what the build's flags make the kernels do.
"""
import numpy as np

F32 = np.float32
MISS_KEY = 0x7fffffff
H5 = (F32(0.0625), F32(0.25), F32(0.375), F32(0.25), F32(0.0625))
INF = float("inf")

LOG2E = F32(float.fromhex("0x1.715476p+0"))
LN2_HI = F32(0.693359375)
LN2_LO = F32(float.fromhex("-0x1.bd0106p-13"))
C6, C5 = F32(float.fromhex("0x1.6c16c2p-10")), F32(float.fromhex("0x1.111112p-7"))
C4, C3 = F32(float.fromhex("0x1.555556p-5")), F32(float.fromhex("0x1.555556p-3"))


def canon(a):
    """uint32 view with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a, F32)
    out = a.view(np.uint32).copy()
    out[np.isnan(a)] = 0x7fc00000
    return out


def exp_neg(x):
    """exp(-x) for float32 x in [0, 80): the header's steps.  Entries outside that range give garbage; callers mask."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        k = np.rint(x * LOG2E).astype(F32)
        r = ((x - k * LN2_HI).astype(F32) - (k * LN2_LO).astype(F32)).astype(F32)
        t = (-r).astype(F32)
        p = (C6 * t + C5).astype(F32)
        for c in (C4, C3, F32(0.5), F32(1), F32(1)):
            p = ((p * t).astype(F32) + c).astype(F32)
        ki = np.where(np.isfinite(k), k, 0).astype(np.int32)
        return (p.view(np.int32) - (ki << 23)).astype(np.int32).view(F32)


def dist2(a, b):
    with np.errstate(all="ignore"):
        d = (a - b).astype(F32)
        sq = (d * d).astype(F32)
        return ((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32)


def inverse_sigmas(sigma_color, sigma_normal, sigma_position):
    """(inv_c of iteration 0, inv_n, inv_x); None for a term that is off."""
    out = []
    for s in (sigma_color, sigma_normal, sigma_position):
        s = F32(s)
        out.append(None if s == INF else F32(F32(1) / F32(s * s)))
    return out


def tap_walk(c, v, normal, position, key, stride, colour_term, inv_n, inv_x):
    """The tap loop of both filters: (c_i [H, W, 3], v_i [H, W] or None) -> (c_{i+1}, v_{i+1} or None).  normal, position
    [H, W, 3] float32, key [H, W] int32.  colour_term(at) is the colour (or luminance) term [H, W] of one tap, at(a)
    being `a` at that tap; None: the term is off.  v is accumulated beside the colours with the squared weights."""
    h, w, _ = c.shape
    acc = np.zeros((h, w, 3), F32)
    av = None if v is None else np.zeros((h, w), F32)
    sw = np.zeros((h, w), F32)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = F32(H5[dy + 2] * H5[dx + 2])
                if dy == 0 and dx == 0:
                    acc = (acc + (k * c).astype(F32)).astype(F32)
                    if v is not None:
                        av = (av + (F32(k * k) * v).astype(F32)).astype(F32)
                    sw = (sw + k).astype(F32)
                    continue
                qy, qx = ys + dy * stride, xs + dx * stride
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)

                def at(a):                                # a at the tap; where the tap is outside, anything (masked)
                    return a[qy, qx]

                take = inside & (at(key) == key)
                zero = np.zeros((h, w), F32)
                xc = zero if colour_term is None else colour_term(at)
                xn = zero if inv_n is None else (dist2(normal, at(normal)) * inv_n).astype(F32)
                xx = zero if inv_x is None else (dist2(position, at(position)) * inv_x).astype(F32)
                X = ((xc + xn).astype(F32) + xx).astype(F32)
                take &= X < F32(80)                       # a NaN compares false: skipped
                kw = (k * exp_neg(np.where(take, X, F32(0)))).astype(F32)
                acc = np.where(take[..., None], (acc + (kw[..., None] * at(c)).astype(F32)).astype(F32), acc)
                if v is not None:
                    av = np.where(take, (av + ((kw * kw).astype(F32) * at(v)).astype(F32)).astype(F32), av)
                sw = np.where(take, (sw + kw).astype(F32), sw)
        return (acc / sw[..., None]).astype(F32), None if v is None else (av / (sw * sw).astype(F32)).astype(F32)


def iteration(c, normal, position, key, stride, inv_c, inv_n, inv_x):
    """c_i [H, W, 3] -> c_{i+1}."""
    term = None if inv_c is None else lambda at: (dist2(c, at(c)) * inv_c).astype(F32)
    return tap_walk(c, None, normal, position, key, stride, term, inv_n, inv_x)[0]


def split_guides(guides):
    g = np.ascontiguousarray(guides, F32)
    return g[..., 0:3], g[..., 4:7], g.view(np.int32)[..., 7]


def denoise_steps(color, guides, sigma_color, sigma_normal, sigma_position, steps):
    """{n: the filter's result after n iterations} for every n in steps (the first n iterations of a longer run are the
    run of n iterations)."""
    c = np.ascontiguousarray(color, F32)
    normal, position, key = split_guides(guides)
    inv_c, inv_n, inv_x = inverse_sigmas(sigma_color, sigma_normal, sigma_position)
    out = {}
    for i in range(max(steps)):
        c = iteration(c, normal, position, key, 1 << i, inv_c, inv_n, inv_x)
        if inv_c is not None:
            inv_c = F32(inv_c * F32(4))
        if i + 1 in steps:
            out[i + 1] = c
    return out


def denoise(color, guides, sigma_color, sigma_normal, sigma_position, iterations=5):
    """The whole filter: color [H, W, 3] = c_0, guides [H, W, 8] as Renderer.guides() returns them."""
    return denoise_steps(color, guides, sigma_color, sigma_normal, sigma_position, (iterations,))[iterations]


def pack_guides(normal, t, position, key):
    """[H, W, 8] float32 records from their parts (key int32; a miss is the caller's to fill)."""
    h, w = key.shape
    g = np.zeros((h, w, 8), F32)
    g[..., 0:3], g[..., 3], g[..., 4:7] = normal, t, position
    g.view(np.int32)[..., 7] = key
    return g


def miss_record():
    g = np.zeros(8, F32)
    g[3] = -1
    g.view(np.int32)[7] = MISS_KEY
    return g


def centre_rays(cam, w, h):
    """RayQuery::centreRays in float32: cam = the 20 camera floats (origin, lower_left, horizontal, vertical, ...).
    Returns (origins [h*w, 3], directions [h*w, 3])."""
    cam = np.asarray(cam, F32)
    o, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    u = ((np.arange(w, dtype=F32) + F32(0.5)) / F32(w)).astype(F32)
    v = ((np.arange(h, dtype=F32) + F32(0.5)) / F32(h)).astype(F32)
    uu, vv = np.broadcast_to(u[None, :, None], (h, w, 1)), np.broadcast_to(v[:, None, None], (h, w, 1))
    d = ((ll + (uu * hor).astype(F32)).astype(F32) + (vv * ver).astype(F32)).astype(F32)
    d = (d - o).astype(F32)
    return np.broadcast_to(o, (h * w, 3)).copy(), d.reshape(-1, 3)
