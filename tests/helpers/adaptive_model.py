"""A numpy model of adaptive sampling's plan step and loop, f32 operation for operation.

Tiles are the render kernels' 8x8 ones: tile t covers x = (t % tiles_x) * 8 + (lane & 7), y = (t // tiles_x) * 8 +
(lane >> 3).  Arrays of per-tile values are flat, in tile order.  IEEE 754 leaves a NaN's sign and payload open and
processors differ in them, so `canon` maps every NaN to one pattern before words are compared."""
import numpy as np

F32 = np.float32
LANES = np.arange(64)


def tiles(w, h):
    """(tiles_y, tiles_x)"""
    return (h + 7) // 8, (w + 7) // 8


def in_frame(w, h):
    """In-frame pixels per tile, int64 [tiles]."""
    ty, tx = tiles(w, h)
    t = np.arange(ty * tx)
    return np.minimum(8, w - (t % tx) * 8) * np.minimum(8, h - (t // tx) * 8)


def lane_pixels(w, h):
    """(x, y, valid), each [tiles, 64]."""
    ty, tx = tiles(w, h)
    t = np.arange(ty * tx)[:, None]
    x = (t % tx) * 8 + (LANES & 7)[None]
    y = (t // tx) * 8 + (LANES >> 3)[None]
    return x, y, (x < w) & (y < h)


def per_lane(a, w, h):
    """a [h, w, c] -> [tiles, 64, c], zeros for the lanes outside the frame."""
    x, y, valid = lane_pixels(w, h)
    out = a[np.where(valid, y, 0), np.where(valid, x, 0)].copy()
    out[~valid] = 0
    return out


def butterfly(v):
    """v [tiles, 64] f32: the xor butterfly sum; every lane ends with the same pairs added in the same order."""
    v = v.astype(F32)
    for k in (1, 2, 4, 8, 16, 32):
        v = (v + v[:, LANES ^ k]).astype(F32)
    return v


def pixel_terms(s, p, n):
    """s, p [..., 3] f32 (sums and first-half sums) -> e [...] f32."""
    with np.errstate(all="ignore"):
        q = (s - p).astype(F32)
        d = ((np.abs(p[..., 0] - q[..., 0]) + np.abs(p[..., 1] - q[..., 1])).astype(F32) + np.abs(p[..., 2] - q[..., 2])).astype(F32)
        i = (((s[..., 0] + s[..., 1]).astype(F32) + s[..., 2]).astype(F32) / F32(n)).astype(F32)
        e = ((d / F32(n // 2)).astype(F32) / np.sqrt(i).astype(F32)).astype(F32)
    return np.where(i > 0, e, F32(0)).astype(F32)


def tile_errors(sums, prev, n):
    """sums, prev [h, w, 3] -> E [tiles] f32, for every tile."""
    h, w, _ = sums.shape
    _, _, valid = lane_pixels(w, h)
    e = pixel_terms(per_lane(sums.astype(F32), w, h), per_lane(prev.astype(F32), w, h), n)
    e = np.where(valid, e, F32(0)).astype(F32)
    with np.errstate(all="ignore"):
        return (butterfly(e)[:, 0] / in_frame(w, h).astype(F32)).astype(F32)


def plan(sums, prev, tile_spp, tile_error, n, nxt, tolerance):
    """One plan step.  Returns (tile_error, tile_spp, prev, listed): the new per-tile arrays, the new prev and the listed
    tiles (ascending tile index; the device's order is by error)."""
    h, w, _ = sums.shape
    tile_spp = np.asarray(tile_spp, np.int32).reshape(-1)
    cand = tile_spp == n
    E = tile_errors(sums, prev, n)
    with np.errstate(invalid="ignore"):
        unconv = cand & ~(E <= F32(tolerance))
    err = np.where(cand, E, np.asarray(tile_error, F32).reshape(-1)).astype(F32)
    spp = np.where(unconv, np.int32(nxt), tile_spp).astype(np.int32)
    x, y, valid = lane_pixels(w, h)
    new_prev = prev.astype(F32).copy()
    m = valid & unconv[:, None]
    new_prev[y[m], x[m]] = sums[y[m], x[m]]
    return err, spp, new_prev, np.flatnonzero(unconv)


def predict(frames, spp_min, spp_max, tolerance):
    """The whole loop from uniform frames alone: frames[k] = the sums [h, w, 3] of a uniform k-spp frame of the same seed.
    Returns tile_spp, tile_error (flat) and the stats."""
    h, w, _ = frames[spp_min].shape
    n_tiles = int(np.prod(tiles(w, h)))
    spp = np.full(n_tiles, spp_min, np.int32)
    err = np.zeros(n_tiles, F32)
    passes, n = 0, spp_min
    while n < spp_max:
        nxt = min(2 * n, spp_max)
        err, spp, _, listed = plan(frames[n], frames[n // 2], spp, err, n, nxt, tolerance)
        if not listed.size:
            break
        passes += 1
        n *= 2
    return spp, err, {"samples": int((in_frame(w, h) * spp.astype(np.int64)).sum()), "passes": passes,
                      "tiles_refined": int((spp > spp_min).sum()), "tiles_at_max": int((spp == spp_max).sum())}


def canon(a):
    """uint32 words of an f32 array with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a, F32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def expand(tile_values, w, h):
    """Per-tile values [tiles] -> per-pixel [h, w]."""
    ty, tx = tiles(w, h)
    return np.repeat(np.repeat(np.asarray(tile_values).reshape(ty, tx), 8, 0), 8, 1)[:h, :w]
