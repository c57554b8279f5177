"""A model of the tile and pixel schedules of variants 7, 8 and 10 (numpy, integers only; no GPU, no library).

It states what the schedule kernels of csrc/crt_hip.hip must produce, from their comments and their arithmetic:

* tile_keys        the key of every 8x8 tile from per-pixel costs, and the two probe statistics
* shard_mask       pixel sharding's keys
* sort_violation   what a descending counting sort determines (a permutation, clamped keys non-increasing; the order
                   among equal clamped keys is FREE, the ranks come from atomics) -- a checker, not a sorter
* a_sorted_order   one order that passes it, ties broken by a caller's generator (the model's own input to the
                   XCD step; any tie-break must give the same slot_pairs)
* xcd_applies / xcd_strips / xcd_order / slot_pairs
                   the XCD regions: per slot the pair (strip of the tile, clamped key of the tile) is determined
* expand_slots     a tile order as 64 pixel slots per tile
* shard_tiles      pixel sharding without the probe

Tiles are numbered in row order, t = ty * tiles_x + tx; pixels p = y * width + x.
"""
import numpy as np

TILE = 8
KEY_CLAMP = 1023          # the counting sort has 1024 buckets
XCD_GROUPS = 8
EMPTY = 0xFFFFFFFF        # a slot outside the frame, an order entry no stage wrote


def tile_grid(width, height):
    """(tiles_x, tiles_y)."""
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def tile_keys(cost, width, height, stride=1, mode=0):
    """Keys [n_tiles] (int64) of the 8x8 tiles and (largest tile work, total work).

    A probe of `stride` wrote the pixels with x % stride == 0 and y % stride == 0; no other pixel is looked at.  For a
    tile, m / s / k = the maximum / sum / number of its probed pixels inside the frame: mode 0 gives m, mode 1
    m + s // max(1, k), mode 2 max(m, 3 * nb // 4) with nb the largest mode-0 key among the tile's up to 8 neighbours.
    The tile work is s."""
    c = np.asarray(cost, np.int64).reshape(height, width)
    tx, ty = tile_grid(width, height)
    m = np.zeros((ty, tx), np.int64)
    s = np.zeros((ty, tx), np.int64)
    k = np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            # tile origins are multiples of 8, hence of every stride: the probed pixels of the tile
            block = c[j * TILE:(j + 1) * TILE:stride, i * TILE:(i + 1) * TILE:stride]
            m[j, i], s[j, i], k[j, i] = block.max(), block.sum(), block.size
    if mode == 0:
        key = m
    elif mode == 1:
        key = m + s // np.maximum(1, k)
    elif mode == 2:
        padded = np.zeros((ty + 2, tx + 2), np.int64)     # costs are >= 0: a missing neighbour counts as 0
        padded[1:-1, 1:-1] = m
        nb = np.zeros_like(m)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if (dy, dx) != (1, 1):
                    nb = np.maximum(nb, padded[dy:dy + ty, dx:dx + tx])
        key = np.maximum(m, (3 * nb) // 4)
    else:
        raise ValueError("mode")
    return key.reshape(-1), (int(s.max()), int(s.sum()))


def shard_mask(keys, shard, shards):
    """key + 1 for this shard's tiles (t % shards == shard), 0 for the others."""
    keys = np.asarray(keys, np.int64)
    t = np.arange(keys.size)
    return np.where(t % shards == shard, keys + 1, 0)


def shard_tile_count(n_tiles, shard, shards):
    """ceil((n_tiles - shard) / shards), 0 when the shard has no tile."""
    return max(0, (n_tiles - shard + shards - 1) // shards)


def clamped(keys):
    return np.minimum(np.asarray(keys, np.int64), KEY_CLAMP)


def sort_violation(order, keys):
    """None if `order` is a descending counting sort of `keys`, else what is wrong: it must be a permutation of
    0..n-1 with min(key, 1023) non-increasing along it."""
    keys = np.asarray(keys, np.int64)
    order = np.asarray(order, np.int64)
    n = keys.size
    if order.shape != (n,):
        return f"{order.shape} entries for {n} keys"
    if not np.array_equal(np.sort(order), np.arange(n)):
        return "not a permutation of 0..n-1"
    ck = clamped(keys)[order]
    up = np.nonzero(ck[1:] > ck[:-1])[0]
    if up.size:
        i = int(up[0])
        return f"clamped key rises at position {i + 1}: {ck[i]} -> {ck[i + 1]}"
    return None


def a_sorted_order(keys, rng=None):
    """One order that passes sort_violation: clamped keys descending, ties by index (rng None) or at random."""
    ck = clamped(keys)
    tie = np.arange(ck.size) if rng is None else rng.permutation(ck.size)
    return np.lexsort((tie, -ck)).astype(np.int64)


def xcd_applies(width, height, shards=1):
    """The XCD step runs for one shard, at most 2048 tile columns and a frame of at least 9 pixels per tile (its
    scratch); otherwise the global order stands."""
    tx, ty = tile_grid(width, height)
    return shards == 1 and tx <= 2048 and width * height >= 9 * tx * ty


def xcd_strips(keys, tiles_x):
    """The strip (0..7) of every tile column: a tile weighs min(key, 1023) + 1, a column the sum of its tiles, and
    column c joins strip min(7, (acc + cost[c] // 2) * 8 // total), acc = the cost of the columns before it."""
    w = clamped(keys) + 1
    col = np.zeros(tiles_x, np.int64)
    np.add.at(col, np.arange(w.size) % tiles_x, w)
    total = int(col.sum())
    strips, acc = [], 0
    for c in range(tiles_x):
        strips.append(min(XCD_GROUPS - 1, (acc + int(col[c]) // 2) * XCD_GROUPS // max(1, total)))
        acc += int(col[c])
    return np.array(strips, np.int64)


def xcd_order(order, keys, tiles_x):
    """The sorted list `order` dealt to the 8 XCD groups: slot b belongs to group b % 8 and is its entry b // 8.

    Strip g's list is the stable sub-list of `order` of the tiles in strip g.  Group g holds n // 8 + (g < n % 8)
    slots; a strip's entries beyond that go to a pool, strips in group order; a group with fewer entries than slots
    fills its last slots from the pool, starting where the deficits of the groups before it end."""
    order = np.asarray(order, np.int64)
    n = order.size
    strip_of_col = xcd_strips(keys, tiles_x)
    lists = [[] for _ in range(XCD_GROUPS)]
    for t in order:
        lists[strip_of_col[t % tiles_x]].append(int(t))
    cap = [n // XCD_GROUPS + (1 if g < n % XCD_GROUPS else 0) for g in range(XCD_GROUPS)]
    pool, deficit_before, d = [], [], 0
    for g in range(XCD_GROUPS):
        pool += lists[g][cap[g]:]
        deficit_before.append(d)
        d += max(0, cap[g] - len(lists[g]))
    out = np.empty(n, np.int64)
    for b in range(n):
        g, i = b % XCD_GROUPS, b // XCD_GROUPS
        out[b] = lists[g][i] if i < len(lists[g]) else pool[deficit_before[g] + i - len(lists[g])]
    return out


def slot_pairs(order, keys, tiles_x):
    """Per slot (strip of the tile, clamped key of the tile), [n, 2]: what the XCD order determines."""
    order = np.asarray(order, np.int64)
    return np.stack([xcd_strips(keys, tiles_x)[order % tiles_x], clamped(keys)[order]], axis=1)


def expand_slots(tile_order, width, height):
    """Slot s of tile tile_order[s >> 6] is the pixel (x0 + (s & 7), y0 + ((s & 63) >> 3)), EMPTY outside the frame."""
    tx, _ = tile_grid(width, height)
    t = np.repeat(np.asarray(tile_order, np.int64), TILE * TILE)
    q = np.tile(np.arange(TILE * TILE), len(tile_order))
    x = (t % tx) * TILE + (q & 7)
    y = (t // tx) * TILE + (q >> 3)
    return np.where((x < width) & (y < height), y * width + x, EMPTY).astype(np.int64)


def shard_tiles(n_tiles, shard, shards):
    """Pixel sharding without the probe: the shard's tiles in row order."""
    return np.arange(shard, n_tiles, shards, dtype=np.int64)
