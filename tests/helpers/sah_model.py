"""A numpy float32 restatement of crt_sah::Builder::build_range (csrc/crt_sah.h) that re-derives every decision of an
exported binary tree from the node's own items.

Input: a `width=2, layouts=1` rebuilt export (crt_scene_export): the binary tree as Rebuilt::emit writes it from the
root, depth first, child[0] before child[1]; the primitives in leaf order, so every subtree owns one contiguous range
of primitive records.  The items are recomputed from those records the way Rebuilt::build makes them: a triangle's box
is the float32 min / max of v0, v0 + e1, v0 + e2, a sphere's is c -/+ |r|, the centre is 0.5f * lo + 0.5f * hi.

check_tree() walks the tree and asserts, for every node:

* its box is pad_box of the union of its items' boxes (compared as floats: the sign of a zero does not count);
* a leaf has one item, or has no sphere, at most leaf_size items, and either no split candidate or a best split that
  does not pay (trav_cost + best_cost / max(half_area, 1e-30f) >= count);
* an internal node is not such a leaf, and with a best split its left child holds exactly the items whose bin on the
  best axis lies below the best split;
* an internal node without a best split (a fallback node) has children of count / 2 and count - count / 2 items, and on
  the widest axis of its box every left centre is <= every right centre (std::nth_element's postcondition).

The sweep is the builder's: 128 bins over the centre extent of each axis whose extent is > 0, right sweep from bin 127
down to 1, left sweep from 0 to 126, candidates with an empty side skipped, `cost < best` strict in axis order 0, 1, 2,
and the same unfused float32 expressions in the same order (half_area = dx * dy + dy * dz + dz * dx).  Minima and
maxima are exact and order-free, so the sweeps are cumulative minima / maxima over the bins.

It returns the fallback nodes, each with whether all its items' centres are bit-equal on all three axes.  Meant for
scenes of at most a few thousand items.
"""
import numpy as np

F32 = np.float32
BINS = 128                      # CRT_SAH_BINS
SPHERE_BIT = 1 << 30
INNER = -1                      # NODE_MESH_INNER


def items_of(export):
    """(lo, hi, c, sphere, rank) of every primitive record of the export, as Rebuilt::build makes its items."""
    p = np.ascontiguousarray(export["prims"], np.float32).reshape(-1, 3, 4)
    sph = p[:, 2, 3].view(np.int32) == 1
    v0 = p[:, 0, :3]
    e1 = np.stack([p[:, 0, 3], p[:, 1, 0], p[:, 1, 1]], 1)
    e2 = np.stack([p[:, 1, 2], p[:, 1, 3], p[:, 2, 0]], 1)
    v1, v2 = (v0 + e1).astype(F32), (v0 + e2).astype(F32)
    lo = np.minimum(v0, np.minimum(v1, v2))
    hi = np.maximum(v0, np.maximum(v1, v2))
    r = np.abs(p[:, 0, 3])[:, None]
    lo = np.where(sph[:, None], (v0 - r).astype(F32), lo).astype(F32)
    hi = np.where(sph[:, None], (v0 + r).astype(F32), hi).astype(F32)
    c = (F32(0.5) * lo + F32(0.5) * hi).astype(F32)
    return lo, hi, c, sph, p[:, 2, 2].view(np.int32).copy()


def half_area(lo, hi):
    """crt_sah::half_area over the last axis, float32, unfused, in the builder's order."""
    d = (hi - lo).astype(F32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return ((dx * dy).astype(F32) + (dy * dz).astype(F32)).astype(F32) + (dz * dx).astype(F32)


def pad_box(lo, hi):
    m = max(F32(1), np.abs(lo).max(), np.abs(hi).max())
    pad = F32(1e-5) * F32(m)
    return (lo - pad).astype(F32), (hi + pad).astype(F32)


def bins_of(c, clo, scale):
    """min(127, (int)((c - clo) * scale)) of the builder, for one axis."""
    return np.minimum(BINS - 1, ((c - clo).astype(F32) * scale).astype(F32).astype(np.int32))


def best_split(lo, hi, c):
    """The binned-SAH sweep over one node's items: (best_axis, best_split, best_cost, clo, scale[3]); best_axis -1
    when no candidate was taken."""
    clo, chi = c.min(0), c.max(0)
    best_cost, best_axis, best_at = F32(np.inf), -1, 0
    scales = np.zeros(3, F32)
    with np.errstate(all="ignore"):
        for a in range(3):
            ext = F32(chi[a] - clo[a])
            if not ext > 0:
                continue
            scale = F32(BINS) / ext
            scales[a] = scale
            b = bins_of(c[:, a], clo[a], scale)
            cnt = np.bincount(b, minlength=BINS)
            blo = np.full((BINS, 3), np.inf, F32)
            bhi = np.full((BINS, 3), -np.inf, F32)
            order = np.argsort(b, kind="stable")
            used, at = np.unique(b[order], return_index=True)
            blo[used] = np.minimum.reduceat(lo[order], at, axis=0)
            bhi[used] = np.maximum.reduceat(hi[order], at, axis=0)
            # right sweep, bins 127 .. 1: counts and boxes of bins >= b
            rc = np.cumsum(cnt[::-1])[::-1]
            rlo = np.minimum.accumulate(blo[::-1], axis=0)[::-1]
            rhi = np.maximum.accumulate(bhi[::-1], axis=0)[::-1]
            right_area = np.where(rc > 0, half_area(rlo, rhi), F32(0)).astype(F32)
            # left sweep, bins 0 .. 126: counts and boxes of bins <= b; the candidate splits between b and b + 1
            lc = np.cumsum(cnt)
            llo = np.minimum.accumulate(blo, axis=0)
            lhi = np.maximum.accumulate(bhi, axis=0)
            left_area = half_area(llo, lhi)
            lcn, rcn = lc[:BINS - 1], rc[1:]
            cost = ((left_area[:BINS - 1] * lcn.astype(F32)).astype(F32)
                    + (right_area[1:] * rcn.astype(F32)).astype(F32)).astype(F32)
            ok = (lcn > 0) & (rcn > 0) & (cost < np.inf)          # NaN and inf never pass `cost < best`
            if not ok.any():
                continue
            masked = np.where(ok, cost, F32(np.inf))
            k = int(np.argmin(masked))                              # the first of equal minima, as the strict sweep
            if masked[k] < best_cost:
                best_cost, best_axis, best_at = F32(masked[k]), a, k + 1
    return best_axis, best_at, best_cost, clo, scales


def _fail(i, what):
    raise AssertionError(f"node {i}: {what}")


def tree_ranges(export):
    """(end, first, count) per node of a width-2, one-layout export: one past the last node of its subtree, and its
    range of primitive records.  Asserts that the skip links and leaf ranges tile the arrays."""
    nodes = np.ascontiguousarray(export["nodes"], np.float32).reshape(-1, 2, 4)
    ints = nodes[:, 1, 2:].view(np.int32)
    n_nodes, n_prims = len(nodes), export["prim_float4s"] // 3
    end_of = np.zeros(n_nodes, np.int64)
    first_of = np.zeros(n_nodes, np.int64)
    count_of = np.zeros(n_nodes, np.int64)
    for i in range(n_nodes - 1, -1, -1):           # children have larger indices than their parent
        a, b = int(ints[i, 0]), int(ints[i, 1])
        if b == INNER:
            if not i + 2 < a <= n_nodes:
                _fail(i, f"skip link {a}")
            left = i + 1
            right = int(end_of[left])
            if not right < a or end_of[right] != a:
                _fail(i, "children do not tile the subtree")
            if first_of[right] != first_of[left] + count_of[left]:
                _fail(i, "children's primitive ranges are not consecutive")
            end_of[i], first_of[i], count_of[i] = a, first_of[left], count_of[left] + count_of[right]
        else:
            f, k = (b - SPHERE_BIT, 1) if b >= SPHERE_BIT else (b, a)
            if not (k >= 1 and 0 <= f and f + k <= n_prims):
                _fail(i, f"leaf range {f}+{k}")
            end_of[i], first_of[i], count_of[i] = i + 1, f, k
    if end_of[0] != n_nodes or first_of[0] != 0 or count_of[0] != n_prims:
        _fail(0, "the root does not cover every node and primitive")
    return end_of, first_of, count_of


def coincident_nodes(export, ranges=None):
    """The internal nodes whose items' centres are all bit-equal on all three axes (no axis has an extent, so no split
    candidate exists: these are exactly the nodes the builder halves), in index order."""
    end_of, first_of, count_of = ranges or tree_ranges(export)
    ints = np.ascontiguousarray(export["nodes"], np.float32).reshape(-1, 2, 4)[:, 1, 2:].view(np.int32)
    c = np.ascontiguousarray(items_of(export)[2]).view(np.uint32)
    same = np.concatenate([[0], np.cumsum((c[1:] == c[:-1]).all(1))])        # same[k]: equal neighbours before item k
    last = first_of + count_of - 1
    all_same = same[last] - same[first_of] == count_of - 1
    return np.nonzero((ints[:, 1] == INNER) & all_same)[0]


def check_tree(export, leaf_size=4, trav_cost=2.0):
    """Checks every node of a width-2, one-layout export (module docstring).  Returns the fallback nodes as dicts:
    node (index in the export), end (one past the subtree's last node), first, count (its primitive range),
    centres_equal (all its items' centres bit-equal on all three axes)."""
    assert export["width"] == 2 and export["layouts"] == 1, "the checker reads the width-2 tree as emitted from the root"
    nodes = np.ascontiguousarray(export["nodes"], np.float32).reshape(-1, 2, 4)
    n_nodes = len(nodes)
    assert n_nodes == export["nodes_per_layout"]
    ints = nodes[:, 1, 2:].view(np.int32)
    nlo = nodes[:, 0, :3]
    nhi = np.concatenate([nodes[:, 0, 3:], nodes[:, 1, :2]], 1)
    lo, hi, c, sph, _ = items_of(export)
    trav_cost = F32(trav_cost)
    fallbacks = []
    n_seen = 0

    end_of, first_of, count_of = tree_ranges(export)

    with np.errstate(all="ignore"):
        for i in range(n_nodes):
            f, count = int(first_of[i]), int(count_of[i])
            s = slice(f, f + count)
            ilo, ihi, ic = lo[s], hi[s], c[s]
            blo, bhi = pad_box(ilo.min(0), ihi.max(0))
            if not (np.array_equal(blo, nlo[i]) and np.array_equal(bhi, nhi[i])):
                _fail(i, f"box {nlo[i]} {nhi[i]} is not the padded union {blo} {bhi} of its {count} items")
            is_leaf = ints[i, 1] != INNER
            if is_leaf:
                n_seen += count
            if count == 1:
                if not is_leaf:
                    _fail(i, "one item but not a leaf")
                if bool(sph[f]) != bool(ints[i, 1] & SPHERE_BIT):
                    _fail(i, "sphere flag of a single-item leaf")
                continue
            n_sph = int(sph[s].sum())
            axis, at, cost, clo, scales = best_split(ilo, ihi, ic)
            leaf_ok = n_sph == 0 and count <= leaf_size
            node_area = max(half_area(nlo[i], nhi[i]), F32(1e-30))
            no_gain = axis < 0 or F32(trav_cost + F32(cost / node_area)) >= F32(count)
            must_leaf = leaf_ok and no_gain
            if is_leaf:
                if not must_leaf:
                    _fail(i, f"a leaf of {count} items ({n_sph} spheres) that the leaf rule does not allow: best axis "
                             f"{axis}, split {at}, cost {cost}, area {node_area}")
                continue
            if must_leaf:
                _fail(i, f"internal, but the leaf rule applies: {count} items, best axis {axis}, cost {cost}")
            left = i + 1
            nl = int(count_of[left])
            if axis >= 0:
                below = bins_of(ic[:, axis], clo[axis], scales[axis]) < at
                if not (below[:nl].all() and not below[nl:].any()):
                    _fail(i, f"{count} items: the left child holds {nl} items, not exactly the {int(below.sum())} below "
                             f"split {at} of axis {axis} (cost {cost})")
                continue
            if nl != count // 2:
                _fail(i, f"fallback node of {count} items with a left child of {nl}")
            d = (nhi[i] - nlo[i]).astype(F32)
            a = 0
            for q in (1, 2):
                if d[q] > d[a]:
                    a = q
            if not ic[:nl, a].max() <= ic[nl:, a].min():
                _fail(i, f"fallback node: a left centre above a right centre on axis {a}")
            fallbacks.append(dict(node=i, end=int(end_of[i]), first=f, count=count,
                                  centres_equal=bool((ic.view(np.uint32) == ic[:1].view(np.uint32)).all())))
    assert n_seen == len(lo)
    return fallbacks
