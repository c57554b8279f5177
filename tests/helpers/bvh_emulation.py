"""Host-side float32 restatements of the rebuilt-BVH kernels' arithmetic, over the arrays of crt_scene_export.

Shared by tests/test_rebuilt_bvh.py, tests/test_synth_scenes.py and tests/test_gpu_synth.py (no GPU needed):

* _check_wide / _check_threaded: structure of the 4-wide and the threaded binary layouts;
* _mt_all / _sphere_all / _prim_t: Moller-Trumbore and Sphere::hit over primitive records, in the kernel's
  operation order;
* _best: the hit rule (closest t, ties to the higher reference rank);
* _trace_wide_rays / _trace_wide: the variant-4 traversal of the exported 4-wide nodes, with the kernel's slab arithmetic.
"""
import numpy as np

F32 = np.float32
BOX_INV_CLAMP = F32(2.0 ** 64)      # crt_hip.hip BOX_INV_CLAMP


def _i(a):
    return np.asarray(a, np.float32).view(np.int32)


def _prim_ranks(prims):
    return _i(prims.reshape(-1, 3, 4)[:, 2, 2])


def _is_sphere(prims):
    return _i(prims.reshape(-1, 3, 4)[:, 2, 3]) == 1


def _prim_box(rec):
    if _i(rec[2, 3]) == 1:
        c, r = rec[0, :3], abs(rec[0, 3])
        return c - r, c + r
    v0 = rec[0, :3]
    e1 = np.array([rec[0, 3], rec[1, 0], rec[1, 1]], np.float32)
    e2 = np.array([rec[1, 2], rec[1, 3], rec[2, 0]], np.float32)
    pts = np.stack([v0, v0 + e1, v0 + e2])
    return pts.min(0), pts.max(0)


def _check_wide(e, prims, split_ranks=()):
    """split_ranks: ranks of triangles a spatial-split build references from several leaves; each reference is boxed
    by its part of the triangle, so only those are exempt from the enclosure check."""
    nodes = e["nodes"].reshape(-1, 8, 4)
    split_ranks = set(int(r) for r in split_ranks)
    ranks = _prim_ranks(e["prims"])
    n = len(nodes)
    assert n == e["nodes_per_layout"]
    seen = np.zeros(len(prims), np.int32)
    parent_of = {0: None}
    for i in range(n):
        q = nodes[i]
        fc, meta, lf, counts = _i(q[6])
        n_int, n_slots = meta & 0xFF, meta >> 8
        assert 0 <= n_int <= n_slots <= 4
        off = 0
        for s in range(4):
            lo = np.array([q[0, s], q[2, s], q[4, s]])
            hi = np.array([q[1, s], q[3, s], q[5, s]])
            c = (counts >> (8 * s)) & 0xFF
            if s >= n_slots:
                assert (lo == 1e30).all() and (hi == 1e30).all() and c == 0
            elif s < n_int:
                assert c == 0
                child = fc + s
                assert 0 < child < n and child not in parent_of
                parent_of[child] = (i, lo, hi)
            else:
                assert c > 0
                for p in range(lf + off, lf + off + c):
                    seen[p] += 1
                    if int(ranks[p]) in split_ranks:
                        continue
                    plo, phi = _prim_box(prims[p])
                    assert (plo > lo).all() and (phi < hi).all(), "leaf box must strictly enclose (padding)"
                off += c
    rs = slice(e["sphere_first"], e["sphere_first"] + e["n_ray_spheres"])
    assert _is_sphere(e["prims"])[rs].all(), "per-ray list holds spheres only"
    seen[rs] += 1
    assert (seen == 1).all(), "every primitive in exactly one leaf or the per-ray sphere list"
    assert len(parent_of) == n
    # child node boxes inside their parent's slot box
    for child, pr in parent_of.items():
        if pr is None:
            continue
        _, lo, hi = pr
        q = nodes[child]
        meta = _i(q[6])[1]
        for s in range(meta >> 8):
            assert q[0, s] >= lo[0] and q[2, s] >= lo[1] and q[4, s] >= lo[2]
            assert q[1, s] <= hi[0] and q[3, s] <= hi[1] and q[5, s] <= hi[2]
    # stack bound = max over root paths of the branching nodes (one entry per node), recomputed independently
    bound = np.zeros(n, np.int64)
    for i in range(n - 1, -1, -1):
        fc, meta = _i(nodes[i, 6])[:2]
        m = meta & 0xFF
        bound[i] = (max(bound[fc + s] for s in range(m)) if m else 0) + (1 if m >= 2 else 0)
    assert e["stack_bound"] == bound[0] + 1


def _check_threaded(e, prims):
    nodes = e["nodes"].reshape(e["layouts"], -1, 2, 4)
    seen = np.zeros(len(prims), np.int32)
    for lay in range(e["layouts"]):
        L = nodes[lay]
        cnt = np.zeros(len(prims), np.int32)
        for i in range(len(L)):
            a, b = _i(L[i, 1, 2:])
            if b == -1:
                assert i < a <= len(L)
            elif b >= 1 << 30:
                cnt[b - (1 << 30)] += 1
            else:
                cnt[b:b + a] += 1
        assert (cnt == 1).all()
        seen += cnt
    assert (seen == e["layouts"]).all()


# ---------------------------------------------------------------- traversal semantics
def _mt_all(prims, o, d, tmax):
    """Möller–Trumbore over all triangle records, float32 with the kernel's operation order."""
    f0, f1, f2 = prims[:, 0], prims[:, 1], prims[:, 2]
    v0 = f0[:, :3]
    e1 = np.stack([f0[:, 3], f1[:, 0], f1[:, 1]], 1)
    e2 = np.stack([f1[:, 2], f1[:, 3], f2[:, 0]], 1)

    def cross(u, v):
        return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                         u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)

    def dot(u, v):
        return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]

    with np.errstate(all="ignore"):
        dd = np.broadcast_to(d, e2.shape)
        h = cross(dd, e2)
        det = dot(e1, h)
        ok = ~(np.abs(det) < F32(1e-8))
        f = F32(1) / det
        s = o - v0
        u = f * dot(s, h)
        ok &= ~((u < 0) | (u > 1))
        q = cross(s, e1)
        v = f * dot(dd, q)
        ok &= ~((v < 0) | ((u + v) > 1))
        t = f * dot(e2, q)
        ok &= ~((t < F32(0.001)) | (t > tmax))
    return np.where(ok, t, -1).astype(np.float32)


def _sphere_all(prims, o, d, tmax):
    f0, f1 = prims[:, 0], prims[:, 1]
    with np.errstate(all="ignore"):
        oc = o - f0[:, :3]
        qa = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        hb = (oc[:, 0] * d[..., 0] + oc[:, 1] * d[..., 1]) + oc[:, 2] * d[..., 2]
        qc = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - f1[:, 0]
        disc = hb * hb - qa * qc
        sq = np.sqrt(np.maximum(disc, 0)).astype(np.float32)
        r1 = (-hb - sq) / qa
        r2 = (-hb + sq) / qa
        bad1 = (r1 < F32(0.001)) | (r1 > tmax)
        bad2 = (r2 < F32(0.001)) | (r2 > tmax)
        t = np.where(bad1, np.where(bad2, -1, r2), r1)
    return np.where(disc < 0, -1, t).astype(np.float32)


def _prim_t(prims, o, d, tmax):
    """t or -1 per record.  o, d, tmax: one ray for all records, or one ray per record ((n, 3), (n, 3), (n,))."""
    sph = _i(prims[:, 2, 3]) == 1
    t = _mt_all(prims, o, d, tmax)
    if sph.any():
        per = np.ndim(o) == 2
        t[sph] = _sphere_all(prims[sph], o[sph] if per else o, d[sph] if per else d,
                             tmax[sph] if np.ndim(tmax) else tmax)
    return t


def _best(t, ranks, closest=np.float32(np.inf), hit=-1):
    ok = t >= 0
    if not ok.any():
        return closest, hit
    tm = t[ok].min()
    r = ranks[ok][t[ok] == tm].max()
    if tm < closest or (tm == closest and r > hit):
        return tm, int(r)
    return closest, hit


def _fma32(a, b, c):
    """fl32(a * b + c) with one rounding, for float32 arrays.  a * b is exact in float64 (48 bits); the sum is taken
    to float64 with round-to-odd (TwoSum's error term says whether it was inexact and on which side), which rounds
    to the same float32 as the exact sum."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = np.broadcast_to(c.astype(np.float64), p.shape)
        s = np.ascontiguousarray(p + c)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & (err != 0)
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def _box_inv(d):
    """The traversal's 1/d: the exact float32 reciprocal clamped to +-2^64 (crt_hip.hip box_inv); -0 gives -2^64."""
    with np.errstate(all="ignore"):
        inv = (F32(1) / np.asarray(d, np.float32)).astype(np.float32)
    return np.clip(inv, -BOX_INV_CLAMP, BOX_INV_CLAMP).astype(np.float32)


def _wide_boxes(q, o, binv, tmax):
    """wide_boxes_of for n rays, each at its own node: q (n, 8, 4), o / binv (n, 3), tmax (n,) -> tmin (n, 4),
    hit (n, 4) of the child boxes against [0.001, tmax].

    Per axis the kernel takes fma(plane, inv, -(o * inv)) of the row the ray enters by (lo for inv >= 0, hi for the
    sign bit of inv set, -0 included) and of the row it leaves by.  fma is monotone in the plane, so these are exactly
    min / max of the two planes' values: the row choice is the min/max form without the min/max.  Against the earlier
    (plane - o) * inv form nothing is provable bit for bit: the two round differently (the fma once, the other
    twice), and for a clamped inv the old form gives +-inf or NaN where this one stays finite.  Both err by about
    ulp(o) * |inv|, inside the boxes' padding; this is the form the kernel runs, so it is the one restated."""
    ent, ext = [], []
    for k in range(3):
        inv = binv[:, k:k + 1]
        n = (-(o[:, k:k + 1] * inv)).astype(np.float32)
        lo, hi = q[:, 2 * k], q[:, 2 * k + 1]
        neg = np.signbit(inv)
        ent.append(_fma32(np.where(neg, hi, lo), inv, n))
        ext.append(_fma32(np.where(neg, lo, hi), inv, n))
    t0 = np.fmax(np.fmax(ent[0], ent[1]), np.fmax(ent[2], F32(0.001)))
    t1 = np.fmin(np.fmin(ext[0], ext[1]), np.fmin(ext[2], tmax[:, None]))
    return t0, t0 < t1


def _ref_sphere_box(rec, o, d):
    """ref_scene_box of one per-ray sphere for n rays: AABB::hit of the sphere's reference scene-level leaf box (the
    sphere's own box, Sphere.cuh:20-25) against [0.001, inf) with the exact 1/d.  The reference never tests a sphere
    whose box its ray misses."""
    c, r = rec[0, :3], rec[0, 3]
    rv = np.array([r, r, r], np.float32)
    a, b = (c - rv).astype(np.float32), (c + rv).astype(np.float32)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    with np.errstate(all="ignore"):
        inv = (F32(1) / d).astype(np.float32)
        t0, t1 = ((lo - o) * inv).astype(np.float32), ((hi - o) * inv).astype(np.float32)
    mn, mx = np.fmin(t0, t1), np.fmax(t0, t1)
    tmin = np.fmax(np.fmax(np.fmax(mn[:, 0], mn[:, 1]), mn[:, 2]), F32(0.001))
    tmax = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), mx[:, 2])
    return ~(tmax <= tmin)


def _merge(closest, hit, rays, t, r):
    """The hit rule over candidate (ray, t, rank) triples: per ray the smallest t >= 0, of equal t the higher rank,
    taken if better than (closest, hit)."""
    ok = t >= 0
    rays, t, r = rays[ok], t[ok], r[ok]
    if not len(rays):
        return
    order = np.lexsort((-r, t, rays))
    rays, t, r = rays[order], t[order], r[order]
    first = np.ones(len(rays), bool)
    first[1:] = rays[1:] != rays[:-1]
    rays, t, r = rays[first], t[first], r[first]
    take = (t < closest[rays]) | ((t == closest[rays]) & (r > hit[rays]))
    closest[rays[take]] = t[take]
    hit[rays[take]] = r[take]


def _trace_wide_rays(e, prims, ranks, o, d, box_tests=None):
    """Closest hit (t (n,), rank (n,); inf / -1 on a miss) of n rays over a 4-wide export, as kernel variant 4
    computes it: the per-ray spheres behind the reference's box test, then the stack traversal with the kernel's slab
    arithmetic.  The rays advance in lockstep, each with its own stack.  box_tests: an int64 array (n,) that
    receives the child boxes tested per ray, the slots of every node visited, as a counting render adds them up (for a
    ray that hits nothing the visiting order cannot change that number)."""
    nodes = e["nodes"].reshape(-1, 8, 4)
    o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    n = len(o)
    ranks = np.asarray(ranks, np.int64)
    binv = _box_inv(d)
    closest, hit = np.full(n, np.inf, np.float32), np.full(n, -1, np.int64)
    first = e["sphere_first"]
    every = np.arange(n)
    for p in range(first, first + e["n_ray_spheres"]):
        reach = _ref_sphere_box(prims[p], o, d)
        t = _sphere_all(prims[p:p + 1], o, d, np.float32(np.inf))
        _merge(closest, hit, every[reach], t[reach], np.full(int(reach.sum()), ranks[p]))
    stack = np.zeros((n, 64), np.int64)
    sp = np.zeros(n, np.int64)
    node = np.zeros(n, np.int64)
    while True:
        act = np.nonzero(node >= 0)[0]
        if not len(act):
            break
        q = nodes[node[act]]
        t0, hitm = _wide_boxes(q, o[act], binv[act], closest[act])
        link = q[:, 6].view(np.int32).astype(np.int64)
        fc, n_int, lf, counts = link[:, 0], link[:, 1] & 0xFF, link[:, 2], link[:, 3]
        if box_tests is not None:
            box_tests[act] += link[:, 1] >> 8
        entry = closest[act].copy()
        pr, pp = [], []
        off = np.zeros(len(act), np.int64)
        for s in range(4):
            c = (counts >> (8 * s)) & 0xFF
            m = (s >= n_int) & (c > 0) & hitm[:, s]
            for k in range(int(c[m].max()) if m.any() else 0):
                mk = np.nonzero(m & (k < c))[0]
                pr.append(mk)
                pp.append(lf[mk] + off[mk] + k)
            off += c
        if pr:
            pr, pp = np.concatenate(pr), np.concatenate(pp)
            t = _prim_t(prims[pp], o[act[pr]], d[act[pr]], entry[pr])
            _merge(closest, hit, act[pr], t, ranks[pp])
        kid = hitm & (np.arange(4)[None, :] < n_int[:, None])
        key = np.where(kid, t0, np.inf)
        order = np.argsort(key, axis=1, kind="stable")          # nearest first, ties to the lower slot
        cnt = kid.sum(1)
        for j in (3, 2, 1):                                      # push the farther children, farthest first
            push = np.nonzero(cnt > j)[0]
            a = act[push]
            stack[a, sp[a]] = fc[push] + order[push, j]
            sp[a] += 1
        go = cnt > 0
        node[act[go]] = fc[go] + order[go, 0]
        rest = act[~go]
        pop = sp[rest] > 0
        sp[rest[pop]] -= 1
        node[rest[pop]] = stack[rest[pop], sp[rest[pop]]]
        node[rest[~pop]] = -1
    return closest, hit


def _trace_wide(e, prims, ranks, o, d):
    """_trace_wide_rays for one ray: (t, rank)."""
    t, r = _trace_wide_rays(e, prims, ranks, np.asarray(o, np.float32)[None], np.asarray(d, np.float32)[None])
    return t[0], int(r[0])
