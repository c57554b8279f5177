"""The GPU binned-SAH build (crtx_build_sah_gpu, crt_scene_options.gpu_build) split by split: against the host builder
and against the numpy model of the rules (tests/helpers/sah_model.py), which does not lean on the host builder.

Scenes: every scene of tests/test_sah_decisions_cpu.py, `interleaved` (69,000 items) and sized soups of 4093 .. 20000
triangles.  Item counts sit at the kernels' constants: SAH_SMALL 16 / 17 (a root that k_sah_small decides, no big node
at all; a root the reduction path decides), SCAN_ITEMS 1024, SAH_CHUNK 4096 and 8192 (uniform against mixed
workgroups), levels of more than 1,024 nodes (20,000 items at leaf size 1).  Spheres sit in big and in small nodes, the
grids have a zero centroid extent on one axis, and the concentric clusters (20 spheres, 20 triangles) run the "no
usable split" halving of a big node and of the small nodes below it.  Options: leaf sizes 1, 4, 16, traversal costs default, 2, 8, widths 2 and 4.

a. host against GPU, by the rules of test_gpu_bvh_build.py::test_gpu_sah_tree_equals_host: equal integer fields, equal
   boxes and node words, equal multisets of primitive ranks under every node.  Exact, no tolerance.
   The one exemption: a node whose items' box centres are all bit-equal has no split candidate and is halved; which
   items make the lower half is each builder's own order (the host's std::nth_element over equal keys after unstable
   partitions, the GPU's stable order).  Under such a node the child sizes and the topology must still agree (every
   integer word of the width-2 nodes is compared everywhere), the node's own box and rank multiset must agree, and both
   trees must pass the checker; the ranks of the leaves below it may differ, and, only in the scenes where coincident
   items have different boxes (BOXES_MAY_DIFFER), so may the boxes below it.
b. the checker over every GPU-built width-2 tree of the scenes small enough for it.
c. Scene.trace through the concentric cluster against brute force over the exported primitives.

Each case prints what it found under the halved nodes (run with -s); DESIGN.md section 12 records it.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import custom_scene  # noqa: E402
import sah_model  # noqa: E402
from bvh_emulation import _best, _check_wide, _prim_ranks, _prim_t  # noqa: E402
from custom_scene import SAH_SOUP_SIZES_BIG  # noqa: E402
from test_sah_decisions_cpu import (CHECKED_WORLDS, COINCIDENT, OPTION_SETS, TOO_LARGE, all_worlds,  # noqa: E402
                                    check_export, export_options)

pytestmark = pytest.mark.gpu

BIG_SOUPS = tuple(f"soup_{n}" for n in SAH_SOUP_SIZES_BIG)
COMPARED_WORLDS = CHECKED_WORLDS + TOO_LARGE + BIG_SOUPS
# coincident items with different boxes: the halves' boxes depend on which items they hold.  Everywhere else the
# coincident items (the two triangles of an axis-aligned quad, twin spheres) share one box, and every box must agree.
BOXES_MAY_DIFFER = ("concentric", "concentric_soup", "concentric_tris", "ties", "degenerate")
INNER = -1


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    d = tmp_path_factory.mktemp("sah_gpu")
    out = all_worlds(d)
    out.update({f"soup_{n}": custom_scene.SizedSoup(d, n) for n in SAH_SOUP_SIZES_BIG})
    return out


def _int_fields(e):
    return {k: v for k, v in e.items() if isinstance(v, int)}


def _boxes2(e):
    n = e["nodes"].reshape(-1, 2, 4)
    return np.concatenate([n[:, 0], n[:, 1, :2]], 1)


def _compare_w2(name, h, g):
    """Host against GPU over the threaded width-2 layout.  Returns (ranks exempt from the leaf comparison, halved
    subtrees, those with other leaf ranks on the GPU, those with other boxes on the GPU)."""
    assert _int_fields(h) == _int_fields(g)
    hi, gi = (e["nodes"].reshape(-1, 2, 4)[:, 1, 2:].view(np.int32) for e in (h, g))
    bad = np.nonzero((hi != gi).any(1))[0]
    assert len(bad) == 0, f"node words (skip / count, leaf range) differ at nodes {bad[:8].tolist()}"
    ranges = sah_model.tree_ranges(h)
    end_of, first_of, count_of = ranges
    co = sah_model.coincident_nodes(h, ranges)
    assert np.array_equal(co, sah_model.coincident_nodes(g, ranges)), "nodes of bit-equal centres"
    assert name in COINCIDENT or len(co) == 0, f"halved nodes {co[:8].tolist()} in a scene without coincident centres"
    n_nodes, n_prims = len(hi), h["prim_float4s"] // 3
    under = np.zeros(n_nodes, bool)                  # strictly below a halved node
    group = np.full(n_prims, -1, np.int64)           # the outermost halved node over a primitive
    outer = []
    for i in co:
        if not under[i]:
            outer.append(int(i))
            group[first_of[i]:first_of[i] + count_of[i]] = i
        under[i + 1:end_of[i]] = True
    box_diff = (_boxes2(h) != _boxes2(g)).any(1)
    bad = np.nonzero(box_diff & ~under)[0]
    assert len(bad) == 0, f"boxes differ at nodes {bad[:8].tolist()}"
    if name not in BOXES_MAY_DIFFER:
        bad = np.nonzero(box_diff)[0]
        assert len(bad) == 0, f"boxes differ under halved nodes whose items share one box: {bad[:8].tolist()}"
    leaves = np.nonzero(hi[:, 1] != INNER)[0]
    assert np.array_equal(first_of[leaves], np.concatenate([[0], np.cumsum(count_of[leaves])[:-1]]))
    leaf_of = np.repeat(leaves, count_of[leaves])
    hr, gr = _prim_ranks(h["prims"]).astype(np.int64), _prim_ranks(g["prims"]).astype(np.int64)
    hs, gs = hr[np.lexsort((hr, leaf_of))], gr[np.lexsort((gr, leaf_of))]     # ranks sorted inside every leaf
    rank_diff = hs != gs
    bad = np.nonzero(rank_diff & (group < 0))[0]
    assert len(bad) == 0, f"leaf rank multisets differ at primitive positions {bad[:8].tolist()}"
    # a halved node holds the same primitives in both trees
    assert np.array_equal(hr[np.lexsort((hr, group))], gr[np.lexsort((gr, group))]), "rank multisets of halved nodes"
    other_ranks = sum(bool(rank_diff[first_of[i]:first_of[i] + count_of[i]].any()) for i in outer)
    other_boxes = sum(bool(box_diff[i + 1:end_of[i]].any()) for i in outer)
    return np.unique(hr[group >= 0]), len(outer), other_ranks, other_boxes


def _wide_node_ranks(e, drop):
    """(node, rank) of every tree primitive of a 4-wide export, sorted, without the ranks in `drop`."""
    meta = e["nodes"].reshape(-1, 8, 4)[:, 6].view(np.int32)
    total = sum((meta[:, 3] >> (8 * s)) & 0xff for s in range(4)).astype(np.int64)
    assert np.array_equal(meta[:, 2], np.concatenate([[0], np.cumsum(total)[:-1]])), "leaf spans are consecutive"
    assert total.sum() == e["sphere_first"]
    node_of = np.repeat(np.arange(len(meta)), total)
    ranks = _prim_ranks(e["prims"])[:e["sphere_first"]].astype(np.int64)
    keep = ~np.isin(ranks, drop)
    node_of, ranks = node_of[keep], ranks[keep]
    order = np.lexsort((ranks, node_of))
    return node_of[order], ranks[order]


def _root_bounds(e):
    """The union of the root's used slots of a 4-wide export: [lo x, hi x, lo y, hi y, lo z, hi z]."""
    root = e["nodes"].reshape(-1, 8, 4)[0]
    used = (root[6].view(np.int32)[1] >> 8) & 0xff
    return [float((np.min, np.max)[r % 2](root[r, :used])) for r in range(6)]


def _compare_w4(name, h, g, exempt_ranks, boxes_agreed):
    """Host against GPU over the 4-wide layout, by test_gpu_sah_tree_equals_host's rules.  exempt_ranks: the
    primitives under halved nodes of the binary tree (from the width-2 comparison at the same options)."""
    hr, gr = _prim_ranks(h["prims"]), _prim_ranks(g["prims"])
    assert np.array_equal(np.sort(hr), np.sort(gr)), "the trees hold the same primitives"
    assert np.array_equal(hr[h["sphere_first"]:], gr[g["sphere_first"]:]), "per-ray spheres"
    if not boxes_agreed:
        # The halves of a coincident cluster hold other items, so their boxes differ, and the collapse, which weighs
        # areas, may cut the binary tree elsewhere: the 4-wide arrays are then not comparable node by node.  Both
        # are checked for structure, and the roots bound the same scene.
        assert name in BOXES_MAY_DIFFER
        for e in (h, g):
            _check_wide(e, e["prims"].reshape(-1, 3, 4))
        assert _root_bounds(h) == _root_bounds(g)
        return
    assert _int_fields(h) == _int_fields(g)
    hn, gn = h["nodes"].reshape(-1, 8, 4), g["nodes"].reshape(-1, 8, 4)
    assert np.array_equal(hn[:, :6], gn[:, :6]), "child boxes"
    assert np.array_equal(hn[:, 6].view(np.int32), gn[:, 6].view(np.int32)), "node meta"
    a, b = _wide_node_ranks(h, exempt_ranks), _wide_node_ranks(g, exempt_ranks)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "rank multisets under the 4-wide nodes"


@pytest.mark.parametrize("opts", list(OPTION_SETS))
@pytest.mark.parametrize("name", COMPARED_WORLDS)
def test_gpu_tree_equals_host_and_model(worlds, name, opts):
    leaf_size, trav_cost = OPTION_SETS[opts]
    w = worlds[name]
    h2 = w.export("rebuilt", **export_options(leaf_size, trav_cost, 2, False))
    g2 = w.export("rebuilt", **export_options(leaf_size, trav_cost, 2, True))
    if name in CHECKED_WORLDS:                       # b. the model over the GPU's tree, before any comparison
        fb = check_export(name, g2, leaf_size, trav_cost)
        if name.startswith("concentric"):
            assert max(f["count"] for f in fb) == 20, "the cluster is halved as one big node, then as small ones"
    exempt, n_halved, other_ranks, other_boxes = _compare_w2(name, h2, g2)
    if (other_ranks or other_boxes) and name in CHECKED_WORLDS:
        check_export(name, h2, leaf_size, trav_cost)          # where the trees differ, both must pass the checker
    h4 = w.export("rebuilt", **export_options(leaf_size, trav_cost, 4, False))
    g4 = w.export("rebuilt", **export_options(leaf_size, trav_cost, 4, True))
    _compare_w4(name, h4, g4, exempt, other_boxes == 0)
    if n_halved:
        print(f"\nHALVED {name} {opts}: {n_halved} halved subtrees, {other_ranks} with other leaf ranks on the GPU, "
              f"{other_boxes} with other boxes")


def test_levels_of_more_than_1024_nodes(worlds):
    """20,000 items at leaf size 1: the deepest levels hold more than 1,024 nodes, so every thread of the
    single-workgroup scans (k_big_scan, k_sah_scan) takes several nodes."""
    e = worlds["soup_20000"].export("rebuilt", **export_options(1, None, 2, True))
    end_of, _, _ = sah_model.tree_ranges(e)
    depth = np.zeros(len(end_of), np.int64)
    ints = e["nodes"].reshape(-1, 2, 4)[:, 1, 2:].view(np.int32)
    for i in np.nonzero(ints[:, 1] == INNER)[0]:
        depth[i + 1] = depth[end_of[i + 1]] = depth[i] + 1
    assert np.bincount(depth).max() > 1024


# ------------------------------------------------------------------------------------------ c. hits on the cluster
@pytest.mark.parametrize("name", ["concentric", "concentric_soup", "concentric_tris"])
@pytest.mark.parametrize("width", [2, 4])
def test_concentric_hits(worlds, name, width):
    """Rays through the halved cluster, from outside and from between the shells: t bits and the primitive of
    Scene.trace over the GPU-built tree equal brute force over the exported records (closest t, ties to the higher
    rank)."""
    cs = worlds[name]
    opts = dict(width=width, leaf_size=4, gpu_build=True)
    e = cs.export("rebuilt", **opts)
    prims, ranks = e["prims"].reshape(-1, 3, 4), _prim_ranks(e["prims"])
    _, _, c, sph, _ = sah_model.items_of(e)
    centre = c[~sph][0] if name == "concentric_tris" else np.zeros(3, np.float32)      # the cluster's one box centre
    rng = np.random.default_rng(5)
    n = 400
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    start = np.where(np.arange(n)[:, None] < 250, 0.45, rng.uniform(0.005, 0.2, (n, 1)))   # outside / between shells
    o = (centre + u * start).astype(np.float32)
    aim = rng.uniform(-0.2, 0.2, (n, 3)) * (np.arange(n)[:, None] % 3 != 0)                  # a third through the centre
    d = ((centre + 0.25 * aim) - o).astype(np.float32) if name == "concentric_tris" else (aim - o).astype(np.float32)
    sc = crt_amd.create_scene(cs.desc, 0, "rebuilt", **opts)
    got = sc.trace(o, d)
    ident = crt_amd.identity_desc(cs.desc)
    exp_t, exp_rank = np.zeros(n, np.float32), np.zeros(n, np.int64)
    for k in range(n):
        exp_t[k], exp_rank[k] = _best(_prim_t(prims, o[k], d[k], np.float32(np.inf)), ranks)
    hit = exp_rank >= 0
    assert hit.sum() >= 250
    assert len(np.unique(exp_rank[hit])) >= 15, "the rays end on most members of the cluster"
    assert np.array_equal(got["t"] >= 0, hit)
    assert np.array_equal(got["t"][hit].view(np.uint32), exp_t[hit].view(np.uint32)), "t bits"
    assert np.array_equal(got["object"][hit], ident[exp_rank[hit], 0]), "object of the rank"
    assert np.array_equal(got["primitive"][hit], ident[exp_rank[hit], 1]), "primitive of the rank"
