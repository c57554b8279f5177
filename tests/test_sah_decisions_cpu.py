"""Every split of the host binned-SAH builder (crt_sah::Builder) against a numpy restatement of its rules (no GPU).

tests/helpers/sah_model.py re-derives, from the items under every node of a width-2 export, the node's box, the leaf
decision and the best split (128 bins, the sweeps' order, the strict comparison, the unfused float32 cost), and which
items the left child must hold.  The other CPU tests check the rebuilt trees for structure and for the hits they
return; any valid tree passes them.  Here a builder that chose a worse split, put an item on the wrong side of a legal
split or missed the leaf rule by one fails.

Scenes: every world of custom_scene.synth_worlds but the one that holds the bunny, the sphere worlds of more than 8
spheres, the concentric clusters (20 spheres, 20 triangles: bit-equal box centres, different boxes), the rippled grids
(zero centroid extent on one axis, ties between candidates) and soups whose item counts sit at the GPU builder's
constants.  A node is halved without a best split only where its items' centres are all bit-equal (COINCIDENT).  Options: leaf sizes 1, 4, 16 and traversal costs default, 2, 8.  tests/test_gpu_sah_build.py runs the same
checker over the GPU builder's trees.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import custom_scene  # noqa: E402
import sah_model  # noqa: E402
from custom_scene import FAMILIES, ONLY, SAH_SOUP_SIZES, SAH_WORLDS, WORLDS  # noqa: E402

LEAF_SIZES = (1, 4, 16)
TRAV_COSTS = (None, 2.0, 8.0)                     # None: the option left at its default (2.0)
OPTION_SETS = {f"leaf{ls}_trav{'def' if tc is None else int(tc)}": (ls, tc) for ls in LEAF_SIZES for tc in TRAV_COSTS}
SOUPS = tuple(f"soup_{n}" for n in SAH_SOUP_SIZES)
# `interleaved` holds the bunny (69,000 items; a checker run takes 15 s): the checker is for scenes of a few thousand
# items, larger ones are compared host against GPU only (tests/test_gpu_sah_build.py)
TOO_LARGE = ("interleaved",)
CHECKED_WORLDS = tuple(w for w in FAMILIES + WORLDS + ONLY if w not in TOO_LARGE) + SAH_WORLDS + SOUPS
# Scenes in which some items' box centres are bit-equal, so that a node of them has no split candidate and is halved:
# the concentric cluster and the duplicated triangles of `ties`, built for it, but also every axis-aligned quad (its two
# triangles share one box: the Cornell walls under the sphere worlds, `planar`, the grids' cells) and the twin spheres.
# Everywhere else a halved node is a failure outright.
COINCIDENT = ("concentric", "concentric_soup", "concentric_tris", "ties", "planar", "grid8", "grid24") + WORLDS


def export_options(leaf_size, trav_cost, width=2, gpu_build=False):
    o = dict(width=width, leaf_size=leaf_size, gpu_build=gpu_build)
    if width == 2:
        o["layouts"] = 1                           # the tree as emitted from the root, child[0] first
    if trav_cost is not None:
        o["traversal_cost"] = trav_cost
    return o


def all_worlds(directory):
    """name -> scene with .export(): the synthetic worlds, the SAH worlds and the sized soups."""
    out = custom_scene.synth_worlds(custom_scene.family_files(directory))
    out.update(custom_scene.sah_worlds(directory))
    out.update({f"soup_{n}": custom_scene.SizedSoup(directory, n) for n in SAH_SOUP_SIZES})
    return out


def check_export(name, e, leaf_size, trav_cost):
    """The checker over one width-2 export; the fallback nodes it found, every one of them legitimate."""
    fb = sah_model.check_tree(e, leaf_size, 2.0 if trav_cost is None else trav_cost)
    for f in fb:
        assert f["centres_equal"], f"{name}: node {f['node']} ({f['count']} items) was halved although its centres differ"
    if name not in COINCIDENT:
        assert not fb, f"{name}: fallback nodes {[f['node'] for f in fb]} in a scene without coincident centres"
    # the vectorised detector the host-against-GPU comparison uses on scenes too large for the checker
    assert [f["node"] for f in fb] == sah_model.coincident_nodes(e).tolist()
    return fb


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    return all_worlds(tmp_path_factory.mktemp("sah"))


def test_scenes_hold_what_they_are_for(worlds):
    """Item counts at the constants, spheres inside the tree, bit-equal centres, a zero centroid extent: read from the
    exports before any decision is checked."""
    for n in SAH_SOUP_SIZES:
        w = worlds[f"soup_{n}"]
        e4, e2 = w.export("rebuilt", width=4), w.export("rebuilt", width=2, layouts=1)
        assert e4["excluded"] == 0 and e4["n_ray_spheres"] == 2
        assert e4["prim_float4s"] // 3 - e4["n_ray_spheres"] == n       # width 4: the pair is tested per ray
        assert e2["prim_float4s"] // 3 == n + 2                          # width 2: every sphere is an item
    for name, k in (("spheres9", 9), ("spheres17", 17), ("spheres40", 40), ("soup200_spheres12", 12)):
        e4 = worlds[name].export("rebuilt", width=4)
        assert e4["n_ray_spheres"] == 0, "more than 8 spheres: all of them in the tree"
        assert int(sah_model.items_of(e4)[3].sum()) == k
    assert worlds["soup200_spheres12"].export("rebuilt", width=4)["prim_float4s"] // 3 == 212
    for name, n_tri in (("concentric", 0), ("concentric_soup", 100)):
        for width in (2, 4):
            e = worlds[name].export("rebuilt", width=width)
            _, _, c, sph, _ = sah_model.items_of(e)
            assert sph.sum() == 20 and len(sph) == 20 + n_tri and e["n_ray_spheres"] == 0
            assert (c[sph].view(np.uint32) == 0).all(), "every sphere's box centre is +0 on every axis, bit for bit"
            lo, hi = sah_model.items_of(e)[:2]
            assert len(np.unique(hi[sph, 0])) == 20, "20 different boxes"
    for width in (2, 4):                               # the triangle cluster: exact only if the loader's arithmetic is
        e = worlds["concentric_tris"].export("rebuilt", width=width)
        lo, hi, c, sph, _ = sah_model.items_of(e)
        tri = ~sph
        assert tri.sum() == 20 and e["excluded"] == 2, "20 triangles; the flat floor stays out"
        assert (c[tri].view(np.uint32) == c[tri][:1].view(np.uint32)).all(), "one box centre, bit for bit"
        assert len(np.unique(hi[tri, 0])) == 20 and len(np.unique(lo[tri, 2])) == 20, "20 different boxes"
    for name, k in (("grid8", 8), ("grid24", 24)):
        e = worlds[name].export("rebuilt", width=4)
        lo, hi, c, sph, _ = sah_model.items_of(e)
        assert e["excluded"] == 0 and len(c) - e["n_ray_spheres"] == 2 * k * k
        tri = ~sph
        assert len(np.unique(c[tri, 1].view(np.uint32))) == 1, "zero centroid extent on y"
        assert (hi[tri, 1] > lo[tri, 1]).all(), "no flat box"
        assert len(np.unique(c[tri, 0])) <= 2 * k and len(np.unique(c[tri, 2])) <= 2 * k, "many equal centre coordinates"


@pytest.mark.parametrize("opts", list(OPTION_SETS))
@pytest.mark.parametrize("name", CHECKED_WORLDS)
def test_host_builder_decisions(worlds, name, opts):
    leaf_size, trav_cost = OPTION_SETS[opts]
    e = worlds[name].export("rebuilt", **export_options(leaf_size, trav_cost))
    fb = check_export(name, e, leaf_size, trav_cost)
    if name.startswith("concentric"):
        assert max(f["count"] for f in fb) == 20, "the whole cluster reaches one node and is halved there"


def test_checker_rejects_a_wrong_tree(worlds):
    """The checker is not vacuous: a tree built for another traversal cost or leaf size, and a tree with one box
    moved by an ulp, fail it."""
    e = worlds["soup"].export("rebuilt", **export_options(4, 2.0))
    sah_model.check_tree(e, 4, 2.0)
    with pytest.raises(AssertionError, match="leaf"):
        sah_model.check_tree(e, 4, 8.0)
    with pytest.raises(AssertionError, match="leaf"):
        sah_model.check_tree(e, 2, 2.0)
    bad = dict(e, nodes=e["nodes"].copy())
    row = bad["nodes"].reshape(-1, 2, 4)
    row[5, 0, 0] = np.nextafter(row[5, 0, 0], np.float32(-np.inf))
    with pytest.raises(AssertionError, match="box"):
        sah_model.check_tree(bad, 4, 2.0)
