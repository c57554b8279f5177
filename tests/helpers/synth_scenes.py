"""Deterministic synthetic OBJ + MTL scenes for the parity tests (tests/test_synth_scenes.py, tests/test_gpu_synth.py).

Every generator writes its files into a directory of the caller's (pytest's tmp_path), from a fixed seed, and returns
the OBJ file list in load order.  Both loaders accept them: crt_amd.HostScene (C++) and oracle/objload.py.  Every mesh
stays far below 2,000 triangles, so an oracle frame of the test sizes takes about a second.

Both loaders re-normalise all meshes loaded so far into a 0.6-wide cube round the origin after every file
(SceneManager.h:307-325), so a generator controls shape, not position: the `far` family is the soup again, and the
translation is applied to the loaders' output (custom_scene.CustomScene(translate=...)).

Grid-exact scenes (planar): a mesh whose x range is exactly [-0.6f, 0.6f] and whose other extents are smaller is
normalised with centre 0 and scale 0.6f / 1.2f = 0.5 exactly, so raw coordinates on the 1/32 grid land on the 1/64
grid bit for bit; a later file whose vertices lie inside the normalised bounds leaves centre 0 and scale 1.
"""
import os

import numpy as np

EDGE = "0.60000002384185791015625"      # float32(0.6), the raw half-extent that makes the normalisation exact

MTL = """newmtl white
Kd 0.73 0.73 0.73
newmtl red
Kd 0.65 0.05 0.05
newmtl lamp
Kd 0 0 0
Ke 6 5 4
newmtl glass
Kd 1 1 1
d 0.5
Ni 1.5
newmtl steel
Kd 0.8 0.85 0.9
Ks 0.9 0.9 0.9
Ns 200
"""
MATERIALS = ("white", "red", "lamp", "glass", "steel")
SHARES = (0.40, 0.22, 0.08, 0.15, 0.15)


def _fmt(x):
    return x if isinstance(x, str) else "%.9g" % x


def write_obj(directory, name, verts, faces, mtl=MTL):
    """verts: rows of 3 numbers (or strings, written verbatim); faces: (i, j, k, material name or None), 0-based.
    Returns the OBJ path; the MTL is written next to it as <name>.mtl."""
    lines = []
    if mtl is not None:
        with open(os.path.join(directory, name + ".mtl"), "w") as f:
            f.write(mtl)
        lines.append(f"mtllib {name}.mtl\n")
    lines += ["v %s %s %s\n" % tuple(_fmt(c) for c in v) for v in verts]
    cur = object()
    for i, j, k, m in faces:
        if m != cur and m is not None:
            lines.append(f"usemtl {m}\n")
            cur = m
        lines.append("f %d %d %d\n" % (i + 1, j + 1, k + 1))
    path = os.path.join(directory, name + ".obj")
    with open(path, "w") as f:
        f.write("".join(lines))
    return path


def _soup_arrays(seed, n, spread=0.16):
    """n random triangles with centroids in [-1, 1]^3 (float32 vertices) and a material name each."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 3))
    v = (c[:, None, :] + rng.normal(scale=spread, size=(n, 3, 3))).astype(np.float32)
    mats = rng.choice(len(MATERIALS), n, p=SHARES)
    return v, [MATERIALS[m] for m in mats], rng


def _soup_faces(v, mats):
    verts = v.reshape(-1, 3)
    return verts, [(3 * t, 3 * t + 1, 3 * t + 2, mats[t]) for t in range(len(v))]


def soup(directory, seed=101, n=600, name="soup"):
    """A random triangle soup filling the normalised cube, five materials (two diffuse, emissive, dielectric,
    metal): a wrong hit changes the colour."""
    v, mats, _ = _soup_arrays(seed, n)
    verts, faces = _soup_faces(v, mats)
    return [write_obj(directory, name, verts, faces)]


def ties(directory, seed=202, n=500):
    """The soup with about 10 % exact duplicates: every duplicate repeats another triangle's three vertices in the
    same order (bit-identical records, hence exactly equal t for every ray) under a different material.  Pairs and
    triples; a duplicate lands before or after its original in the face list; half the duplicates share the
    original's vertex entries, half repeat them as new `v` lines.  At most three coincident centroids, far below
    the ten a leaf of the sequential mesh builder holds, so its stack cap is not reached."""
    v, mats, rng = _soup_arrays(seed, n)
    verts = [tuple(p) for p in v.reshape(-1, 3)]
    faces = [[3 * t, 3 * t + 1, 3 * t + 2, mats[t], t] for t in range(n)]     # last: the original's number
    originals = rng.choice(n, n // 15, replace=False)
    dup = []
    for q, t in enumerate(originals):
        for copy in range(1 + q % 2):                       # pairs and triples alternate
            other = MATERIALS[(MATERIALS.index(mats[t]) + 1 + copy) % len(MATERIALS)]
            if (q + copy) % 2:
                idx = [3 * t, 3 * t + 1, 3 * t + 2]
            else:
                idx = [len(verts), len(verts) + 1, len(verts) + 2]
                verts += verts[3 * t:3 * t + 3]
            dup.append(idx + [other, int(t)])
    for q, f in enumerate(dup):
        at = [k for k, g in enumerate(faces) if g[4] == f[4]][0]
        faces.insert(at if q % 2 else int(rng.integers(at + 1, len(faces) + 1)), f)
    return [write_obj(directory, "ties", verts, [tuple(f[:4]) for f in faces])]


def degenerate(directory, seed=303, n=450, each=20):
    """The soup plus three kinds of zero-area triangle, `each` of a kind: two equal vertices, three collinear
    vertices, and needles of edge ratio 1e6."""
    v, mats, rng = _soup_arrays(seed, n)
    extra = []
    for kind in range(3):
        for _ in range(each):
            a = rng.uniform(-0.9, 0.9, 3)
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            w = np.cross(u, rng.normal(size=3))
            w /= np.linalg.norm(w)
            if kind == 0:
                tri = [a, a + 0.3 * u, a]
            elif kind == 1:
                tri = [a, a + 0.25 * u, a + 0.5 * u]       # float32 rounding may leave it a sliver: still degenerate
            else:
                tri = [a, a + 0.5 * u, a + 0.5e-6 * w]
            extra.append(np.asarray(tri, np.float32))
    at = rng.choice(n, len(extra), replace=False)            # interleaved with the soup, not appended
    tris, names = list(v), list(mats)
    for k, tri in zip(sorted(at.tolist(), reverse=True), extra):
        tris.insert(k, tri)
        names.insert(k, MATERIALS[k % len(MATERIALS)])
    verts, faces = _soup_faces(np.asarray(tris, np.float32), names)
    return [write_obj(directory, "degenerate", verts, faces)]


def planar(directory, seed=404):
    """Axis-aligned quads on an exact grid (1/32 raw, 1/64 once normalised): stacks of horizontal quads, some coplanar
    and overlapping with different materials, vertical quads in both other orientations, on a floor whose x range
    makes the normalisation exact (module docstring).  Their reference boxes have zero thickness.  The second file is
    a mesh of one triangle, on the 1/64 grid inside the first mesh's normalised bounds.

    Horizontal quads lie on even grid levels (y = 0 among them), the edges of vertical quads on odd ones.  A ray that runs exactly in a
    horizontal quad's plane (tests' in-plane camera) then crosses no vertical quad along its edge.  Such an edge hit is a
    genuine one (Moller-Trumbore accepts u = 0 or v = 0) which the reference loses: with the ray's origin on a face of
    an enclosing box and a zero direction component, AABB::hit computes 0 * inf = NaN there and culls the subtree.  The
    rebuilt tree keeps the hit, so on such a plane the two legitimately differ on up to a fifth of the primary rays
    (DESIGN.md section 4b); the scene is laid out so that the comparison stays a check of the tree."""
    rng = np.random.default_rng(seed)
    verts, faces = [], []

    def quad(p, du, dv, m):
        b = len(verts)
        p, du, dv = (np.asarray(x, np.float64) for x in (p, du, dv))
        verts.extend([tuple(p), tuple(p + du), tuple(p + du + dv), tuple(p + dv)])
        faces.extend([(b, b + 1, b + 2, m), (b, b + 2, b + 3, m)])

    b = len(verts)                                           # the floor: x in [-0.6f, 0.6f]
    verts.extend([("-" + EDGE, -0.5, -0.5), (EDGE, -0.5, -0.5), (EDGE, -0.5, 0.5), ("-" + EDGE, -0.5, 0.5)])
    faces.extend([(b, b + 1, b + 2, "white"), (b, b + 2, b + 3, "white")])
    g = 1.0 / 32
    for _ in range(60):
        axis = int(rng.integers(0, 3))
        others = [a for a in range(3) if a != axis]
        p = np.zeros(3)
        p[axis] = g * int(rng.integers(-12, 13))             # few distinct planes: many quads share one exactly
        if axis == 1:
            p[axis] = g * 2 * int(rng.integers(-7, 4))        # horizontal quads on even levels (below), under the lamp
        du, dv = np.zeros(3), np.zeros(3)
        for a, e in zip(others, (du, dv)):
            size = int(rng.integers(2, 9))
            start = int(rng.integers(-15, 15 - size))
            if a == 1:                                        # vertical quads begin and end on odd levels
                size = 2 * int(rng.integers(1, 5))            # below the lamp: the floor and the lamp bound y
                start = 2 * int(rng.integers(-7, (6 - size) // 2 + 1)) + 1
            p[a] = g * start
            e[a] = g * size
        quad(p, du, dv, MATERIALS[int(rng.integers(0, len(MATERIALS)))])
    quad((-0.25, 0.25, -0.25), (0.5, 0, 0), (0, 0, 0.5), "lamp")        # a light over the stacks
    first = write_obj(directory, "planar", verts, faces)
    k = 1.0 / 64
    one = write_obj(directory, "single", [(-8 * k, 2 * k, 3 * k), (9 * k, 5 * k, -2 * k), (1 * k, 10 * k, 6 * k)],
                    [(0, 1, 2, "red")])
    return [first, one]


def many_meshes(directory, seed=505, files=12):
    """Twelve OBJ files of 8-50 triangles, each a cluster of its own with its own MTL: a scene-level BVH several
    levels deep, and the materialIDOffset quirk (the previous mesh's unique-material count) on every file."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(files):
        n = int(rng.integers(8, 51))
        centre = rng.uniform(-0.8, 0.8, 3)
        c = centre + rng.uniform(-0.25, 0.25, (n, 3))
        v = (c[:, None, :] + rng.normal(scale=0.12, size=(n, 3, 3))).astype(np.float32)
        mats = [MATERIALS[(k + int(m)) % len(MATERIALS)] for m in rng.integers(0, 3, n)]
        verts, faces = _soup_faces(v, mats)
        out.append(write_obj(directory, f"part{k:02d}", verts, faces))
    return out


def far(directory, seed=606, n=600):
    """The soup of another seed; the tests translate the loaded scene by FAR_OFFSET (module docstring)."""
    return soup(directory, seed, n, name="far")


FAR_OFFSET = (1000.0, 1000.0, -1000.0)


def sized_soup(directory, n, seed=707):
    """The soup recipe with exactly n triangles (file soup_<n>.obj): item counts at the builders' constants."""
    return soup(directory, seed, n, name=f"soup_{n}")


def grid_arrays(k, ripple=0.0):
    """A regular k x k quad grid in the plane y = 0 with shared vertices: ((k + 1)^2 vertices float32, 2 k^2 faces
    as vertex index triples).  Every column and every row of cells repeats its x and z box bounds, so many centroid
    coordinates are equal and many SAH candidates tie.

    ripple = 0: planar, every box has zero y thickness (the mesh builder's case; the reference's own box test never
    enters such a box, so through a scene every triangle would be unreachable).  ripple = h > 0: vertex (i, j) lies at
    y = +h where i + j is even and at -h where it is odd.  Every triangle then spans y in [-h, h] exactly, so every
    box centre is 0.5f * -h' + 0.5f * h' = 0 on y (h' the normalised h: the loaders centre y on 0 exactly), the
    centroid extent of that axis is zero, and no box is flat."""
    i, j = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing="ij")
    y = np.where((i + j) % 2 == 0, ripple, -ripple)
    verts = np.stack([i / k - 0.5, y, j / k - 0.5], -1).reshape(-1, 3).astype(np.float32)
    at = lambda a, b: a * (k + 1) + b                                   # noqa: E731
    faces = []
    for a in range(k):
        for b in range(k):
            faces += [(at(a, b), at(a + 1, b), at(a + 1, b + 1)), (at(a, b), at(a + 1, b + 1), at(a, b + 1))]
    return verts, np.asarray(faces, np.uint32)


def concentric_triangles(directory, n=20):
    """n copies of one triangle scaled about its box centre by (k + 1) / 32, on a floor whose x range makes the
    normalisation exact (module docstring): every raw coordinate is a small multiple of 1/256, the normalisation's
    centre is such a number too and its scale 0.5, so every box is C -/+ h_k with exactly representable bounds and every
    box centre 0.5f * lo + 0.5f * hi is C bit for bit, while the n boxes all differ.  The triangle has a vertex at
    each end of its box on every axis; the vertex means differ, so the sequential mesh builder splits them as usual.
    The flat floor is unreachable for the reference's box test and stays out of the rebuilt tree."""
    verts = [("-" + EDGE, -0.5, -0.5), (EDGE, -0.5, -0.5), (EDGE, -0.5, 0.5), ("-" + EDGE, -0.5, 0.5)]
    faces = [(0, 1, 2, "white"), (0, 2, 3, "white")]
    for k in range(n):
        s = (k + 1) / 32
        x, y, z = s / 4, s / 8, s * 3 / 16
        b = len(verts)
        verts += [(-x, -y, -z), (x, y, -z), (0.0, y, z)]
        faces.append((b, b + 1, b + 2, MATERIALS[k % len(MATERIALS)]))
    return [write_obj(directory, "concentric_tris", verts, faces)]


def grid(directory, k, ripple=0.03125):
    """grid_arrays as an OBJ file (grid_<k>.obj), materials cycling."""
    verts, faces = grid_arrays(k, ripple)
    return [write_obj(directory, f"grid_{k}", verts,
                      [(int(f[0]), int(f[1]), int(f[2]), MATERIALS[(t // 2) % len(MATERIALS)]) for t, f in enumerate(faces)])]


# ---------------------------------------------------------------------------------------------- sphere worlds
# material rows for spheres (custom_scene.mat_row layout): grey and green diffuse, fuzzy metal, glass, a light
SPHERE_MATS = [[0.0, 0.5, 0.5, 0.5, 0, 0, 0, 0.0, 1.0], [0.0, 0.1, 0.6, 0.15, 0, 0, 0, 0.0, 1.0],
               [1.0, 0.8, 0.7, 0.4, 0, 0, 0, 0.2, 1.0], [2.0, 1.0, 1.0, 1.0, 0, 0, 0, 0.0, 1.5],
               [3.0, 0.0, 0.0, 0.0, 4.0, 4.0, 3.0, 0.0, 1.0]]
GROUND = ((0.0, -1000.0, 0.0), 999.0, 0)


def random_spheres(n, seed=7, lo=0.02, hi=0.08):
    """n spheres inside the normalised scene cube, mixed radii, materials cycling through SPHERE_MATS."""
    rng = np.random.default_rng(seed)
    return [(tuple(float(x) for x in np.float32(rng.uniform(-0.22, 0.22, 3))), float(np.float32(rng.uniform(lo, hi))),
             k % len(SPHERE_MATS)) for k in range(n)]


def sphere_worlds(floor_y=-0.3):
    """name -> (spheres, order or None, needs two meshes).  order None = meshes first, then the spheres.

    floor_y: the y of the mesh's lowest vertex, for the sphere that touches that plane exactly."""
    r = np.float32(0.0625)
    cy = np.float32(np.float32(floor_y) + r)
    assert np.float32(cy - r) == np.float32(floor_y), "c.y - r must give the plane back exactly"
    three = random_spheres(3, seed=11)
    return {
        "s0": ([], None, False),
        "s1": ([((0.1, -0.1, 0.05), 0.08, 3)], None, False),
        "s3": (three, None, False),
        "s8": (random_spheres(8, seed=12), None, False),
        "s3_ground": (random_spheres(2, seed=15) + [GROUND], None, False),
        "s9_ground": (random_spheres(8, seed=13) + [GROUND], None, False),
        "s40": (random_spheres(40, seed=14, lo=0.01, hi=0.05), None, False),
        "before": (three, [(1, 0), (1, 1), (1, 2), (0, 0)], False),
        "interleaved": (three, [(1, 0), (0, 0), (1, 1), (0, 1), (1, 2)], True),
        "twins": ([((0.05, -0.05, 0.0), 0.09, 2), ((0.05, -0.05, 0.0), 0.09, 1), ((-0.15, 0.1, -0.1), 0.05, 3)],
                  None, False),
        "tangent": ([((0.0, float(cy), 0.0), float(r), 2), ((-0.1, 0.1, 0.05), 0.04, 0)], None, False),
    }


def concentric_spheres(n=20):
    """n spheres centred exactly at the origin, n distinct radii (largest 0.2): every box is -r .. r, so every box
    centre is exactly 0 on every axis, and the boxes all differ.  More than the GPU builder's small-node limit of 16."""
    return [((0.0, 0.0, 0.0), float(np.float32(0.01 * (k + 1))), k % len(SPHERE_MATS)) for k in range(n)]


SPHERES_ONLY = {"only3": random_spheres(3, seed=21, lo=0.05, hi=0.12),
                "only12": random_spheres(12, seed=22, lo=0.03, hi=0.1)}
