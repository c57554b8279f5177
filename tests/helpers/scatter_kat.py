"""Known-answer records of the scatter step (tests/golden/scatter_kat.npz): generator, census and the device's view.

One record is one hand-made hit of one path: a ray, a hit record, a material of the fixture's table, a throughput, a
bounce count, a bounce limit and an XORWOW state.  The oracle (pyoracle.kat_scatter) runs it through one iteration of
rayColor's loop in two stages: A after the scatter / emission / sky, B after the next iteration's head (bounce limit,
Russian roulette).  Stage B is what scatter_step() of crt_paths.h and shade_rec() + next_ray() of crt_hip.hip return.

The records are built class by class (CLASSES below) with a fixed seed.  Where a class needs particular uniform draws
the generator's state is solved for them: XORWOW's output k is  f(v4_{k-1}) ^ g(v_{k-1}) + d + k * 362437  with
f(x) = x ^ (x << 4) and g(v) = T(S(v)), S(v) = v ^ (v >> 2), T(t) = t ^ (t << 1); S and T are invertible, so with v4
and d fixed the words v0..v3 give any four first outputs (state_for_draws).  tests/test_scatter_kat.py checks the
inversion against pyoracle.rng_draw.

Fixture arrays (uint32 words unless stated):
  mats   (M, 9)      the material table: type, albedo3, emission3, roughness, ior (float bits)
  rows   (M, 2, 4)   the per-material rows the step kernel reads for that table (shade_rows_of)
  rec    (n, 24)     o3 d3 t | outward normal3 front | material | throughput3 bounce max_bounces | rng6 | status
                     material: index into mats; M stands for "the scene's material count", -1 for -1
  lin    (n, 3)      the sum of the record's pixel before the step
  out    (n, 2, 20)  the oracle's stages: ended | o3 d3 | throughput3 | bounce | add3 | rng6
  draws  (n, 2)      int32: generator outputs used up to each stage
  label  (n,)        bytes: the record's class
"""
import io
import zipfile

import numpy as np

F32, U32 = np.float32, np.uint32
STEP = 362437                       # XORWOW's Weyl increment
SEED = 20240607
ACTIVE, ENDED = 0, 1                # crt_path.status
REC_WORDS = 24
O, D, T, NRM, FRONT, MAT, THR, BOUNCE, MAXB, RNG, STATUS = (slice(0, 3), slice(3, 6), 6, slice(7, 10), 10, 11,
                                                             slice(12, 15), 15, 16, slice(17, 23), 23)
# columns of a stage
S_ENDED, S_O, S_D, S_THR, S_BOUNCE, S_ADD, S_RNG = 0, slice(1, 4), slice(4, 7), slice(7, 10), 10, slice(11, 14), slice(14, 20)
NAN_BITS = 0x7fc00000


def canon(a):
    """uint32 view with every NaN mapped to one pattern (as denoise_model.canon)."""
    a = np.ascontiguousarray(a)
    f = a.view(F32)
    out = a.view(U32).copy()
    out[np.isnan(f)] = NAN_BITS
    return out


def bits(x):
    return np.asarray(x, F32).view(U32)


# ------------------------------------------------------------------------------------------ XORWOW, solved for draws
def _inv_s(y):                      # v from v ^ (v >> 2)
    v = y
    for k in (2, 4, 8, 16):
        v ^= v >> k
    return v & 0xffffffff


def _inv_t(y):                      # t from t ^ (t << 1)
    t = y
    for k in (1, 2, 4, 8, 16):
        t = (t ^ (t << k)) & 0xffffffff
    return t


def state_for_draws(x, v4, d):
    """The state (v0..v4, d) whose first len(x) <= 4 outputs are x; words not needed are 0."""
    f = lambda w: (w ^ (w << 4)) & 0xffffffff   # noqa: E731
    v, prev = [0, 0, 0, 0], int(v4)
    for k, xk in enumerate(x):
        new = (int(xk) - (int(d) + (k + 1) * STEP)) & 0xffffffff       # v4 after draw k + 1
        v[k] = _inv_s(_inv_t(new ^ f(prev)))
        prev = new
    return np.array([*v, int(v4), int(d)], U32)


def uniform_of(x):
    """curand_uniform of the output word x: fl(float(x) * 2^-32 + 2^-33), exact in float64 before the one rounding."""
    return F32(np.float64(F32(U32(x))) * 2.0 ** -32 + 2.0 ** -33)


def draw_le(u):
    """The largest output word whose uniform is <= u (u a float32 in (0, 1])."""
    lo, hi = 0, 0xffffffff
    assert uniform_of(lo) <= u
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if uniform_of(mid) <= u:
            lo = mid
        else:
            hi = mid - 1
    return lo


def draw_gt(u):
    """The smallest output word whose uniform is > u."""
    x = draw_le(u) + 1
    assert x <= 0xffffffff and uniform_of(x) > u
    return x


HALF, QUARTER, THREE_Q = 1 << 31, 1 << 30, 3 << 30      # uniforms 0.5, 0.25, 0.75: rand_range(-1, 1) = 0, -0.5, +0.5
ONE = 0xffffffff                                        # uniform 1.0


# ------------------------------------------------------------------------------------------ the material rows
def shade_rows_of(mats):
    """material_shade_row of crt_scene.h in float32: (code, 0, 0, 0) (payload) per row of the table."""
    mats = np.asarray(mats, F32).reshape(-1, 9)
    rows = np.zeros((len(mats), 2, 4), F32)
    for k, m in enumerate(mats):
        kind = int(m[0])
        code = kind if kind in (0, 1, 2, 3) else 4
        rows[k, 0, 0] = np.array([code], np.int32).view(F32)[0]
        if code == 0:
            rows[k, 1, :3] = m[1:4]
        elif code == 1:
            rows[k, 1, :3] = m[1:4]
            rows[k, 1, 3] = m[7] if m[7] < 1 else F32(1)
        elif code == 2:
            r0 = lambda r: F32(F32(F32(1) - r) / F32(F32(1) + r)) ** 2     # noqa: E731
            with np.errstate(all="ignore"):
                inv = F32(F32(1) / m[8])
                rows[k, 1] = [m[8], inv, F32(r0(inv)), F32(r0(m[8]))]
        elif code == 3:
            rows[k, 1, :3] = m[4:7]
    return rows


def schlick_f32(c, ri):
    """Dielectric::schlicksReflectance in float32 operation order (pow(float, 5) by squaring)."""
    c, ri = F32(c), F32(ri)
    r0 = F32(F32(F32(1) - ri) / F32(F32(1) + ri))
    r0 = F32(r0 * r0)
    a = F32(F32(1) - c)
    r = a
    a = F32(a * a)
    a = F32(a * a)
    r = F32(r * a)
    return F32(r0 + F32(F32(F32(1) - r0) * r))


# ------------------------------------------------------------------------------------------ the generator
class _Builder:
    def __init__(self, seed):
        self.g = np.random.default_rng(seed)
        self.mats, self.mat_key = [], {}
        self.rec, self.lin, self.label = [], [], []
        self.k_state = 0

    def mat(self, kind, albedo=(0, 0, 0), emission=(0, 0, 0), roughness=0.0, ior=1.0):
        row = np.array([kind, *albedo, *emission, roughness, ior], F32)
        key = row.view(U32).tobytes()
        if key not in self.mat_key:
            self.mat_key[key] = len(self.mats)
            self.mats.append(row)
        return self.mat_key[key]

    def init_state(self):
        import pyoracle
        self.k_state += 1
        return pyoracle.rng_init(41, 1000 + self.k_state)

    def crafted(self, *x):
        v4, d = self.g.integers(1, 2 ** 32, 2, dtype=np.uint64)
        return state_for_draws(x, v4, d)

    def add(self, label, d, outward, front, mat, *, o=None, t=1.0, thr=None, bounce=0, maxb=20, rng=None, status=ACTIVE):
        g = self.g
        r = np.zeros(REC_WORDS, U32)
        r[O] = bits(g.uniform(-0.3, 0.3, 3) if o is None else o)
        r[D] = bits(d)
        r[T] = bits(t)
        r[NRM] = bits(outward)
        r[FRONT] = int(bool(front))
        r[MAT] = np.array([mat], np.int32).view(U32)[0]
        r[THR] = bits(1.0 - g.uniform(0, 1, 3) if thr is None else thr)
        r[BOUNCE], r[MAXB] = bounce, maxb
        r[RNG] = self.init_state() if rng is None else rng
        r[STATUS] = status
        self.rec.append(r)
        self.lin.append(bits(g.uniform(0.25, 4, 3)))
        self.label.append(label)
        return len(self.rec) - 1


def _unit64(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _len2_f32(v):
    v = np.asarray(v, F32)
    return F32(F32(F32(v[0] * v[0]) + F32(v[1] * v[1])) + F32(v[2] * v[2]))


def band_search(seed, n=1 << 22):
    """Pairs (c, ior) for the back face of a glass hit with z = ior^2 * (1 - c^2) next to 1: ior = fl(1 / sqrt(1 - c^2))
    and a direction (fl(sqrt(1 - c^2)), 0, -c) of float32 length exactly 1, so unit(d) == d and the device sees c itself.
    Returns c, s, ior, z and the reference's float64 test ri * sqrt(1 - c^2) > 1, candidates in their seeded order."""
    g = np.random.default_rng(seed)
    c = g.uniform(0.3, 0.9, n).astype(F32)
    c64 = c.astype(np.float64)
    y = 1.0 - c64 * c64                                     # c * c is exact in float64: one rounding, as the fma
    s = np.sqrt(y).astype(F32)
    ior = (1.0 / np.sqrt(y)).astype(F32)
    one = (F32(s * s) + F32(0)).astype(F32) + (c * c).astype(F32)
    ok = one.astype(F32) == F32(1)
    r = ior.astype(np.float64)
    z = (r * r) * y
    tir = r * np.sqrt(y) > 1.0
    return c[ok], s[ok], ior[ok], z[ok], tir[ok]


def build_inputs(seed=SEED):
    """(mats, rec, lin, label) of every class, before the oracle has seen them."""
    b = _Builder(seed)
    g = b.g
    nan = float("nan")
    Z, NZ = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)

    lam = [b.mat(0, a) for a in ((0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15))]
    met = [b.mat(1, (0.7, 0.6, 0.5), roughness=r) for r in (0.0, 0.3, 1.0)]
    gla = [b.mat(2, ior=i) for i in (1.5, 1.33, 2.4)]
    light = b.mat(3, emission=(15.0, 14.0, 13.0))
    unknown = b.mat(7, (0.3, 0.3, 0.3), (2.0, 2.0, 2.0))
    by_code = [lam, met, gla, [light], [unknown]]

    # ---- general position: every code, both faces, unit and non-unit directions, bounces 0..19, some misses
    for i in range(448):
        d = _unit64(g.normal(size=3))
        if i % 2:
            d = d * 10.0 ** g.uniform(-2, 2)
        nrm = _unit64(g.normal(size=3))
        code = i % 5
        mat = by_code[code][int(g.integers(len(by_code[code])))]
        miss = i % 11 == 10
        b.add("general", d, nrm, np.dot(d, nrm) < 0, mat, t=-1.0 if miss else g.uniform(0.01, 5.0), bounce=i % 20)

    # ---- the glass band: back face, so ri = ior; the first draw of half the open ones is 1.0 (always refracts)
    c, s, ior, z, tir = band_search(seed + 1)
    dist = np.abs(z - 1.0)
    inband = dist < 2.0 ** -40
    near = (dist >= 2.0 ** -40) & (dist < 2.0 ** -34)
    for name, sel, cap in (("band_tir", inband & tir, 12), ("band_open", inband & ~tir, 12),
                           ("band_near", near & (z > 1), 12), ("band_near", near & (z < 1), 12)):
        for n_done, k in enumerate(np.nonzero(sel)[0][:cap]):
            m = b.mat(2, ior=ior[k])
            rng = b.crafted(ONE) if n_done % 2 else None
            b.add(name, (s[k], 0.0, -c[k]), NZ, 0, m, bounce=1, rng=rng)

    # ---- glass edges
    up1 = np.nextafter(F32(1), F32(2))                       # 1 + 2^-23
    for front, outward in ((1, Z), (0, NZ)):
        b.add("glass_cos1", (0.0, 0.0, -1.0), outward, front, gla[0])
        b.add("glass_cos0", (1.0, 0.0, 0.0), outward, 0, gla[0])         # dot(d, outward) = 0 is not a front face
        sgn = 1.0 if front else -1.0
        b.add("glass_cos_gt1", (0.0, 0.0, -1.0), (0.0, 0.0, sgn * up1), front, gla[0])
        b.add("glass_cos_gt1", (0.0, 0.0, -1.0), (0.0, 0.0, sgn * up1), front, gla[0], rng=b.crafted(ONE))
        b.add("glass_ior1", (0.6, 0.0, -0.8), outward, front, b.mat(2, ior=1.0))
        b.add("glass_ior1", (0.6, 0.0, -0.8), outward, front, b.mat(2, ior=1.0), rng=b.crafted(ONE))
        b.add("glass_nan_normal", (0.6, 0.0, -0.8), (nan, 0.0, sgn), front, gla[0])
    # the Schlick draw on either side of equality: three angles whose (s, 0, -c) has float32 length 1, both faces
    cs, ss, _, _, _ = band_search(seed + 2, 1 << 12)
    for target in (0.8, 0.85, 0.9):
        k = int(np.argmin(np.abs(cs - F32(target))))
        ck, sk = cs[k], ss[k]
        for front, outward in ((1, Z), (0, NZ)):
            ri = F32(F32(1) / F32(1.5)) if front else F32(1.5)
            val = schlick_f32(ck, ri)
            le = draw_le(val)
            xs = [(le, uniform_of(le) < val), (draw_gt(val), False)]
            if uniform_of(le) == val:                       # equality itself refracts; the draw below it reflects
                below = draw_le(np.nextafter(val, F32(0)))
                xs.append((below, True))
            for x, reflects in xs:
                b.add("schlick_reflect" if reflects else "schlick_refract", (sk, 0.0, -ck), outward, front, gla[0],
                      rng=b.crafted(x))

    # ---- Lambert: unit(q) == -n for the six axis normals and both faces; neighbours; a rejected first triple
    for axis in range(3):
        for sign in (1.0, -1.0):
            n = np.zeros(3)
            n[axis] = sign
            x = [HALF, HALF, HALF, int(g.integers(2 ** 32))]
            x[axis] = QUARTER if sign > 0 else THREE_Q
            tangent = np.roll(n, 1) * 0.25
            for front in (1, 0):
                b.add("lambert_degenerate", -n + tangent, n if front else -n, front, lam[axis], rng=b.crafted(*x))
    for which in (0, 1):
        for word in (HALF - 128, HALF + 256):                # a = -2^-24, +2^-23 in one component
            x = [HALF, HALF, QUARTER, int(g.integers(2 ** 32))]
            x[which] = word
            b.add("lambert_neighbour", (0.1, 0.2, -1.0), Z, 1, lam[0], rng=b.crafted(*x))
    for k in range(3):
        top = 0xffffff00                                     # uniform 1.0 - 2^-24: (a, b, c) ~ (1, 1, 1), rejected
        b.add("lambert_rejected", (0.1, 0.2, -1.0), Z, 1, lam[k], rng=b.crafted(top, top, top, int(g.integers(2 ** 32))))

    # ---- metal
    below = (QUARTER, THREE_Q)                               # q.z = -0.5 / +0.5; the shading normal is +z on both faces
    for front, outward in ((1, Z), (0, NZ)):
        for _ in range(2):                                   # dot(d, outward) = 0 is not a front face: n = -outward
            b.add("metal_tangent", (1.0, 0.0, 0.0), outward, 0, met[0])
        b.add("metal_tangent", (0.0, 3.0, 0.0), outward, 0, met[0])
        anti = b.crafted(HALF, HALF, below[0], 0)
        b.add("metal_cancel", (0.0, 0.0, -1.0), outward, front, met[2], rng=anti)
        b.add("metal_below", (ss[3], 0.0, -cs[3]), outward, front, met[2], rng=anti)
        b.add("metal_kept", (ss[3], 0.0, -cs[3]), outward, front, met[2], rng=b.crafted(HALF, HALF, below[1], 0))
        for r in (1.5, nan):
            m = b.mat(1, (0.9, 0.8, 0.7), roughness=r)
            for _ in range(2):
                b.add("metal_clamp", (0.5, 0.3, -0.8), outward, front, m)

    # ---- the roulette and the bounce limit: after an invalid material (first draw) and after a white Lambert hit on
    # n = +y with q = (0, 0, -0.5) (fourth draw)
    white = b.mat(0, (1.0, 1.0, 1.0))
    p95 = draw_le(F32(0.95))
    assert uniform_of(HALF) == F32(0.5) and uniform_of(p95) == F32(0.95) and uniform_of(0) == F32(2.0 ** -33)

    def both(label, x, thr, bounce=5, maxb=20):
        b.add(label, (0.3, -1.0, 0.2), (0.0, 1.0, 0.0), 1, -1, thr=thr, bounce=bounce, maxb=maxb,
              rng=None if x is None else b.crafted(x))
        b.add(label, (0.3, -1.0, 0.2), (0.0, 1.0, 0.0), 1, white, thr=thr, bounce=bounce, maxb=maxb,
              rng=None if x is None else b.crafted(HALF, HALF, QUARTER, x))

    both("roulette_at_p", HALF, (0.5, 0.25, 0.125))
    both("roulette_above_p", HALF + 256, (0.5, 0.25, 0.125))
    both("roulette_at_p", p95, (0.97, 0.99, 0.2))
    both("roulette_above_p", draw_gt(F32(0.95)), (0.97, 0.99, 0.2))
    both("roulette_tiny_p", 0, (1e-9, 1e-10, 0.0))
    both("roulette_tiny_p_ends", 8, (1e-9, 1e-10, 0.0))
    both("roulette_zero_p", 0, (0.0, 0.0, 0.0))
    both("roulette_nan", HALF, (nan, 0.5, 0.25))
    both("roulette_nan", None, (nan, nan, nan))
    both("roulette_first", None, (1.0, 1.0, 1.0), bounce=2)
    both("roulette_none", None, (0.5, 0.25, 0.125), bounce=1)
    both("limit_20", None, (0.5, 0.25, 0.125), bounce=19)
    both("limit_1", None, (1.0, 1.0, 1.0), bounce=0, maxb=1)

    # ---- directions of extreme length, on the sky, glass and metal
    shape = np.array([0.48, -0.6, -0.64])                    # towards the surface; the zero direction faces nothing
    for label, scale in (("dir_tiny", 1e-17), ("dir_huge", 3e19), ("dir_big", 1e19), ("dir_zero", 0.0)):
        d = (shape * scale).astype(F32)
        if label == "dir_tiny":
            assert 0 < _len2_f32(d) < F32(2.0 ** -100)
        if label == "dir_huge":
            with np.errstate(over="ignore"):
                assert np.isinf(_len2_f32(d))
        if label == "dir_big":
            assert np.isfinite(_len2_f32(d))
        front = bool(d[2] < 0)
        b.add(label, d, Z, front, lam[0], t=-1.0)
        b.add(label, d, Z, front, gla[0], o=(0.0, 0.0, 0.0), t=0.5)
        b.add(label, d, Z, front, met[1], o=(0.0, 0.0, 0.0), t=0.5)

    # ---- the rest
    M = None                                                 # the table's length, known at the end: patched below
    b.add("misc_miss", (0.2, 0.9, -0.3), Z, 0, lam[0], t=-1.0)
    b.add("misc_miss", (0.2, -0.9, -0.3), (0.0, 0.0, 0.0), 0, -1, t=-0.0001)
    b.add("misc_light", (0.0, 1.0, 0.1), (0.0, -1.0, 0.0), 1, light)
    b.add("misc_light", (0.0, 1.0, 0.1), (0.0, 1.0, 0.0), 0, light, bounce=7)
    b.add("misc_unknown", (0.0, 1.0, 0.1), (0.0, -1.0, 0.0), 1, unknown)
    b.add("misc_unknown", (0.0, 1.0, 0.1), (0.0, -1.0, 0.0), 1, b.mat(-1))
    past = [b.add("misc_index_n", (0.0, 1.0, 0.1), (0.0, -1.0, 0.0), 1, 0, bounce=k) for k in (0, 4)]
    for k in (0, 4):
        b.add("misc_index_neg", (0.0, 1.0, 0.1), (0.0, -1.0, 0.0), 1, -1, bounce=k)
    for m in (lam[0], met[1], gla[0], gla[2]):               # the flag is taken as stored
        b.add("misc_front_flip", (0.6, 0.0, -0.8), Z, 0, m)
        b.add("misc_front_flip", (0.6, 0.0, -0.8), NZ, 1, m)
    for m in (lam[0], met[1], gla[0], light, -1):
        b.add("misc_ended_in", (0.6, 0.0, -0.8), Z, 1, m, status=ENDED)

    M = len(b.mats)
    for k in past:
        b.rec[k][MAT] = M
    return (np.array(b.mats, F32).view(U32), np.array(b.rec, U32), np.array(b.lin, U32),
            np.array(b.label, dtype="S24"))


def oracle_records(mats, rec):
    """The (n, 32) records pyoracle.kat_scatter takes, from the fixture's."""
    M = len(mats)
    n = len(rec)
    out = np.zeros((n, 32), U32)
    out[:, 0:11] = rec[:, 0:11]
    idx = rec[:, MAT].view(np.int32)
    valid = (idx >= 0) & (idx < M)
    out[:, 11:20] = np.where(valid[:, None], mats[np.clip(idx, 0, M - 1)], 0)
    out[:, 20] = ~valid
    out[:, 21:24] = rec[:, THR]
    out[:, 24], out[:, 25] = rec[:, BOUNCE], rec[:, MAXB]
    out[:, 26:32] = rec[:, RNG]
    return out


def build_fixture(seed=SEED):
    import pyoracle
    mats, rec, lin, label = build_inputs(seed)
    out, draws = pyoracle.kat_scatter(oracle_records(mats, rec))
    assert draws.max() <= 64, f"a record used {draws.max()} draws"
    fx = {"mats": mats, "rows": shade_rows_of(mats.view(F32)).view(U32), "rec": rec, "lin": lin, "out": out,
          "draws": draws, "label": label}
    missing = census_missing(fx)
    assert not missing, missing
    return fx


def save(path, fx):
    """A .npz whose bytes depend on the arrays alone (np.savez stamps the members with the time of day)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(fx):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(fx[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------ the census
def _views(fx):
    rec, out, draws = fx["rec"], fx["out"], fx["draws"]
    A, B = out[:, 0], out[:, 1]
    front = rec[:, FRONT] != 0
    outward = rec[:, NRM].view(F32)
    n = np.where(front[:, None], outward, -outward)
    return dict(rec=rec, A=A, B=B, endA=A[:, S_ENDED] != 0, endB=B[:, S_ENDED] != 0, dA=draws[:, 0],
                dH=draws[:, 1] - draws[:, 0], n=n, dirA=A[:, S_D].view(F32),
                active=rec[:, STATUS] == ACTIVE)


def _same_rows(a, b):
    return (canon(a) == canon(b)).all(1)


# label -> (least count, what the stored outputs of a record of the class must show)
CLASSES = {
    "general": (400, lambda v: v["active"]),
    "band_tir": (8, lambda v: (v["dA"] == 0) & ~v["endA"]),                   # total reflection: no Schlick draw
    "band_open": (8, lambda v: v["dA"] == 1),
    "band_near": (16, lambda v: ~v["endA"]),
    "glass_cos1": (2, lambda v: ~v["endA"]),
    "glass_cos0": (2, lambda v: ~v["endA"]),
    "glass_cos_gt1": (4, lambda v: ~v["endA"]),
    "glass_ior1": (4, lambda v: ~v["endA"]),
    "glass_nan_normal": (2, lambda v: np.isnan(v["dirA"]).any(1)),
    "schlick_reflect": (6, lambda v: (v["dirA"] * v["n"]).sum(1) > 0),
    "schlick_refract": (6, lambda v: (v["dirA"] * v["n"]).sum(1) < 0),
    "lambert_degenerate": (12, lambda v: _same_rows(v["dirA"], v["n"]) & (v["dA"] == 3)),
    "lambert_neighbour": (4, lambda v: ~_same_rows(v["dirA"], v["n"]) & (v["dA"] == 3)),
    "lambert_rejected": (3, lambda v: v["dA"] >= 6),
    "metal_tangent": (6, lambda v: v["endA"]),
    "metal_cancel": (2, lambda v: v["endA"]),
    "metal_below": (2, lambda v: v["endA"]),
    "metal_kept": (2, lambda v: ~v["endA"]),
    "metal_clamp": (8, lambda v: v["dA"] >= 3),
    "roulette_at_p": (4, lambda v: ~v["endB"] & (v["dH"] == 1)),
    "roulette_above_p": (4, lambda v: v["endB"] & ~v["endA"] & (v["dH"] == 1)),
    "roulette_tiny_p": (2, lambda v: ~v["endB"] & (v["dH"] == 1)),
    "roulette_tiny_p_ends": (2, lambda v: v["endB"] & (v["dH"] == 1)),
    "roulette_zero_p": (2, lambda v: v["endB"] & (v["dH"] == 1)),
    "roulette_nan": (4, lambda v: v["dH"] == 1),
    "roulette_first": (2, lambda v: (v["dH"] == 1) & (v["B"][:, S_BOUNCE] == 3)),
    "roulette_none": (2, lambda v: (v["dH"] == 0) & ~v["endB"]),
    "limit_20": (2, lambda v: v["endB"] & ~v["endA"] & (v["dH"] == 0) & (v["B"][:, S_BOUNCE] == 20)),
    "limit_1": (2, lambda v: v["endB"] & ~v["endA"] & (v["dH"] == 0) & (v["B"][:, S_BOUNCE] == 1)),
    "dir_tiny": (3, lambda v: v["active"]),
    "dir_huge": (3, lambda v: v["active"]),
    "dir_big": (3, lambda v: v["active"]),
    "dir_zero": (3, lambda v: v["active"]),
    "misc_miss": (2, lambda v: v["endA"] & (v["dA"] == 0)),
    "misc_light": (2, lambda v: v["endA"] & (v["A"][:, S_ADD].view(F32) > 1).all(1)),
    "misc_unknown": (2, lambda v: v["endA"] & ~v["A"][:, S_ADD].any(1)),
    "misc_index_n": (2, lambda v: ~v["endA"] & (v["dA"] == 0) & _same_rows(v["A"][:, S_D], v["rec"][:, D])),
    "misc_index_neg": (2, lambda v: ~v["endA"] & (v["dA"] == 0) & _same_rows(v["A"][:, S_D], v["rec"][:, D])),
    "misc_front_flip": (8, lambda v: v["active"]),
    "misc_ended_in": (5, lambda v: ~v["active"]),
}
# the classes whose records run a slow sequence behind a wave ballot (the f64 glass test, the IEEE reciprocal and
# square root): the ones the wave-composition test puts among general-position lanes
SLOW = ("band_tir", "band_open", "roulette_tiny_p", "roulette_zero_p", "dir_tiny", "dir_huge", "dir_zero")


def census(fx):
    """label -> number of records of the class whose stored outputs show the class's outcome."""
    v = _views(fx)
    label = fx["label"]
    assert set(np.unique(label).tolist()) <= {k.encode() for k in CLASSES}
    return {k: int((pred(v) & (label == k.encode())).sum()) for k, (_, pred) in CLASSES.items()}


def census_missing(fx):
    """The classes below their count, with what was found (empty: the fixture is complete)."""
    got = census(fx)
    labelled = {k: int((fx["label"] == k.encode()).sum()) for k in CLASSES}
    out = {k: (got[k], least) for k, (least, _) in CLASSES.items() if got[k] < least}
    out.update({k + " (records of the class without its outcome)": (got[k], labelled[k])
                for k in CLASSES if got[k] != labelled[k]})
    return out


def records_of(fx, *labels):
    return np.nonzero(np.isin(fx["label"], [k.encode() for k in labels]))[0]


# ------------------------------------------------------------------------------------------ the device's view
def scene_material(fx, base):
    """Each record's material index in a scene that holds the fixture's table after `base` materials of its own."""
    idx = fx["rec"][:, MAT].view(np.int32)
    return np.where(idx < 0, idx, idx + base).astype(np.int32)


def batch(fx, idx, base, max_bounces):
    """The arrays of one device call over the records idx (repeats allowed): entry j is record idx[j] on pixel j.
    Records with another bounce limit than the call's come in ENDED and must be left alone.
    Returns rays (n, 8) f32, hits (n, 8) f32, paths (n, 8) i32, rng (n, 6) u32, lin (n, 3) f32."""
    rec = fx["rec"][idx]
    n = len(idx)
    rays = np.zeros((n, 8), F32)
    rays[:, 0:3] = rec[:, O].view(F32)
    rays[:, 3] = np.inf
    rays[:, 4:7] = rec[:, D].view(F32)
    hits = np.zeros((n, 8), U32)
    hits[:, 0] = rec[:, T]
    hits[:, 3] = scene_material(fx, base)[idx].view(U32)
    hits[:, 4:7] = rec[:, NRM]
    hits[:, 7] = rec[:, FRONT]
    paths = np.zeros((n, 8), np.int32)
    paths[:, 0:3] = rec[:, THR].view(np.int32)
    paths[:, 3] = rec[:, BOUNCE].view(np.int32)
    paths[:, 4] = np.arange(n)
    skip = (rec[:, STATUS] != ACTIVE) | (rec[:, MAXB] != max_bounces)
    paths[:, 5] = np.where(skip, ENDED, ACTIVE)
    return rays, hits.view(F32), paths, rec[:, RNG].copy(), fx["lin"][idx].view(F32).copy()


def expected(fx, idx, base, max_bounces):
    """What Scene.path_step must leave of batch(fx, idx, base, max_bounces): the same five arrays."""
    rays, hits, paths, rng, lin = batch(fx, idx, base, max_bounces)
    B = fx["out"][idx, 1]
    ran = paths[:, 5] == ACTIVE
    ended = B[:, S_ENDED] != 0
    go = ran & ~ended
    rays[go, 0:3] = B[go, S_O].view(F32)
    rays[go, 4:7] = B[go, S_D].view(F32)
    paths[ran, 0:3] = B[ran, S_THR].view(np.int32)
    paths[ran, 3] = B[ran, S_BOUNCE].view(np.int32)
    paths[ran & ended, 5] = ENDED
    rng[ran] = B[ran, S_RNG]
    end = ran & ended
    with np.errstate(all="ignore"):
        lin[end] = (lin[end] + B[end, S_ADD].view(F32)).astype(F32)
    return rays, paths, rng, lin


def geometric_front(fx, idx):
    """dot(d, outward) < 0 in the device's float32 operation order: the face the render kernels take."""
    d, n = fx["rec"][idx][:, D].view(F32), fx["rec"][idx][:, NRM].view(F32)
    with np.errstate(all="ignore"):
        dot = ((d[:, 0] * n[:, 0]).astype(F32) + (d[:, 1] * n[:, 1]).astype(F32)).astype(F32) + (d[:, 2] * n[:, 2]).astype(F32)
        return dot.astype(F32) < 0


def shade_records(fx, idx):
    """The (n, 32) records of crt_selftest_shade for the records idx: the hit's shading record is the outward normal
    with the material's code, and its payload row; an index outside the table is code 5 (SHADE_INVALID)."""
    rec = fx["rec"][idx]
    M = len(fx["mats"])
    mat = rec[:, MAT].view(np.int32)
    valid = (mat >= 0) & (mat < M)
    rows = fx["rows"][np.clip(mat, 0, M - 1)]
    out = np.zeros((len(idx), 32), U32)
    out[:, 0:7] = rec[:, 0:7]
    out[:, 7] = ~(rec[:, T].view(F32) < 0)
    out[:, 8:11] = rec[:, NRM]
    out[:, 11] = np.where(valid, rows[:, 0, 0], 5)
    out[:, 12:16] = np.where(valid[:, None], rows[:, 1], 0)
    out[:, 16:19] = rec[:, THR]
    out[:, 19], out[:, 20] = rec[:, BOUNCE], rec[:, MAXB]
    out[:, 21:27] = rec[:, RNG]
    return out
