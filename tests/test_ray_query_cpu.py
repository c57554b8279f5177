"""Ray queries, the host-only half (no GPU needed): header / exports / bindings, crt_trace_validate_rays, the per-rank
identity table (crt_scene_export_identity) and the normal a triangle's hit record carries."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import custom_scene  # noqa: E402
from bvh_emulation import _is_sphere, _prim_ranks  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
NEW = ("crt_trace_validate_rays", "crt_scene_export_identity", "crt_scene_trace", "crt_scene_occluded",
       "crt_scene_trace_device", "crt_scene_trace_last_stats")
REBUILT = {"w4": dict(width=4), "w4_leaf16": dict(width=4, leaf_size=16), "w4_sbvh": dict(width=4, spatial_splits=True),
           "w2_leaf16": dict(width=2, leaf_size=16)}


# ------------------------------------------------------------------------------------------ header, exports, bindings
def test_new_names_declared_exported_bound():
    import subprocess
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "crt_hip.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.HIP_LIB)], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    L = _lib.hip()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported and name in _lib.HIP_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.crt_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", header)


def _c_sizeof(tmp_path, names):
    """sizeof of the header's structs as a C compiler lays them out."""
    import subprocess
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "crt_hip.h"\nint main(void) { printf("' + " ".join(["%zu"] * len(names)) +
                   '\\n", ' + ", ".join(f"sizeof({n})" for n in names) + "); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-I", str(REPO / "include"), "-o", str(exe), str(src)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_struct_sizes_on_both_sides(tmp_path):
    ray, hit, opt, stats = _c_sizeof(tmp_path, ["crt_ray", "crt_hit", "crt_trace_options", "crt_trace_stats"])
    assert ray == 32 and hit == 32
    assert C.sizeof(_lib.Ray) == 32 and C.sizeof(_lib.Hit) == 32
    assert C.sizeof(_lib.TraceOptions) == opt and C.sizeof(_lib.TraceStats) == stats
    assert crt_amd.HIT_DTYPE.itemsize == 32
    assert [crt_amd.HIT_DTYPE.fields[k][1] for k in ("t", "object", "primitive", "material", "normal", "front_face")] == \
        [getattr(_lib.Hit, k).offset for k in ("t", "object", "primitive", "material", "normal", "front_face")]


# ------------------------------------------------------------------------------------------ crt_trace_validate_rays
def _clean(n=16):
    rng = np.random.default_rng(5)
    return crt_amd.pack_rays(rng.uniform(-1, 1, (n, 3)), rng.normal(size=(n, 3)), None)


def _validate(r):
    bad = C.c_int64(-7)
    rc = _lib.hip().crt_trace_validate_rays(r.ctypes.data_as(C.c_void_p), len(r), C.byref(bad))
    return rc, bad.value, _lib.hip().crt_last_error().decode()


def test_validate_accepts_clean_rays():
    r = _clean()
    assert r.shape == (16, 8) and np.isinf(r[:, 3]).all() and (r[:, 7] == 0).all()
    assert _validate(r)[:2] == (0, -7)
    assert crt_amd.validate_rays(r) == -1
    assert _lib.hip().crt_trace_validate_rays(None, 0, None) == 0
    assert _lib.hip().crt_trace_validate_rays(None, 3, None) == -1
    assert _lib.hip().crt_trace_validate_rays(r.ctypes.data_as(C.c_void_p), -1, None) == -1


BAD = {"nan_o": (0, np.nan), "inf_o": (1, np.inf), "ninf_o": (2, -np.inf), "nan_d": (4, np.nan), "inf_d": (5, np.inf),
       "ninf_d": (6, -np.inf), "nan_tmax": (3, np.nan), "far_o": (2, 2.0 ** 59), "far_o_neg": (0, -2.0 ** 59)}


@pytest.mark.parametrize("case", list(BAD))
@pytest.mark.parametrize("at", [0, 7, 15])
def test_validate_rejects(case, at):
    r = _clean()
    col, value = BAD[case]
    r[at, col] = value
    if at < 15:
        r[15, 4] = np.nan              # a later bad ray: the FIRST one is named
    rc, bad, msg = _validate(r)
    assert rc == -1 and bad == at and f"ray {at}:" in msg
    assert crt_amd.validate_rays(r) == at


def test_validate_rejects_zero_direction():
    for zero in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)):
        r = _clean()
        r[9, 4:7] = zero
        assert _validate(r)[:2] == (-1, 9)


def test_validate_accepts_edge_values():
    r = _clean(12)
    r[0, 4:7] = (0.0, -0.0, 1.0)       # zero components of either sign
    r[1, 4:7] = (-0.0, 2.0, 0.0)
    r[2, 4:7] = (1e-30, 0.0, 0.0)
    r[3, 3] = np.inf
    r[4, 3] = 0.0
    r[5, 3] = -1.0
    r[6, 3] = -np.inf
    r[7, :3] = np.nextafter(np.float32(2.0 ** 59), np.float32(0))       # the largest origin inside the bound
    r[8, 7] = np.nan                   # the reserved word is not read
    assert _validate(r)[:2] == (0, -7)


def test_host_entries_reject_bad_arguments_without_a_device():
    """Argument errors come before any device call; n == 0 is CRT_OK and launches nothing."""
    L = _lib.hip()
    r = _clean(4)
    hits = np.zeros((4, 8), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.crt_scene_trace(None, p(r), 4, None, p(hits)) == -1
    assert L.crt_scene_occluded(None, p(r), 4, None, p(hits)) == -1
    assert L.crt_scene_trace_device(None, p(r), 4, None, p(hits), None, 0, None) == -1
    assert L.crt_scene_trace_last_stats(None, None) == -1


# ------------------------------------------------------------------------------------------ identity table
@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    return custom_scene.synth_worlds(custom_scene.family_files(tmp_path_factory.mktemp("rq_synth")))


def _all_oracle_prims(cs):
    """Every primitive id OracleScene.trace can return: (mesh, permuted triangle) and (-1 - sphere, 0)."""
    tris = [np.stack([np.full(n, m), np.arange(n)], 1) for m, n in enumerate(cs.loaded.mesh_info[:, 3].astype(np.int64) // 3)]
    sph = np.stack([-1 - np.arange(cs.n_spheres), np.zeros(cs.n_spheres, np.int64)], 1)
    return np.concatenate(tris + [sph]).astype(np.int64)


def _check_identity(desc, cs, ranks_of):
    ident = crt_amd.identity_desc(desc, "reference")
    e = crt_amd.export_desc(desc, "reference")
    assert ident.shape == (e["ranks"], 3) and ident.dtype == np.int32
    for name, o in REBUILT.items():
        assert np.array_equal(crt_amd.identity_desc(desc, "rebuilt", **o), ident), name
    # the material column is the record's material word: triangle f2.y, sphere f1.y
    prims = e["prims"].reshape(-1, 3, 4)
    sph = _is_sphere(e["prims"])
    mat = np.where(sph, prims[:, 1, 1].view(np.int32), prims[:, 2, 1].view(np.int32))
    assert np.array_equal(ident[_prim_ranks(e["prims"]), 2], mat)
    assert np.array_equal(sph, ident[_prim_ranks(e["prims"]), 0] < 0)
    if cs is not None:   # it inverts oracle_ranks
        ids = _all_oracle_prims(cs)
        assert np.array_equal(ident[ranks_of(ids), :2], ids)
        assert len(np.unique(ranks_of(ids))) == len(ids) == len(ident)
    return ident


@pytest.mark.parametrize("name", custom_scene.FAMILIES + custom_scene.WORLDS + custom_scene.ONLY)
def test_identity_table_synth(worlds, name):
    cs = worlds[name]
    _check_identity(cs.desc, cs, cs.oracle_ranks)


def test_identity_table_cornell_bunny(scenes):
    hs = crt_amd.HostScene(scenes["cornell_bunny"])
    cs = custom_scene.CustomScene(scenes["cornell_bunny"])       # the same world (SceneManager's sphere pair), for the ids
    ident = _check_identity(hs.desc(), None, None)
    assert np.array_equal(hs.identity(), ident) and np.array_equal(hs.identity("rebuilt", width=4), ident)
    ids = _all_oracle_prims(cs)
    assert np.array_equal(ident[cs.oracle_ranks(ids), :2], ids)
    assert np.array_equal(_check_identity(cs.desc, cs, cs.oracle_ranks)[:, :2], ident[:, :2])


def test_identity_null_arguments():
    assert _lib.hip().crt_scene_export_identity(None, None, None, None) == -1


# ------------------------------------------------------------------------------------------ the record's normal
def tri_normals_f32(prims):
    """unit(cross(e1, e2)) of triangle records [n, 3, 4] in float32, the operation order of Mesh.cuh:303-304 and
    Vec3::unit: cross components as a*b - c*d, length as sqrt((x*x + y*y) + z*z), then (1 / length) * v."""
    f = np.float32
    ux, uy, uz = prims[:, 0, 3], prims[:, 1, 0], prims[:, 1, 1]
    vx, vy, vz = prims[:, 1, 2], prims[:, 1, 3], prims[:, 2, 0]
    with np.errstate(all="ignore"):
        cx = (uy * vz).astype(f) - (uz * vy).astype(f)
        cy = (uz * vx).astype(f) - (ux * vz).astype(f)
        cz = (ux * vy).astype(f) - (uy * vx).astype(f)
        s = f(1) / np.sqrt(((cx * cx).astype(f) + (cy * cy).astype(f)).astype(f) + (cz * cz).astype(f)).astype(f)
        return np.stack([(s * cx).astype(f), (s * cy).astype(f), (s * cz).astype(f)], 1)


@pytest.mark.parametrize("name", ["soup", "degenerate"])
def test_triangle_normal_operation_order(worlds, name):
    """Validates tri_normals_f32, the numpy helper tests/test_gpu_ray_query.py pins the hit record's normal with, bit
    for bit, on the GPU.  It runs no code of the library: the shading records that hold the normal are not exported on
    the host, so the bit-exact comparison can only be made against a device query (GPU test 1).  Here the helper's
    float32 result is checked against float64 geometry: unit length and parallel to cross(e1, e2) within float32
    rounding, for every triangle that can be hit (zero-area ones have no finite normal and no ray hits them: |det| <
    1e-8 rejects)."""
    e = worlds[name].ref_export()
    prims = e["prims"].reshape(-1, 3, 4)[~_is_sphere(e["prims"])]
    n = tri_normals_f32(prims)
    ok = np.isfinite(n).all(1)
    assert ok.sum() >= 0.9 * len(prims) and (name != "degenerate" or (~ok).sum() > 0)
    p = prims.astype(np.float64)
    e1 = np.stack([p[:, 0, 3], p[:, 1, 0], p[:, 1, 1]], 1)
    e2 = np.stack([p[:, 1, 2], p[:, 1, 3], p[:, 2, 0]], 1)
    c = np.cross(e1, e2)
    big = ok & (np.linalg.norm(c, axis=1) > 1e-3 * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    assert big.sum() >= 0.8 * len(prims)
    ref = c[big] / np.linalg.norm(c[big], axis=1, keepdims=True)
    # cancellation in the f32 cross product of a well-shaped triangle stays below 1e-3 / sin(angle) relative
    assert np.abs(n[big].astype(np.float64) - ref).max() < 1e-3
    assert np.abs(np.linalg.norm(n[big].astype(np.float64), axis=1) - 1).max() < 1e-6
