// crt_scene.h — the scene handle's entries and the host half of scene creation: the Flattener (the reference's scene and
// mesh BVHs into the threaded layout, the DFS ranks), Rebuilt (the host SAH / SBVH build and the 4-wide collapse), the
// per-rank shading records, the per-material rows, the identity table and the crt_scene_* entries.  Host code only.
// Included by crt_hip.hip after crt_handles.h; needs crt_sah.h, crt_device.h's record layouts and crtx_build_sah_gpu.
#pragma once

namespace {

inline float i2f(int v) { float f; std::memcpy(&f, &v, 4); return f; }
inline int i2i_host(float f) { int v; std::memcpy(&v, &f, 4); return v; }

inline bool zero_thickness(const float bmin[3], const float bmax[3]) {
    // AABB::hit can never report such a box (the slab of that axis is empty: tmax <= tmin)
    return bmin[0] == bmax[0] || bmin[1] == bmax[1] || bmin[2] == bmax[2];
}

// CRT_SETUP_TRACE=1: the host stages of scene creation timed on stderr (tools/setup_breakdown.py).
struct SetupTrace {
    bool on = std::getenv("CRT_SETUP_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char* stage) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[crt setup] %-28s %8.2f ms\n", stage, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// The host loops of scene creation that gather or fill one record per primitive run on up to 16 threads
// (CRT::parallel_ranges; on config E's million triangles they took ~120 ms of its 0.34-s scene creation on one,
// profiles/r05k).
using CRT::parallel_ranges;

// Flattens the reference's scene + mesh BVHs into the threaded layout and records, per primitive,
// its reference DFS rank (the order BVHNode::hit / Mesh::hit visit primitives) and whether any box
// on its path is zero-thickness (then the reference never reports it).
struct Flattener {
    const crt_scene_desc* D;
    std::vector<float4> nodes, prims;
    std::vector<int> mesh_prim_base;
    std::vector<int> rank_of;        // per prim
    std::vector<char> reachable;     // per prim
    std::vector<int> rank_code;      // per rank: prim code
    std::vector<int> sphere_of;      // per sphere prim, in prim order after the triangles: its index in D->spheres
    int max_depth = 0;
    std::string err;

    void visit_prim(int p, int code, bool thin) {
        if (rank_of[p] >= 0) return;
        rank_of[p] = (int)rank_code.size();
        rank_code.push_back(code);
        reachable[p] = !thin;
    }
    // Primitives no leaf references get the remaining ranks (never hit); ranks go into the records.
    void finalize_ranks() {
        const int n = (int)(prims.size() / 3);
        for (int p = 0; p < n; ++p) {
            if (rank_of[p] < 0) {
                rank_of[p] = (int)rank_code.size();
                rank_code.push_back(p);
                reachable[p] = 0;
            }
            const bool sphere = (rank_code[rank_of[p]] & SPHERE_BIT) != 0;
            if (sphere) prims[3 * p + 1].z = i2f(rank_of[p]);
            prims[3 * p + 2].z = i2f(rank_of[p]);
        }
    }

    int push_node(const float bmin[3], const float bmax[3], int a, int b) {
        nodes.push_back(make_float4(bmin[0], bmin[1], bmin[2], bmax[0]));
        nodes.push_back(make_float4(bmax[1], bmax[2], i2f(a), i2f(b)));
        return (int)(nodes.size() / 2) - 1;
    }
    void set_a(int idx, int a) { nodes[2 * idx + 1].z = i2f(a); }
    int count() const { return (int)(nodes.size() / 2); }

    bool emit_mesh(int m, int ni, int depth, bool thin) {
        const crt_mesh_desc& M = D->meshes[m];
        if (ni < 0 || ni >= M.node_count) { err = "mesh node index out of range"; return false; }
        if (depth > 4096) { err = "mesh BVH too deep"; return false; }
        max_depth = std::max(max_depth, depth);
        const crt_bvh_node_desc& N = M.nodes[ni];
        thin = thin || zero_thickness(N.bmin, N.bmax);
        if (!N.is_leaf) {
            int idx = push_node(N.bmin, N.bmax, 0, NODE_MESH_INNER);
            if (!emit_mesh(m, N.left, depth + 1, thin) || !emit_mesh(m, N.right, depth + 1, thin)) return false;
            set_a(idx, count());
        } else {
            if (N.obj_index < 0 || N.obj_count < 0 || N.obj_index % 3 || N.obj_count % 3 ||
                (uint64_t)N.obj_index + N.obj_count > M.index_count) { err = "bad mesh leaf range"; return false; }
            long first = mesh_prim_base[m] + N.obj_index / 3;
            if (first >= SPHERE_BIT) { err = "too many primitives"; return false; }
            push_node(N.bmin, N.bmax, N.obj_count / 3, (int)first);
            for (int k = 0; k < (int)N.obj_count / 3; ++k) visit_prim((int)first + k, (int)first + k, thin);
        }
        return true;
    }
    bool emit_scene(int ni, int depth, bool thin) {
        if (ni < 0 || ni >= D->n_scene_nodes) { err = "scene node index out of range"; return false; }
        if (depth > 4096) { err = "scene BVH too deep"; return false; }
        max_depth = std::max(max_depth, depth);
        const crt_bvh_node_desc& N = D->scene_nodes[ni];
        thin = thin || zero_thickness(N.bmin, N.bmax);
        if (!N.is_leaf) {
            int idx = push_node(N.bmin, N.bmax, 0, NODE_SCENE_INNER);
            if (!emit_scene(N.left, depth + 1, thin) || !emit_scene(N.right, depth + 1, thin)) return false;
            set_a(idx, count());
            return true;
        }
        if (N.obj_index < 0 || N.obj_index >= D->n_objects) { err = "scene leaf object out of range"; return false; }
        const crt_object_desc& O = D->objects[N.obj_index];
        if (O.kind == CRT_OBJECT_MESH) {
            if (O.index < 0 || O.index >= D->n_meshes) { err = "mesh object index out of range"; return false; }
            int idx = push_node(N.bmin, N.bmax, 0, NODE_SCENE_INNER);
            if (D->meshes[O.index].node_count > 0 && !emit_mesh(O.index, 0, depth + 1, thin)) return false;
            set_a(idx, count());
        } else if (O.kind == CRT_OBJECT_SPHERE) {
            if (O.index < 0 || O.index >= D->n_spheres) { err = "sphere object index out of range"; return false; }
            const crt_sphere_desc& S = D->spheres[O.index];
            int p = (int)(prims.size() / 3);
            if (p >= SPHERE_BIT) { err = "too many primitives"; return false; }
            prims.push_back(make_float4(S.center[0], S.center[1], S.center[2], S.radius));
            prims.push_back(make_float4(S.radius * S.radius, i2f(S.material), 0.f, 0.f));   // Sphere.cuh:21
            prims.push_back(make_float4(0.f, i2f(S.material), 0.f, i2f(1)));                  // word 11 = 1: sphere
            rank_of.push_back(-1);
            reachable.push_back(0);
            sphere_of.push_back(O.index);
            visit_prim(p, SPHERE_BIT | p, thin);
            push_node(N.bmin, N.bmax, 0, SPHERE_BIT | p);
        } else {
            err = "unknown object kind";
            return false;
        }
        return true;
    }
    bool build_triangles() {
        mesh_prim_base.assign(D->n_meshes, 0);
        size_t total = 0;
        for (int m = 0; m < D->n_meshes; ++m) {
            const crt_mesh_desc& M = D->meshes[m];
            if ((uint64_t)M.index_offset + M.index_count > D->n_indices ||
                (uint64_t)M.vertex_offset + M.vertex_count > D->n_positions ||
                (uint64_t)M.face_offset + M.index_count / 3 > D->n_faces || M.index_count % 3) {
                err = "mesh ranges exceed the scene arrays";
                return false;
            }
            mesh_prim_base[m] = (int)total;
            total += M.index_count / 3;
        }
        prims.reserve(3 * (total + (size_t)std::max(D->n_spheres, 0)));   // emit_scene appends the spheres
        prims.assign(3 * total, make_float4(0.f, 0.f, 0.f, 0.f));
        bool bad_index = false;
        for (int m = 0; m < D->n_meshes; ++m) {
            const crt_mesh_desc& M = D->meshes[m];
            float4* out = prims.data() + 3 * (size_t)mesh_prim_base[m];
            std::atomic<bool> bad{false};
            parallel_ranges(M.index_count / 3, [&](size_t b, size_t e) {
                for (size_t t = b; t < e; ++t) {
                    uint32_t iv[3];
                    for (int c = 0; c < 3; ++c) {
                        iv[c] = D->indices[M.index_offset + 3 * t + c];
                        if (iv[c] >= M.vertex_count) { bad.store(true, std::memory_order_relaxed); iv[c] = 0; }   // reported below
                    }
                    const float* p0 = D->positions + 3 * ((size_t)M.vertex_offset + iv[0]);
                    const float* p1 = D->positions + 3 * ((size_t)M.vertex_offset + iv[1]);
                    const float* p2 = D->positions + 3 * ((size_t)M.vertex_offset + iv[2]);
                    const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};   // Mesh.cuh:277
                    const float e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};   // Mesh.cuh:278
                    const uint32_t mat = (uint32_t)(D->face_materials[M.face_offset + t] + (int32_t)M.material_id_offset);
                    out[3 * t] = make_float4(p0[0], p0[1], p0[2], e1[0]);
                    out[3 * t + 1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
                    out[3 * t + 2] = make_float4(e2[2], i2f((int)mat), 0.f, 0.f);
                }
            });
            bad_index = bad_index || bad.load();
        }
        if (bad_index) { err = "vertex index out of range"; return false; }
        rank_of.assign(prims.size() / 3, -1);
        reachable.assign(prims.size() / 3, 0);
        return true;
    }
};

// CRT_BVH_REBUILT: binned-SAH tree over the reachable primitives of a flattened reference scene,
// emitted as `layouts` threaded arrays (crt_sah.h).  Primitive records keep their rank.
struct Rebuilt {
    std::vector<float4> nodes, prims;
    std::vector<int> rank_code;
    int n_nodes = 0, max_depth = 0;
    long excluded = 0;
    std::string err;

    int width = 2;
    int stack_bound = 0;   // width 4: most stack entries any traversal can hold
    int sphere_first = 0, n_ray_spheres = 0;   // width 4: spheres kept out of the tree (tested per ray)
    std::vector<float4> chain;                 // their reference scene-level leaf boxes (2 float4 per box)
    static constexpr int kMaxRaySpheres = 8;
    // With more than kMaxRaySpheres spheres the small ones go into the tree's leaves, but a sphere of at least this
    // radius stays per ray: only there is its reference scene-level box replayed (ray_spheres).  The f32 roots of
    // Sphere::hit err by about ulp(r^2) / |oc . d|; for the radius-999 ground sphere that puts a spurious root of a
    // ray leaving the surface above t = 0.001 while the reference's box test has already rejected the ray
    // (tests/golden/ground_sphere_rays.json), and a leaf's padded box is too wide to reject it.  Below radius 1 the
    // same needs a ray within 3e-5 rad of the tangent plane that also starts within 0.001 |d| of the box face.
    static constexpr float kRaySphereRadius = 1.0f;

    // gpu_device >= 0: the binned-SAH tree is built on that GPU (crtx_build_sah_gpu, crt_bvh_build.hip)
    long spatial_splits = 0;   // SBVH: nodes cut by a plane, and primitive references in the leaves
    long references = 0;

    // gpu_device >= 0: the binned-SAH tree is built on that GPU (crtx_build_sah_gpu, crt_bvh_build.hip); spatial:
    // SBVH on the host (crt_sah::SpatialBuilder), width 4 only
    bool build(const Flattener& F, int leaf_size, int layouts, float trav_cost, int wide, int gpu_device = -1,
               bool spatial = false, float alpha = 1e-5f, float max_dup = 1.f) {
        SetupTrace tr;
        width = wide;
        const int n = (int)(F.prims.size() / 3);
        std::vector<crt_sah::Item> items;
        items.reserve(n);
        std::vector<int> ray_sph;
        std::vector<crt_sah::TriVerts> verts;
        if (spatial && width != 4) { err = "spatial splits need width 4"; return false; }
        int n_sph = 0, n_large = 0;
        for (int p = 0; p < n; ++p)
            if (F.rank_code[F.rank_of[p]] & SPHERE_BIT) {
                ++n_sph;
                n_large += F.reachable[p] && !(std::fabs(F.prims[3 * (size_t)p].w) < kRaySphereRadius);
            }
        const bool all_per_ray = width == 4 && n_sph <= kMaxRaySpheres;
        if (width == 4 && !all_per_ray && n_large > kMaxRaySpheres) {
            err = "more than 8 spheres of radius >= 1 among more than 8 spheres: large spheres are tested per ray, "
                  "at most 8 of them (width 2 takes any number)";
            return false;
        }
        for (int p = 0; p < n; ++p) {
            const bool sphere = (F.rank_code[F.rank_of[p]] & SPHERE_BIT) != 0;
            if (!F.reachable[p]) { excluded += !sphere; continue; }
            const float4 f0 = F.prims[3 * p], f1 = F.prims[3 * p + 1], f2 = F.prims[3 * p + 2];
            const bool spheres_per_ray = all_per_ray || (width == 4 && !(std::fabs(f0.w) < kRaySphereRadius));
            if (sphere && spheres_per_ray) {
                // a per-ray sphere's hit point becomes a ray origin too: the same 2^60 bound as the tree's boxes
                // (wide_boxes: |o| * 2^64 must stay finite)
                const float c[3] = {f0.x, f0.y, f0.z}, r = std::fabs(f0.w);
                for (int a = 0; a < 3; ++a)
                    if (!(std::fabs(c[a] - r) < 0x1p60f && std::fabs(c[a] + r) < 0x1p60f)) {
                        err = "sphere bounds non-finite or beyond 2^60";
                        return false;
                    }
                ray_sph.push_back(p);
                continue;
            }
            crt_sah::Item it;
            it.src = p;
            it.sphere = sphere;
            if (sphere) {
                const float c[3] = {f0.x, f0.y, f0.z}, r = std::fabs(f0.w);
                for (int a = 0; a < 3; ++a) { it.lo[a] = c[a] - r; it.hi[a] = c[a] + r; }
            } else {
                const float v0[3] = {f0.x, f0.y, f0.z};
                const float e1[3] = {f0.w, f1.x, f1.y}, e2[3] = {f1.z, f1.w, f2.x};
                for (int a = 0; a < 3; ++a) {
                    const float v1 = v0[a] + e1[a], v2 = v0[a] + e2[a];
                    it.lo[a] = std::min(v0[a], std::min(v1, v2));
                    it.hi[a] = std::max(v0[a], std::max(v1, v2));
                }
            }
            if (spatial && !sphere) {   // the triangle's vertices for clipping, v0 + e1 and v0 + e2 exact in double
                crt_sah::TriVerts T;
                const double v0[3] = {f0.x, f0.y, f0.z};
                const double e1[3] = {f0.w, f1.x, f1.y}, e2[3] = {f1.z, f1.w, f2.x};
                for (int a = 0; a < 3; ++a) {
                    T.v[0][a] = v0[a];
                    T.v[1][a] = v0[a] + e1[a];
                    T.v[2][a] = v0[a] + e2[a];
                }
                it.tri = (int)verts.size();
                verts.push_back(T);
            }
            bool finite = true;
            for (int a = 0; a < 3; ++a) {
                it.c[a] = 0.5f * it.lo[a] + 0.5f * it.hi[a];
                // box_inv's clamp (2^64) keeps |coord| * inv finite only below 2^60 (wide_boxes)
                finite = finite && std::fabs(it.lo[a]) < 0x1p60f && std::fabs(it.hi[a]) < 0x1p60f;
            }
            if (!finite) { err = "primitive bounds non-finite or beyond 2^60"; return false; }
            items.push_back(it);
        }
        rank_code.assign(F.rank_code.size(), 0);
        auto append_ray_spheres = [&]() {
            sphere_first = (int)(prims.size() / 3);
            const int n_ref = F.count();
            for (int p : ray_sph) {
                const int np = (int)(prims.size() / 3);
                for (int q = 0; q < 3; ++q) prims.push_back(F.prims[3 * p + q]);
                rank_code[F.rank_of[p]] = SPHERE_BIT | np;
                // the sphere's leaf in the flattened reference scene and every scene-level node enclosing it
                int leaf = -1;
                for (int i = 0; i < n_ref && leaf < 0; ++i)
                    if (i2i(F.nodes[2 * (size_t)i + 1].w) == (SPHERE_BIT | p)) leaf = i;
                const float4 B = F.nodes[2 * (size_t)leaf + 1];
                prims[3 * (size_t)np + 1].w = i2f((int)(chain.size() / 2));
                chain.push_back(F.nodes[2 * (size_t)leaf]);
                chain.push_back(make_float4(B.x, B.y, 0.f, 0.f));
            }
            n_ray_spheres = (int)ray_sph.size();
        };
        if (items.empty()) {   // nothing hittable: one empty-box node that no ray enters
            const float lo[3] = {0, 0, 0};
            prims.assign(3, make_float4(0, 0, 0, 0));
            for (int l = 0; l < layouts; ++l) {
                nodes.push_back(make_float4(lo[0], lo[1], lo[2], lo[0]));
                nodes.push_back(make_float4(lo[1], lo[2], i2f(1), i2f(NODE_MESH_INNER)));
            }
            n_nodes = 1;
            if (width == 4) {   // a 4-wide root with no slots
                nodes.clear();
                for (int r = 0; r < 6; ++r) nodes.push_back(make_float4(1e30f, 1e30f, 1e30f, 1e30f));
                nodes.push_back(make_float4(i2f(0), i2f(0), i2f(0), i2f(0)));
                nodes.push_back(make_float4(0.f, 0.f, 0.f, 0.f));
                prims.clear();
                append_ray_spheres();
                stack_bound = 1;
            }
            return true;
        }
        tr.lap("  SAH items");
        std::vector<crt_sah::Node> bnv;
        std::vector<crt_sah::Item> its;
        if (spatial) {
            crt_sah::SpatialBuilder B(std::move(items), std::move(verts), leaf_size, trav_cost, alpha, max_dup);
            B.build();
            max_depth = B.max_depth();
            spatial_splits = B.spatial_splits();
            bnv = B.nodes();
            its = B.items();
        } else if (gpu_device >= 0) {
            std::vector<int> order;
            if (crtx_build_sah_gpu(gpu_device, items, leaf_size, trav_cost, &bnv, &order, &max_depth) != CRT_OK) {
                err = std::string("GPU SAH build: ") + crt_last_error();
                return false;
            }
            its.resize(order.size());
            for (size_t i = 0; i < order.size(); ++i) its[i] = items[order[i]];
        } else {
            crt_sah::Builder B(std::move(items), leaf_size, trav_cost);
            B.build();
            max_depth = B.max_depth();
            bnv = B.nodes();
            its = B.items();
        }
        references = (long)its.size();
        tr.lap(gpu_device >= 0 ? "  SAH build (GPU)" : "  SAH build (host)");
        if (width == 4) {
            if (!emit4(F, bnv, its, !spatial)) return false;
            tr.lap("  4-wide collapse + emission");
            append_ray_spheres();
            tr.lap("  per-ray spheres");
            return true;
        }
        prims.resize(3 * its.size());
        for (size_t i = 0; i < its.size(); ++i) {
            const int p = its[i].src;
            for (int q = 0; q < 3; ++q) prims[3 * i + q] = F.prims[3 * p + q];
            rank_code[F.rank_of[p]] = its[i].sphere ? (SPHERE_BIT | (int)i) : (int)i;
        }
        const auto& bn = bnv;
        n_nodes = (int)bn.size();
        nodes.reserve(2 * (size_t)n_nodes * layouts);
        for (int l = 0; l < layouts; ++l) {
            const size_t base = nodes.size() / 2;
            emit(bn, its, 0, l, layouts, base);
        }
        return true;
    }

private:
    // 4-wide nodes in BFS order (internal children of a node consecutive), primitives re-laid out so the
    // leaf children of every node are consecutive in slot order.  See the node format at wide_boxes().
    bool emit4(const Flattener& F, const std::vector<crt_sah::Node>& bn, const std::vector<crt_sah::Item>& its,
               bool unique_items) {
        prims.clear();
        SetupTrace tr;
        // a 4-wide node step costs about one triangle test (the cost probe's weights); node costs 0.5
        // and 2 measured the same (profiles/r02ax)
        const crt_sah::Collapse col(bn, 1.0);
        tr.lap("    collapse DP");
        // BFS one level at a time: the level's cuts (Collapse::open, a few dependent reads of the binary tree each) in
        // parallel, then its child and primitive offsets in order
        std::vector<int> queue{0}, first_child_of, leaf_first_of;
        std::vector<crt_sah::Wide> wide;
        size_t n_items = 0;
        for (size_t lb = 0; lb < queue.size();) {
            const size_t le = queue.size();
            wide.resize(le);
            parallel_ranges(le - lb, [&](size_t b, size_t e) {
                for (size_t qi = lb + b; qi < lb + e; ++qi) wide[qi] = col.open(queue[qi]);
            }, 4096);
            for (size_t qi = lb; qi < le; ++qi) {
                const crt_sah::Wide& w = wide[qi];
                first_child_of.push_back((int)queue.size());
                for (int s = 0; s < w.n_internal; ++s) queue.push_back(w.bin[s]);
                leaf_first_of.push_back((int)n_items);
                int total_leaf = 0;
                for (int s = w.n_internal; s < w.n_slots; ++s) {
                    if (bn[w.bin[s]].count > 255) { err = "leaf too large"; return false; }
                    total_leaf += bn[w.bin[s]].count;
                }
                // node_step4 takes the leaf span from counts * 0x01010101 (byte-wise running sums)
                if (total_leaf > 255) { err = "leaf children of one node hold more than 255 primitives"; return false; }
                n_items += (size_t)total_leaf;
                // prim_test addresses a record as __umul24(index, 48): the 4-wide tree holds fewer than 2^24 primitives
                if (n_items >= ((size_t)1 << 24)) { err = "the 4-wide tree holds at most 2^24 - 1 primitives"; return false; }
            }
            lb = le;
        }
        const size_t n_wide = queue.size();
        tr.lap("    node cuts (BFS)");
        // node records and each primitive position's item (item_at), then the primitive records: every node and every
        // position is written once.  Every span node_step4 can form (leaf_first + the node's leaf counts) lies inside
        // the primitive array by construction; the fast kernel relies on it (the checked build re-checks it on the
        // device).
        nodes.assign(8 * n_wide, make_float4(0.f, 0.f, 0.f, 0.f));
        std::vector<int> item_at(n_items);
        parallel_ranges(n_wide, [&](size_t b, size_t e) {
            for (size_t qi = b; qi < e; ++qi) {
                const crt_sah::Wide& w = wide[qi];
                uint32_t counts = 0;
                int at = leaf_first_of[qi];
                for (int s = w.n_internal; s < w.n_slots; ++s) {
                    const crt_sah::Node& L = bn[w.bin[s]];
                    counts |= (uint32_t)L.count << (8 * s);
                    for (int i = L.first; i < L.first + L.count; ++i) item_at[at++] = i;
                }
                float4* row = nodes.data() + 8 * qi;
                for (int a = 0; a < 3; ++a) {
                    float lo[4], hi[4];
                    for (int s = 0; s < 4; ++s) {
                        lo[s] = hi[s] = 1e30f;   // empty slot: zero-thickness, never hit
                        if (s < w.n_slots) { lo[s] = bn[w.bin[s]].lo[a]; hi[s] = bn[w.bin[s]].hi[a]; }
                    }
                    row[2 * a] = make_float4(lo[0], lo[1], lo[2], lo[3]);
                    row[2 * a + 1] = make_float4(hi[0], hi[1], hi[2], hi[3]);
                }
                row[6] = make_float4(i2f(first_child_of[qi]), i2f(w.n_internal | (w.n_slots << 8)), i2f(leaf_first_of[qi]),
                                     i2f((int)counts));
            }
        }, 4096);
        tr.lap("    node records");
        prims.reserve(3 * (n_items + kMaxRaySpheres));   // append_ray_spheres adds at most kMaxRaySpheres records
        prims.resize(3 * n_items);
        // a primitive referenced by several leaves (spatial splits) keeps the rank code of its last position, as the
        // sequential emission did; unique items (the binned builders) have one position each, so any order will do
        auto gather = [&](size_t b, size_t e) {
            for (size_t np = b; np < e; ++np) {
                const crt_sah::Item& it = its[item_at[np]];
                for (int q = 0; q < 3; ++q) prims[3 * np + q] = F.prims[3 * (size_t)it.src + q];
                rank_code[F.rank_of[it.src]] = it.sphere ? (SPHERE_BIT | (int)np) : (int)np;
            }
        };
        if (unique_items) parallel_ranges(n_items, gather);
        else gather(0, n_items);
        n_nodes = (int)queue.size();
        tr.lap("    primitive gather");
        // stack bound: visiting a node with 2+ hit internal children pushes ONE entry (its remaining children)
        if (n_nodes >= (1 << 24)) { err = "too many nodes for 24-bit stack entries"; return false; }
        std::vector<int> bound(n_nodes, 0);
        for (int n = n_nodes - 1; n >= 0; --n) {
            const int fc = i2i(nodes[8 * (size_t)n + 6].x), m = wide[n].n_internal;
            int b = 0;
            for (int s = 0; s < m; ++s) b = std::max(b, bound[fc + s]);
            bound[n] = b + (m >= 2 ? 1 : 0);
        }
        stack_bound = bound[0] + 1;
        return true;
    }
    static int i2i(float f) { int v; std::memcpy(&v, &f, 4); return v; }

    void emit(const std::vector<crt_sah::Node>& bn, const std::vector<crt_sah::Item>& its, int ni, int layout,
              int layouts, size_t base) {
        const crt_sah::Node& N = bn[ni];
        const size_t idx = nodes.size() / 2;
        int a = 0, b;
        if (N.child[0] < 0) {
            if (its[N.first].sphere) b = SPHERE_BIT | N.first;
            else { a = N.count; b = N.first; }
        } else {
            b = NODE_MESH_INNER;
        }
        nodes.push_back(make_float4(N.lo[0], N.lo[1], N.lo[2], N.hi[0]));
        nodes.push_back(make_float4(N.hi[1], N.hi[2], i2f(a), i2f(b)));
        if (N.child[0] < 0) return;
        int first = N.child[0], second = N.child[1];
        if (layouts == 6) {   // near child first along the layout's direction
            const int ax = layout / 2;
            const bool neg = layout & 1;
            const float c0 = bn[first].lo[ax] + bn[first].hi[ax], c1 = bn[second].lo[ax] + bn[second].hi[ax];
            if (neg ? (c1 > c0) : (c1 < c0)) std::swap(first, second);
        }
        emit(bn, its, first, layout, layouts, base);
        emit(bn, its, second, layout, layouts, base);
        nodes[2 * idx + 1].z = i2f((int)(nodes.size() / 2 - base));   // skip, relative to the layout
    }
};

}  // namespace

// Host half of scene creation: flatten the reference BVHs (ranks, reachability) and, for CRT_BVH_REBUILT,
// build the SAH tree.  Shared by crt_scene_create_ex and crt_scene_export.
static int build_scene_arrays(const crt_scene_desc* D, const crt_scene_options* opts, crt_scene_options& o,
                              Flattener& F, Rebuilt& RB, int gpu_device) {
    o = crt_scene_options{};
    if (opts) o = *opts;
    if (o.bvh != CRT_BVH_REFERENCE && o.bvh != CRT_BVH_REBUILT) return set_error(CRT_ERR_INVALID_ARGUMENT, "unknown bvh mode");
    if (o.leaf_size == 0) o.leaf_size = 4;
    if (o.layouts == 0) o.layouts = 6;
    if (o.traversal_cost == 0.f) o.traversal_cost = 2.f;   // measured optimum for 4-wide leaves <= 4 (profiles/r01i)
    if (o.width == 0) o.width = 4;
    if (o.width != 2 && o.width != 4) return set_error(CRT_ERR_INVALID_ARGUMENT, "width must be 2 or 4");
    if (!(o.traversal_cost > 0.f && o.traversal_cost <= 64.f)) return set_error(CRT_ERR_INVALID_ARGUMENT, "traversal_cost must be in (0, 64]");
    if (o.leaf_size < 1 || o.leaf_size > 16) return set_error(CRT_ERR_INVALID_ARGUMENT, "leaf_size must be 1..16");
    if (o.layouts != 1 && o.layouts != 6) return set_error(CRT_ERR_INVALID_ARGUMENT, "layouts must be 1 or 6");
    if (D->n_scene_nodes <= 0 || !D->scene_nodes) return set_error(CRT_ERR_INVALID_ARGUMENT, "scene has no BVH nodes");
    if (D->n_materials < 0 || (D->n_materials > 0 && !D->materials)) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad materials");
    SetupTrace tr;
    if (!F.build_triangles()) return set_error(CRT_ERR_INVALID_ARGUMENT, "scene: " + F.err);
    tr.lap("triangle records");
    if (!F.emit_scene(0, 0, false)) return set_error(CRT_ERR_INVALID_ARGUMENT, "scene: " + F.err);
    tr.lap("flatten reference BVHs");
    F.finalize_ranks();
    tr.lap("ranks");
    if (o.bvh == CRT_BVH_REBUILT) {
        if (o.width == 4) o.layouts = 1;
        if (o.spatial_alpha == 0.f) o.spatial_alpha = 1e-5f;
        if (o.spatial_max_dup == 0.f) o.spatial_max_dup = 1.f;
        if (o.spatial_splits != 0 && o.spatial_splits != 1) return set_error(CRT_ERR_INVALID_ARGUMENT, "spatial_splits must be 0 or 1");
        if (!(o.spatial_alpha > 0.f && o.spatial_alpha <= 1.f) || !(o.spatial_max_dup > 0.f && o.spatial_max_dup <= 8.f))
            return set_error(CRT_ERR_INVALID_ARGUMENT, "spatial_alpha must be in (0, 1], spatial_max_dup in (0, 8]");
        if (!RB.build(F, o.leaf_size, o.layouts, o.traversal_cost, o.width, o.gpu_build && !o.spatial_splits ? gpu_device : -1,
                      o.spatial_splits != 0, o.spatial_alpha, o.spatial_max_dup))
            return set_error(CRT_ERR_INVALID_ARGUMENT, "scene: " + RB.err);
        tr.lap("rebuilt tree (all)");
        if ((size_t)RB.n_nodes * o.layouts * (o.width == 4 ? 8 : 2) >= (size_t)1 << 31)
            return set_error(CRT_ERR_INVALID_ARGUMENT, "scene too large");
    }
    return CRT_OK;
}

extern "C" {

int crt_scene_create(const crt_scene_desc* D, int device, crt_scene** out) {
    return crt_scene_create_ex(D, device, nullptr, out);
}

int crt_scene_export(const crt_scene_desc* D, const crt_scene_options* opts, float* nodes, float* prims,
                     int32_t* rank_code, int64_t info[10]) {
    if (!D || !info) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    crt_scene_options o;
    Flattener F{D};
    Rebuilt RB;
    if (int rc = build_scene_arrays(D, opts, o, F, RB, 0)) return rc;
    const bool rebuilt = o.bvh == CRT_BVH_REBUILT;
    const std::vector<float4>& N = rebuilt ? RB.nodes : F.nodes;
    const std::vector<float4>& Pr = rebuilt ? RB.prims : F.prims;
    const std::vector<int>& rc = rebuilt ? RB.rank_code : F.rank_code;
    info[0] = (int64_t)N.size();
    info[1] = (int64_t)Pr.size();
    info[2] = (int64_t)rc.size();
    info[3] = rebuilt ? RB.n_nodes : F.count();
    info[4] = rebuilt ? o.layouts : 1;
    info[5] = rebuilt ? RB.width : 2;
    info[6] = rebuilt ? RB.stack_bound : 0;
    info[7] = rebuilt ? RB.excluded : 0;
    info[8] = rebuilt ? RB.sphere_first : 0;
    info[9] = rebuilt ? RB.n_ray_spheres : 0;
    if (nodes) std::memcpy(nodes, N.data(), N.size() * sizeof(float4));
    if (prims) std::memcpy(prims, Pr.data(), Pr.size() * sizeof(float4));
    if (rank_code) std::memcpy(rank_code, rc.data(), rc.size() * sizeof(int));
    return CRT_OK;
}

// Per-rank shading records (layout in crt_device.h).  The triangle normal is unit(cross(e1, e2)) in the
// device's f32 operation order (the library is compiled with -ffp-contract=off and IEEE sqrt / division on
// the host too), so the record holds exactly the value shade() used to compute per hit.
// What shade() needs of material `mat`: its SHADE_* code and payload (crt_device.h); an index outside the scene's
// materials is SHADE_INVALID.  The one source of the per-rank shading records and of the per-material rows of the path
// steps (crt_paths.h), so both hold the same bits.
static uint32_t material_shade_row(const crt_scene_desc* D, uint32_t mat, float4& pay) {
    pay = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mat >= (uint32_t)D->n_materials) return SHADE_INVALID;
    const crt_material_desc& M = D->materials[mat];
    switch (M.type) {
        case CRT_LAMBERTIAN: pay = make_float4(M.albedo[0], M.albedo[1], M.albedo[2], 0.f); return SHADE_LAMBERT;
        case CRT_METAL:
            pay = make_float4(M.albedo[0], M.albedo[1], M.albedo[2], M.roughness < 1.f ? M.roughness : 1.f);
            return SHADE_METAL;
        case CRT_DIELECTRIC: {
            // Material.cuh:113 ri = front ? 1.0f / ior : ior, and Schlick's r0 = ((1 - ri) / (1 + ri))^2
            // (:133-134) for both faces, in IEEE f32 as the device would compute them per hit
            auto r0 = [](float r) { const float x = (1 - r) / (1 + r); return x * x; };
            const float inv = 1.0f / M.ior;
            pay = make_float4(M.ior, inv, r0(inv), r0(M.ior));
            return SHADE_DIELECTRIC;
        }
        case CRT_DIFFUSE_LIGHT: pay = make_float4(M.emission[0], M.emission[1], M.emission[2], 0.f); return SHADE_LIGHT;
        default: return SHADE_NOEMIT;
    }
}

// The path steps' per-material table: 2 x float4 per material, (code, 0, 0, 0) (payload).
static std::vector<float4> material_shade_rows(const crt_scene_desc* D) {
    std::vector<float4> out;
    out.reserve(2 * (size_t)std::max(D->n_materials, 0));
    for (int i = 0; i < D->n_materials; ++i) {
        float4 pay;
        const uint32_t code = material_shade_row(D, (uint32_t)i, pay);
        out.push_back(make_float4(i2f((int)code), 0.f, 0.f, 0.f));
        out.push_back(pay);
    }
    return out;
}

static std::vector<float4> shading_records(const std::vector<int>& rank_code, const std::vector<float4>& prims,
                                           const crt_scene_desc* D) {
    std::vector<float4> out(3 * rank_code.size(), make_float4(0.f, 0.f, 0.f, 0.f));
    parallel_ranges(rank_code.size(), [&](size_t rb, size_t re) {
        for (size_t r = rb; r < re; ++r) {
            const bool sphere = (rank_code[r] & SPHERE_BIT) != 0;
            const size_t p = (size_t)(rank_code[r] & ~SPHERE_BIT);
            const float4 f0 = prims[3 * p], f1 = prims[3 * p + 1], f2 = prims[3 * p + 2];
            const uint32_t mat = (uint32_t)i2i_host(sphere ? f1.y : f2.y);
            float4 pay;
            const uint32_t code = material_shade_row(D, mat, pay);
            float4 a;
            if (sphere) {
                a = make_float4(f0.x, f0.y, f0.z, i2f((int)(code | SHADE_SPHERE)));
                out[3 * r + 2] = make_float4(1 / f0.w, 0.f, 0.f, 0.f);
            } else {
                const float ux = f0.w, uy = f1.x, uz = f1.y, vx = f1.z, vy = f1.w, vz = f2.x;
                const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
                const float s = 1.0f / std::sqrt(cx * cx + cy * cy + cz * cz);
                a = make_float4(s * cx, s * cy, s * cz, i2f((int)code));
            }
            out[3 * r] = a;
            out[3 * r + 1] = pay;
        }
    });
    return out;
}

// Per-rank identity of the ray queries' hit record: (object, primitive, material, 0) of the primitive with reference
// DFS rank r.  Built from the Flattener alone, so it is the same table for every bvh mode of one description.
// object = mesh index, or -1 - index in D->spheres; primitive = triangle within its mesh after the build permutation
// (0 for a sphere); material = the record's material word (the index shade() uses, out of range or not).
static std::vector<int32_t> identity_table(const Flattener& F) {
    const size_t n_tri = F.prims.size() / 3 - F.sphere_of.size();
    std::vector<int32_t> out(4 * F.rank_code.size(), 0);
    for (size_t r = 0; r < F.rank_code.size(); ++r) {
        const bool sphere = (F.rank_code[r] & SPHERE_BIT) != 0;
        const size_t p = (size_t)(F.rank_code[r] & ~SPHERE_BIT);
        int32_t* o = out.data() + 4 * r;
        if (sphere) {
            o[0] = -1 - F.sphere_of[p - n_tri];
            o[1] = 0;
            o[2] = i2i_host(F.prims[3 * p + 1].y);
        } else {
            const size_t m = (size_t)(std::upper_bound(F.mesh_prim_base.begin(), F.mesh_prim_base.end(), (int)p) -
                                      F.mesh_prim_base.begin()) - 1;
            o[0] = (int32_t)m;
            o[1] = (int32_t)(p - (size_t)F.mesh_prim_base[m]);
            o[2] = i2i_host(F.prims[3 * p + 2].y);
        }
    }
    return out;
}

int crt_scene_export_identity(const crt_scene_desc* D, const crt_scene_options* opts, int32_t* out, int64_t* n_ranks) {
    if (!D || !n_ranks) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    crt_scene_options o;
    Flattener F{D};
    Rebuilt RB;
    if (int rc = build_scene_arrays(D, opts, o, F, RB, 0)) return rc;
    const std::vector<int32_t> id = identity_table(F);
    *n_ranks = (int64_t)F.rank_code.size();
    if (out)
        for (size_t r = 0; r < F.rank_code.size(); ++r) std::memcpy(out + 3 * r, id.data() + 4 * r, 3 * sizeof(int32_t));
    return CRT_OK;
}

int crt_scene_create_ex(const crt_scene_desc* D, int device, const crt_scene_options* opts, crt_scene** out) {
    if (!D || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    crt_scene_options o;
    Flattener F{D};
    Rebuilt RB;
    if (int rc = build_scene_arrays(D, opts, o, F, RB, device)) return rc;
    SetupTrace tr;
    const bool rebuilt = o.bvh == CRT_BVH_REBUILT;
    std::vector<float4> mats;
    for (int i = 0; i < D->n_materials; ++i) {
        const crt_material_desc& M = D->materials[i];
        mats.push_back(make_float4(i2f(M.type), M.albedo[0], M.albedo[1], M.albedo[2]));
        mats.push_back(make_float4(M.emission[0], M.emission[1], M.emission[2], M.roughness < 1.f ? M.roughness : 1.f));
        mats.push_back(make_float4(M.ior, 0.f, 0.f, 0.f));
    }
    if (int rc = use_device(device)) return rc;
    crt_scene* S = new (std::nothrow) crt_scene;
    if (!S) return set_error(CRT_ERR_OUT_OF_MEMORY, "host allocation failed");
    S->device = device;
    S->bvh = o.bvh;
    S->layouts = rebuilt ? o.layouts : 1;
    S->n_nodes = rebuilt ? RB.n_nodes : F.count();
    S->n_prims = (int)((rebuilt ? RB.prims : F.prims).size() / 3);
    S->n_ranks = (int)F.rank_code.size();
    S->n_mats = D->n_materials;
    S->max_depth = rebuilt ? RB.max_depth : F.max_depth;
    S->excluded = rebuilt ? RB.excluded : 0;
    S->width = rebuilt ? RB.width : 2;
    S->stack_cap = rebuilt ? (o.stack_cap > 0 ? o.stack_cap : RB.stack_bound) : 0;
    S->stack_bound = rebuilt ? RB.stack_bound : 0;
    S->sphere_first = rebuilt ? RB.sphere_first : 0;
    S->spatial_splits = rebuilt ? RB.spatial_splits : 0;
    S->references = rebuilt ? RB.references : 0;
    {
        int in_tree = 0;   // spheres the 4-wide tree itself holds (not tested per ray)
        if (rebuilt)
            for (int r = 0; r < (int)RB.rank_code.size(); ++r)
                if ((RB.rank_code[r] & SPHERE_BIT) && (RB.rank_code[r] & ~SPHERE_BIT) < RB.sphere_first) ++in_tree;
        S->tree_spheres = in_tree > 0 || !rebuilt;
    }
    if (rebuilt && RB.n_ray_spheres == 2) {
        for (int s = 0; s < 2; ++s) {
            const size_t q = 3 * (size_t)(RB.sphere_first + s);
            const float4 f0 = RB.prims[q], f1 = RB.prims[q + 1];
            const int k = i2i_host(f1.w);
            const float4 A = RB.chain[2 * (size_t)k], B = RB.chain[2 * (size_t)k + 1];
            const float v[12] = {f0.x, f0.y, f0.z, f1.x, f1.z, A.x, A.y, A.z, A.w, B.x, B.y, 0.f};
            std::memcpy(S->sph2[s], v, sizeof v);
        }
    }
    S->n_chain = rebuilt ? (int)(RB.chain.size() / 2) : 0;
    S->n_ray_spheres = rebuilt ? RB.n_ray_spheres : 0;
    auto up = [&](DevBuf<float4>& dst, const std::vector<float4>& src) -> hipError_t {
        hipError_t e = dst.alloc(src.size());
        if (e == hipSuccess && !src.empty())
            e = hipMemcpy(dst.get(), src.data(), src.size() * sizeof(float4), hipMemcpyHostToDevice);
        return e;
    };
    const std::vector<int>& rc = rebuilt ? RB.rank_code : F.rank_code;
    std::vector<float4> swizzled;   // width 4: row k of node n at slot k ^ (n & 7) of its record (node_row)
    if (S->width == 4) {
        swizzled.resize(RB.nodes.size());
        for (size_t n = 0; n < RB.nodes.size() / 8; ++n)
            for (size_t k = 0; k < 8; ++k) swizzled[8 * n + (k ^ (n & 7))] = RB.nodes[8 * n + k];
    }
    tr.lap("node swizzle");
    const std::vector<float4> shade = shading_records(rc, rebuilt ? RB.prims : F.prims, D);
    tr.lap("shading records");
    const std::vector<int32_t> ident = identity_table(F);
    const std::vector<float4> mat_rows = material_shade_rows(D);
    hipError_t e;
    if ((e = up(S->d_nodes, S->width == 4 ? swizzled : (rebuilt ? RB.nodes : F.nodes))) != hipSuccess ||
        (e = up(S->d_prims, rebuilt ? RB.prims : F.prims)) != hipSuccess ||
        (e = up(S->d_mats, mats)) != hipSuccess ||
        (e = up(S->d_chain, rebuilt ? RB.chain : std::vector<float4>())) != hipSuccess ||
        (e = up(S->d_shade, shade)) != hipSuccess ||
        (e = up(S->d_mat_rows, mat_rows)) != hipSuccess ||
        (e = S->d_ident.alloc(ident.size() / 4)) != hipSuccess ||   // four words per rank
        (!ident.empty() && (e = hipMemcpy(S->d_ident.get(), ident.data(), ident.size() * sizeof(int32_t),
                                          hipMemcpyHostToDevice)) != hipSuccess)) {
        crt_scene_destroy(S);
        return set_error(CRT_ERR_HIP, std::string("scene upload: ") + hipGetErrorString(e));
    }
    tr.lap("uploads");
    // the uploads above are null-stream copies: wait for them here, once per handle, so that a caller may trace or
    // render over the scene on any stream (a non-blocking one too) as soon as it holds the handle
    if ((e = hipStreamSynchronize(0)) != hipSuccess) {
        crt_scene_destroy(S);
        return set_error(CRT_ERR_HIP, std::string("scene upload: ") + hipGetErrorString(e));
    }
    *out = S;
    return CRT_OK;
}

int crt_scene_get_stats(const crt_scene* S, crt_scene_stats* out) {
    if (!S || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    out->device_nodes = (int64_t)S->n_nodes * S->layouts;
    out->width = S->width;
    out->stack_bound = S->stack_cap;
    out->spatial_splits = S->spatial_splits;
    out->references = S->references;
    out->device_prims = S->n_prims;
    out->device_bytes = (int64_t)S->n_nodes * S->layouts * (S->width == 4 ? 128 : 32) + (int64_t)S->n_prims * 48 + (int64_t)S->n_mats * 48 +
                        (int64_t)S->n_ranks * 48;
    out->max_depth = S->max_depth;
    out->n_materials = S->n_mats;
    out->bvh = S->bvh;
    out->layouts = S->layouts;
    out->excluded_prims = S->excluded;
    return CRT_OK;
}

void crt_scene_destroy(crt_scene* S) {
    if (!S) return;
    (void)hipSetDevice(S->device);
    delete S;
}

}  // extern "C"
