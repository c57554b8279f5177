// crt_hip.hip — MI355X (gfx950) render layer: kernels + the C ABI of include/crt_hip.h.
//
// Hot path: crt_render_kernel — one lane per pixel (8x8 pixel tile per wave64,
// 16x16 per 256-thread workgroup), the pixel's samples traced strictly in order
// so each pixel's XORWOW stream is consumed exactly as in the reference
// (CUDAKernels.h:147-166).  Inside a wave, lanes are decoupled at PATH-SEGMENT
// granularity: a lane whose path ends (miss, light, absorption, Russian
// roulette, max bounces) immediately starts its next sample, so every loop
// iteration traces one ray per live lane instead of idling until the longest
// path of the wave finishes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "crt_hip.h"
#include "crt_device.h"
#include "crt_devmem.h"
#include "crt_sah.h"
#include "crt/ParallelFor.h"

using namespace crt;

// ------------------------------------------------------------------ errors
static thread_local std::string g_last_error;
static int set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
int crtx_set_error(int code, const std::string& msg) { return set_error(code, msg); }   // crt_bvh_build.hip
int crtx_build_sah_gpu(int device, const std::vector<crt_sah::Item>& items, int leaf_size, float trav_cost,
                       std::vector<crt_sah::Node>* nodes_out, std::vector<int>* order_out, int* max_depth);
#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return set_error(CRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------------ kernels
struct RenderParams {
    const float4* __restrict__ nodes;
    const float4* __restrict__ prims;
    const float4* __restrict__ mats;
    const float4* __restrict__ shade;     // per reference DFS rank: shading record (crt_device.h)
    int n_nodes, n_mats, n_prims;         // n_nodes: nodes of ONE threaded layout
    int n_layouts;                        // 1, or 6 direction-ordered layouts (CRT_BVH_REBUILT)
    uint32_t* __restrict__ ovf;           // variant 4: traversal-stack entries beyond the LDS part
    int stack_cap;                        // variant 4: stack entries a ray can need (host bound)
    int stack_lds;                        // variant 4: entries kept in LDS (<= STACK_LDS; rest in ovf)
    int sphere_first, n_ray_spheres;      // variant 4: spheres tested per ray at generation (not in the BVH)
    int tree_spheres;                     // variant 4: the 4-wide tree's leaves hold spheres too
    const float4* __restrict__ sphere_chain;   // their reference scene-level leaf boxes (see ray_spheres)
    int n_chain;                                // boxes in sphere_chain
    // exactly two per-ray spheres (every reference scene: SceneManager's ground + metal sphere): their data
    // by value; the kernels stage it in LDS once, so a pass reads it with uniform LDS loads instead of two
    // dependent vector loads.  Per sphere: center.xyz, radius^2, rank bits, box lo.xyz, box hi.xyz, pad
    float sph2[2][12];
    unsigned* err;                // device error flag (bit 0: primitive index out of range)
    int width, height, spp, max_bounces;
    float rcp_w, rcp_h;           // next_ray's u = (x + U) / width by uv_div when fast_uv (crt_renderer_create)
    int fast_uv;
    int accumulate;
    int regen_threshold;          // variant 2: parked lanes needed before a shading/regeneration pass
    uint32_t* __restrict__ rng;   // W*H*6 (v0..v4, d)
    float* __restrict__ sum;      // W*H*3
    unsigned long long* __restrict__ counters;  // crt_work_counters layout
    crt_camera_desc cam;
    // variant 7 (persistent, 4-wide scenes): lanes take pixels from a global queue
    const uint32_t* __restrict__ order;   // slot -> pixel index (most expensive first, from the probe); ~0 = none
    uint32_t* __restrict__ queue;         // next unclaimed slot
    int n_slots;
    int tiles_x;                          // variant 8: 8x8 tiles per row (order[] holds tile indices)
    uint32_t* __restrict__ probe_cost;    // probe launch (variant 4): rays per pixel; nothing else is written
    int probe_stride;                     // probe launch (variant 4): lanes take every probe_stride-th pixel in x and y
    uint32_t* __restrict__ pix_rays;      // variant 7: rays each pixel took this frame (the next frame's tile order)
    int crit_tiles, crit_threshold;       // variant 8: the first crit_tiles tiles of the cost order regenerate at
                                          // crit_threshold parked lanes instead of regen_threshold
    int drain_threshold;                  // variant 7: the threshold once the pixel queue is empty
    int wave_drain;                       // variants 4/8: sixty-fourths of the live lanes a draining wave passes at
    int top_levels;                       // 4-wide variants: a new ray's first node steps taken from LDS (<= CRT_TOP_LEVELS)
};
// Variant 8's tail fill (crt_renderer_set_tail_fill, fill_prologue) reads its launch arguments from the fields of
// variant 7's pixel queue and of variant 4's probe, which no variant-8 kernel reads (a launch is one variant): the
// struct, and with it the argument layout of every kernel that takes it, stays as it is.
//   queue            null = no tail fill; else two counts (the tail parts rendered by the main launch and by the sweep),
//                    then one flag per rank of the cost order: 0, 1 = the head stored its state, 2 = the tail part is
//                    rendered
//   n_slots          blocks below it are heads (the launch's tiles; 0 in the sweep)
//   drain_threshold  K: the heads of the first K ranks hold back their last samples
//   probe_stride     delta: the samples they hold back
__device__ __forceinline__ uint32_t* fill_flags(const RenderParams& P) { return P.queue + 2; }
__device__ __forceinline__ uint32_t* fill_done(const RenderParams& P) { return P.queue + (P.n_slots ? 0 : 1); }
__device__ __forceinline__ uint32_t fill_heads(const RenderParams& P) { return (uint32_t)P.n_slots; }
__device__ __forceinline__ uint32_t fill_tiles(const RenderParams& P) { return (uint32_t)P.drain_threshold; }
__device__ __forceinline__ int fill_spp(const RenderParams& P) { return P.probe_stride; }

#ifdef CRT_PROFILE_LIVE
// profiling build (tools/live_histogram.py): variant 8's wave time by the number of lanes that still have samples,
// s_memtime cycles summed over waves in 9 buckets of 8 lanes (the last: 64)
__device__ unsigned long long g_live_hist[16];
#endif
#ifdef CRT_PROFILE_PAIRS
__device__ unsigned long long g_pair_hist[32];   // [0, 16): log2 buckets of leaf pairs per wave step; [16, 25): lanes / 8
#endif

struct TraceCounts {
    uint32_t boxes, tris, spheres, step_slots, round_slots, trace_calls;
    // COUNT-mode section profile (variant 4; wave-uniform shader-clock cycles, s_memtime)
    uint64_t cyc_regen, cyc_step, cyc_round, passes;
    uint64_t cyc_shade, cyc_next;   // inside the regen pass: ray_spheres() + shade(), next_ray(); the rest is ray init
    uint64_t cyc_sph;               // of cyc_shade: the per-ray spheres (ray_spheres)
    uint64_t cyc_setup, cyc_top, cyc_head;   // CRT_PROFILE_PASS: new-ray set-up, LDS root step, loop head
#ifdef CRT_PROFILE_ROWS
    uint64_t cyc_rows, cyc_prims;            // node-row and primitive-record load-to-data cycles (profiling build)
#endif
};
__device__ __forceinline__ uint64_t shader_clock() { return __builtin_amdgcn_s_memtime(); }
// Profiling build only (tools/build_profile_lib.sh pass -DCRT_PROFILE_PASS, tools/pass_profile.py): the section timers
// the counting kernel keeps (s_memtime per section) also in the timed kernel, with the regeneration pass split into
// its parts.  g_pass_prof, summed over variant 8's waves: [0] step, [1] rounds, [2] pass total, [3] finish_ray (spheres
// + shade), [4] of which the per-ray spheres, [5] next_ray, [6] new-ray set-up (1/d, rows, LDS ray record), [7] the
// LDS root step (top_steps), [8] loop head (live / parked ballots, the drain rule), [9] passes, [10] waves, [11] wave
// lifetime (first to last instruction), [12] node steps, [13] leaf rounds, [14] rays.  -DCRT_PROFILE_PASS_FIRST=K keeps
// only the first K workgroups of the tile order (K = 1: the most expensive tile, config B's critical chain).  With
// -DCRT_PROFILE_ROWS as well: [15] the node step's wait for its seven rows and [16] the leaf round's wait for its
// primitive records (the loads issued, then an explicit vmcnt(0) between two timers)
// a 64-bit value of one lane, to every lane (the profiling builds' timer accumulators)
__device__ __forceinline__ uint64_t bcast64(uint64_t v, int lane) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), lane) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}
#ifdef CRT_PROFILE_PASS
constexpr bool kProfilePass = true;
__device__ unsigned long long g_pass_prof[20];
#ifndef CRT_PROFILE_PASS_FIRST
#define CRT_PROFILE_PASS_FIRST 0x7fffffff
#endif
#else
constexpr bool kProfilePass = false;
#endif

// Hit rule shared by every variant and both BVH modes: a candidate (t, rank) replaces the current hit
// when t < closest, or t == closest and its reference DFS rank is higher.  In CRT_BVH_REFERENCE mode the
// traversal visits primitives in rank order, so this is exactly the reference's closed-interval
// acceptance (ties go to the later primitive); in CRT_BVH_REBUILT mode it reproduces that choice in
// any visiting order.
__device__ __forceinline__ bool better(float t, int rank, float closest, int hit) {
    return t < closest || (t == closest && rank > hit);
}

// Node array offset (in float4) of the threaded layout a ray walks: layout 2*axis + (d[axis] < 0) for the
// dominant axis of d when six direction-ordered layouts are resident, else 0.
__device__ __forceinline__ int layout_base(V3 d, int n_layouts, int n_nodes) {
    if (n_layouts == 1) return 0;
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const int l = (ax >= ay && ax >= az) ? (d.x < 0.f) : (ay >= az ? 2 + (d.y < 0.f) : 4 + (d.z < 0.f));
    return 2 * l * n_nodes;
}

// Closest hit over the threaded scene+mesh BVH.  Returns the reference DFS rank of the hit primitive
// or -1; `closest` = IntersectionTime of the accepted hit.
// Semantics: BVHNode::hit (BVHNode.cuh:115-156), Mesh::hit (Mesh.cuh:55-110),
// AABB::hit (AABB.cuh:123-146), rayTriangleIntersect (Mesh.cuh:266-308),
// Sphere::hit (Sphere.cuh:27-47); closed-interval acceptance so ties go to the
// later primitive, exactly as in the reference order.
template <bool COUNT>
__device__ __forceinline__ int trace(const float4* __restrict__ nodes, const float4* __restrict__ prims,
                                     int n_nodes, int nbase, V3 o, V3 d, float& closest, TraceCounts& cnt) {
    const float INF = __builtin_inff();
    // AABB::hit computes 1/d per node visit; the value is the same every time.
    const V3 inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    closest = INF;
    int hit = -1;
    int node = 0;
    while (node < n_nodes) {
        const float4 A = nodes[nbase + 2 * node];
        const float4 B = nodes[nbase + 2 * node + 1];
        const int a = __float_as_int(B.z);
        const int b = __float_as_int(B.w);
        const bool scene_level = (b == NODE_SCENE_INNER) || (b >= SPHERE_BIT);
        const float tcl = scene_level ? INF : closest;
        if (COUNT) cnt.boxes++;
        const float t0x = (A.x - o.x) * inv.x, t0y = (A.y - o.y) * inv.y, t0z = (A.z - o.z) * inv.z;
        const float t1x = (A.w - o.x) * inv.x, t1y = (B.x - o.y) * inv.y, t1z = (B.y - o.z) * inv.z;
        float tmin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
        float tmax = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
        tmin = fmaxf(tmin, 0.001f);
        tmax = fminf(tmax, tcl);
        const bool box_hit = !(tmax <= tmin);
        int next = node + 1;
        if (b < 0) {
            if (!box_hit) next = a;
        } else if (box_hit) {
            if (b >= SPHERE_BIT) {
                const int p = b - SPHERE_BIT;
                if (COUNT) cnt.spheres++;
                const float4 f0 = prims[3 * p], f1 = prims[3 * p + 1];
                const V3 oc = o - v3(f0.x, f0.y, f0.z);
                const float qa = dot(d, d);
                const float hb = dot(oc, d);
                const float qc = dot(oc, oc) - f1.x;
                const float disc = hb * hb - qa * qc;
                if (!(disc < 0)) {
                    const float sq = sqrt_exact_wave(disc);
                    float root = (-hb - sq) / qa;
                    bool ok = true;
                    if (root < 0.001f || root > closest) {
                        root = (-hb + sq) / qa;
                        if (root < 0.001f || root > closest) ok = false;
                    }
                    const int rank = __float_as_int(f1.z);
                    if (ok && better(root, rank, closest, hit)) { closest = root; hit = rank; }
                }
            } else {
                for (int k = 0; k < a; ++k) {
                    const int p = b + k;
                    if (COUNT) cnt.tris++;
                    const float4 f0 = prims[3 * p], f1 = prims[3 * p + 1], f2 = prims[3 * p + 2];
                    const V3 e1 = v3(f0.w, f1.x, f1.y);
                    const V3 e2 = v3(f1.z, f1.w, f2.x);
                    const V3 h = cross(d, e2);
                    const float det = dot(e1, h);
                    if (fabsf(det) < 1e-8f) continue;
                    const float f = 1.f / det;
                    const V3 s = o - v3(f0.x, f0.y, f0.z);
                    const float u = f * dot(s, h);
                    if (u < 0.f || u > 1.f) continue;
                    const V3 q = cross(s, e1);
                    const float v = f * dot(d, q);
                    if (v < 0.f || (u + v) > 1.f) continue;
                    const float t = f * dot(e2, q);
                    if (t < 0.001f || t > closest) continue;
                    const int rank = __float_as_int(f2.z);
                    if (!better(t, rank, closest, hit)) continue;
                    closest = t;
                    hit = rank;
                }
            }
        }
        node = next;
    }
    return hit;
}

// Lanes of the wave (active lanes only) whose predicate holds.  HIP's __ballot widens the predicate to an int and
// compares it again (two VALU per ballot); the builtin takes the compare's lane mask as it is.
__device__ __forceinline__ uint64_t wave_ballot(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t x) {
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// ---------------------------------------------------------------- wave helpers
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Wave64 inclusive scans with DPP (no LDS traffic): Kogge-Stone inside each 16-lane row
// (row_shr 1,2,4,8 with identity fill), then row_bcast15 / row_bcast31 carry the row totals.
// Same sequence as LLVM's AMDGPU atomic optimizer uses on gfx9.
#define CRT_DPP_ROW_SHR(n) (0x110 | (n))
#define CRT_DPP_BCAST15 0x142
#define CRT_DPP_BCAST31 0x143
// bound_ctrl: a lane whose source is out of range reads 0 (the identity), so LLVM's DPP combiner can fold
// each step into one v_add_u32_dpp / v_max_u32_dpp instead of v_mov (identity) + v_mov_dpp + the op.
__device__ __forceinline__ int wave_inclusive_scan(int x, int /*lane*/) {
    x += __builtin_amdgcn_update_dpp(0, x, CRT_DPP_ROW_SHR(1), 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, CRT_DPP_ROW_SHR(2), 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, CRT_DPP_ROW_SHR(4), 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, CRT_DPP_ROW_SHR(8), 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, CRT_DPP_BCAST15, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, CRT_DPP_BCAST31, 0xc, 0xf, false);
    return x;
}
// The same scan as six in-place v_add_u32_dpp.  In traverse_step4 the combiner leaves the builtin form as v_mov_dpp +
// v_add pairs (it reuses the partial sums for the exclusive prefix): 14 VALU instead of 6.  The s_nops are the
// VALU-write -> DPP-read wait states, which the compiler does not insert inside an asm block.
__device__ __forceinline__ int wave_inclusive_scan_dpp(int x) {
    __asm__ volatile(
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
        : "+v"(x));
    return x;
}
// Inclusive max-scan of non-negative values (0 = none) with the same structure.
__device__ __forceinline__ uint32_t wave_inclusive_max_scan_u(uint32_t x) {
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CRT_DPP_ROW_SHR(1), 0xf, 0xf, true));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CRT_DPP_ROW_SHR(2), 0xf, 0xf, true));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CRT_DPP_ROW_SHR(4), 0xf, 0xf, true));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CRT_DPP_ROW_SHR(8), 0xf, 0xf, true));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CRT_DPP_BCAST15, 0xa, 0xf, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CRT_DPP_BCAST31, 0xc, 0xf, false));
    return x;
}
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
// Reference (ds_bpermute) form, used by the scan self-test.
__device__ __forceinline__ int wave_inclusive_scan_shfl(int x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    return x;
}

// Per-wave LDS for the cooperative leaf step.
struct WaveLds {
    float4 ray0[64];                 // o.x, o.y, o.z, d.x of each lane's ray
    float4 ray1[64];                 // d.y, d.z, closest at leaf entry, first prim (int bits)
    unsigned long long key[64];      // per owner: (t bits << 32) | (0xffffffff - rank), min-reduced
    int prefix[64];                  // first pair index of each owner's leaf
    unsigned char owner_at[64];      // owner lane of the pair that starts at each slot of a round
};
// The 4-wide kernels' per-wave LDS (traverse_step4): WaveLds without the owners' pair prefixes, which the fast build
// keeps in the ray records (ray1.w), so the 256 B go to the top nodes (CRT_TOP_LEVELS) within occupancy 6.
struct WaveLdsWide {
    float4 ray0[64];
    float4 ray1[64];
    unsigned long long key[64];
    unsigned char owner_at[64];
    uint32_t rays;                   // variant 8: the wave's ray count (in LDS, not a VGPR live across the loop)
#ifdef CRT_CHECKED
    int prefix[64];                  // checked build: each owner's first pair index and pair count
    int span_n[64];
#endif
};

// Möller–Trumbore (Mesh.cuh:266-308) on a triangle record; returns t or -1 when rejected (any accepted
// t >= 0.001).
__device__ __forceinline__ float tri_test_rec(float4 f0, float4 f1, float4 f2, V3 o, V3 d, float tmax) {
    const V3 e1 = v3(f0.w, f1.x, f1.y);
    const V3 e2 = v3(f1.z, f1.w, f2.x);
    const V3 h = cross(d, e2);
    const float det = dot(e1, h);
    if (fabsf(det) < 1e-8f) return -1.f;
    const float f = recip_exact(det);          // == 1.f / det bit for bit (see crt_device.h)
    const V3 s = o - v3(f0.x, f0.y, f0.z);
    const float u = f * dot(s, h);
    if (u < 0.f || u > 1.f) return -1.f;
    const V3 q = cross(s, e1);
    const float v = f * dot(d, q);
    if (v < 0.f || (u + v) > 1.f) return -1.f;
    const float t = f * dot(e2, q);
    if (t < 0.001f || t > tmax) return -1.f;
    return t;
}
// The same test without early exits, for the leaf rounds: u, v and t are pure functions of the record and the ray, so
// computing them on every lane and rejecting once returns the same value (the reject predicate keeps the reference's
// comparisons, NaN included).  1/det by rcp_newton when every active lane's |det| is below 2^126 (a wave-uniform
// choice; lanes with |det| < 1e-8 are rejected whatever f is), else by IEEE division.
__device__ __forceinline__ float tri_test_flat(float4 f0, float4 f1, float4 f2, V3 o, V3 d, float tmax) {
    const V3 e1 = v3(f0.w, f1.x, f1.y);
    const V3 e2 = v3(f1.z, f1.w, f2.x);
    const V3 h = cross(d, e2);
    const float det = dot(e1, h);
    const float a = fabsf(det);
    float f;
    if (__builtin_amdgcn_ballot_w64(!(a < RCP_FAST_MAX)) == 0) {
        f = rcp_newton(det);
    } else {
        __asm__ volatile("");
        f = 1.0f / det;
    }
    const V3 s = o - v3(f0.x, f0.y, f0.z);
    const float u = f * dot(s, h);
    const V3 q = cross(s, e1);
    const float v = f * dot(d, q);
    const float t = f * dot(e2, q);
    const bool rej = (a < 1e-8f) | (u < 0.f) | (u > 1.f) | (v < 0.f) | ((u + v) > 1.f) | (t < 0.001f) | (t > tmax);
    return rej ? -1.f : t;
}
__device__ __forceinline__ float tri_test(const float4* __restrict__ prims, int p, V3 o, V3 d, float tmax, int& rank) {
    const float4 f0 = prims[3 * p], f1 = prims[3 * p + 1], f2 = prims[3 * p + 2];
    rank = __float_as_int(f2.z);
    return tri_test_rec(f0, f1, f2, o, d, tmax);
}

// Sphere::hit (Sphere.cuh:27-47) as a candidate: the root it would accept against any closest >= the
// result (the near root if >= 0.001, else the far one), or -1.  Independent of the visiting order, so
// it can enter the same min-reduction as triangles.
__device__ __forceinline__ float sphere_candidate(float4 f0, float4 f1, V3 o, V3 d, float tmax) {
    const V3 oc = o - v3(f0.x, f0.y, f0.z);
    const float qa = dot(d, d);
    const float hb = dot(oc, d);
    const float qc = dot(oc, oc) - f1.x;
    const float disc = hb * hb - qa * qc;
    if (disc < 0) return -1.f;
    const float sq = sqrt_exact_wave(disc);
    float root = (-hb - sq) / qa;
    if (root < 0.001f || root > tmax) {
        root = (-hb + sq) / qa;
        if (root < 0.001f || root > tmax) return -1.f;
    }
    return root;
}

// Any primitive of a CRT_BVH_REBUILT leaf: triangle, or sphere (record word 11 == 1; only when the tree
// holds spheres — a uniform flag, so triangle-only trees skip the branch).
// Record at a 32-bit byte offset from a uniform base: the load takes the SGPR base + VGPR offset form, no
// 64-bit address arithmetic per lane (the host keeps primitive and 4-wide node arrays below 4 GiB).
__device__ __forceinline__ const float4* rec_at(const float4* base, uint32_t byte_off) {
    return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + byte_off);
}

// (Storing the records as three planes of float4, for contiguous 16-B words per load, measured 2.7 % slower: the three
// planes are three cache lines per triangle where the 48-B record mostly sits in one, profiles/r02c.)
__device__ __forceinline__ float prim_test(const float4* __restrict__ prims, int p, V3 o, V3 d, float tmax, int& rank,
                                           bool tree_spheres = true) {
    // 24-bit multiply (full rate; v_mul_lo_u32 is quarter rate): the 4-wide tree holds < 2^24 primitives (emit4)
    const float4* r = rec_at(prims, __umul24((uint32_t)p, 48u));
    const float4 f0 = r[0], f1 = r[1], f2 = r[2];
    // keep the unused word: the third row then loads as one dwordx4 instead of a dword + a dwordx2 (one vector-L1
    // lookup set less per pair; -0.7 %, profiles/r02s)
    __asm__ volatile("" : : "v"(f2.y));
    rank = __float_as_int(f2.z);
    if (tree_spheres && __float_as_int(f2.w) == 1) return sphere_candidate(f0, f1, o, d, tmax);
    // without early exits: the leaf rounds are full of lanes, so the exits only cost branches (-0.75 %, profiles/r02ap)
    return tri_test_flat(f0, f1, f2, o, d, tmax);
}

// Sphere::hit (Sphere.cuh:27-47) against [0.001, closest]; updates closest/hit (= rank) on acceptance.
__device__ __forceinline__ void sphere_test(const float4* __restrict__ prims, int b, V3 o, V3 d, float& closest, int& hit) {
    const int p = b - SPHERE_BIT;
    const float4 f0 = prims[3 * p], f1 = prims[3 * p + 1];
    const V3 oc = o - v3(f0.x, f0.y, f0.z);
    const float qa = dot(d, d);
    const float hb = dot(oc, d);
    const float qc = dot(oc, oc) - f1.x;
    const float disc = hb * hb - qa * qc;
    if (disc < 0) return;
    const float sq = sqrt_exact_wave(disc);
    float root = (-hb - sq) / qa;
    if (root < 0.001f || root > closest) {
        root = (-hb + sq) / qa;
        if (root < 0.001f || root > closest) return;
    }
    const int rank = __float_as_int(f1.z);
    if (!better(root, rank, closest, hit)) return;
    closest = root;
    hit = rank;
}

// Variant 1: per-lane threaded traversal, leaf triangles tested cooperatively by the whole wave.
// Every lane that reaches a mesh leaf in a step contributes its (lane, triangle) pairs; the wave
// tests 64 pairs per round and min-reduces (t, later-index-wins) per owner in LDS.  Within one
// leaf a triangle's acceptance depends only on the closest hit at leaf entry, so the result is
// the same closest hit (ties to the later triangle) as Mesh::hit's sequential loop.
// MUST be called by all 64 lanes (inactive lanes pass active=false).
template <bool COUNT>
__device__ int trace_coop(const float4* __restrict__ nodes, const float4* __restrict__ prims, int n_nodes, int nbase,
                          int n_prims, unsigned* err, V3 o, V3 d, bool active, float& closest, TraceCounts& cnt,
                          WaveLds& L, int lane) {
    const float INF = __builtin_inff();
    const V3 inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    closest = INF;
    int hit = -1;
    int node = active ? 0 : n_nodes;
    L.ray0[lane] = make_float4(o.x, o.y, o.z, d.x);
    L.owner_at[lane] = 0;      // owner + 1, 0 = none
    if (COUNT) cnt.trace_calls++;
    while (wave_ballot(node < n_nodes)) {
        if (COUNT) cnt.step_slots++;        // one traversal step of the wave (x64 lanes)
        int leaf_n = 0, leaf_first = 0;
        if (node < n_nodes) {
            const float4 A = nodes[nbase + 2 * node];
            const float4 B = nodes[nbase + 2 * node + 1];
            const int a = __float_as_int(B.z);
            const int b = __float_as_int(B.w);
            const bool scene_level = (b == NODE_SCENE_INNER) || (b >= SPHERE_BIT);
            const float tcl = scene_level ? INF : closest;
            if (COUNT) cnt.boxes++;
            const float t0x = (A.x - o.x) * inv.x, t0y = (A.y - o.y) * inv.y, t0z = (A.z - o.z) * inv.z;
            const float t1x = (A.w - o.x) * inv.x, t1y = (B.x - o.y) * inv.y, t1z = (B.y - o.z) * inv.z;
            float tmin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
            float tmax = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
            tmin = fmaxf(tmin, 0.001f);
            tmax = fminf(tmax, tcl);
            const bool box_hit = !(tmax <= tmin);
            int next = node + 1;
            if (b < 0) {
                if (!box_hit) next = a;
            } else if (box_hit) {
                if (b >= SPHERE_BIT) {
                    if (COUNT) cnt.spheres++;
                    sphere_test(prims, b, o, d, closest, hit);
                } else {
                    leaf_n = a;
                    leaf_first = b;
                }
            }
            node = next;
        }
        if (!wave_ballot(leaf_n > 0)) continue;
        const int incl = wave_inclusive_scan(leaf_n, lane);
        const int total = __builtin_amdgcn_readlane(incl, 63);
        const int pfx = incl - leaf_n;
        if (leaf_n > 0) {
            L.ray1[lane] = make_float4(d.y, d.z, closest, __int_as_float(leaf_first));
            L.prefix[lane] = pfx;
            L.key[lane] = ~0ull;
        }
        uint32_t carry = 0;   // owner + 1 of the last pair of the previous round
        for (int base = 0; base < total; base += 64) {
            if (COUNT) cnt.round_slots++;
            // owner of pair (base + lane): lanes whose leaf starts in this round mark their start slot,
            // then an inclusive max-scan over slots (owners are increasing in slot order) fills the gaps;
            // slots before the first start of the round belong to the previous round's last owner.
            if (leaf_n > 0 && pfx >= base && pfx < base + 64) L.owner_at[pfx - base] = (unsigned char)(lane + 1);
            wave_sync();
            const uint32_t mark = L.owner_at[lane];
            L.owner_at[lane] = 0;                     // reset own slot for the next round
            const uint32_t owner1 = max(wave_inclusive_max_scan_u(mark), carry);
            const int owner = (int)owner1 - 1;
            const int j = base + lane;
            if (j < total) {
                const float4 r0 = L.ray0[owner], r1 = L.ray1[owner];
                const int k = j - L.prefix[owner];
                const int p = __float_as_int(r1.w) + k;
                if (COUNT) cnt.tris++;
                if ((unsigned)p < (unsigned)n_prims && (unsigned)k < 0xffffffffu) {
                    int rank;
                    const float t = tri_test(prims, p, v3(r0.x, r0.y, r0.z), v3(r0.w, r1.x, r1.y), r1.z, rank);
                    if (t >= 0.f)
                        atomicMin(&L.key[owner], ((unsigned long long)__float_as_uint(t) << 32) | (0xffffffffu - (unsigned)rank));
                } else {
                    atomicOr(err, 1u);                // indexing bug: report instead of faulting
                }
            }
            carry = __builtin_amdgcn_readlane(owner1, 63);
            wave_sync();
        }
        if (leaf_n > 0) {
            const unsigned long long kk = L.key[lane];
            const float t = __uint_as_float((unsigned)(kk >> 32));
            const int rank = (int)(0xffffffffu - (unsigned)kk);
            if (kk != ~0ull && better(t, rank, closest, hit)) {
                closest = t;
                hit = rank;
            }
        }
    }
    return hit;
}

// One wave traversal step (variant 2): every lane with node < n_nodes tests one node; the leaves
// reached in this step are intersected cooperatively (same rounds as trace_coop).  All 64 lanes call it.
// PREFETCH: the caller keeps the current node's 32 B in (pA, pB); the next node is loaded right after
// the box test so its latency overlaps this step's leaf rounds.
template <bool COUNT, bool PREFETCH>
__device__ __forceinline__ void traverse_step(const float4* __restrict__ nodes, const float4* __restrict__ prims,
                                              int n_nodes, int nbase, int n_prims, unsigned* err, V3 o, V3 d,
                                              V3 inv, int& node, float& closest, int& hit, TraceCounts& cnt,
                                              WaveLds& L, int lane, float4& pA, float4& pB) {
    const float INF = __builtin_inff();
    if (COUNT) cnt.step_slots++;
    int leaf_n = 0, leaf_first = 0;
    if (node < n_nodes) {
        const float4 A = PREFETCH ? pA : nodes[nbase + 2 * node];
        const float4 B = PREFETCH ? pB : nodes[nbase + 2 * node + 1];
        const int a = __float_as_int(B.z);
        const int b = __float_as_int(B.w);
        const bool scene_level = (b == NODE_SCENE_INNER) || (b >= SPHERE_BIT);
        const float tcl = scene_level ? INF : closest;
        if (COUNT) cnt.boxes++;
        const float t0x = (A.x - o.x) * inv.x, t0y = (A.y - o.y) * inv.y, t0z = (A.z - o.z) * inv.z;
        const float t1x = (A.w - o.x) * inv.x, t1y = (B.x - o.y) * inv.y, t1z = (B.y - o.z) * inv.z;
        float tmin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
        float tmax = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
        tmin = fmaxf(tmin, 0.001f);
        tmax = fminf(tmax, tcl);
        const bool box_hit = !(tmax <= tmin);
        int next = node + 1;
        if (b < 0) {
            if (!box_hit) next = a;
        } else if (box_hit) {
            if (b >= SPHERE_BIT) {
                if (COUNT) cnt.spheres++;
                sphere_test(prims, b, o, d, closest, hit);
            } else {
                leaf_n = a;
                leaf_first = b;
            }
        }
        node = next;
        if (PREFETCH && next < n_nodes) {
            pA = nodes[nbase + 2 * next];
            pB = nodes[nbase + 2 * next + 1];
        }
    }
    if (!wave_ballot(leaf_n > 0)) return;
    const int incl = wave_inclusive_scan_dpp(leaf_n);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    const int pfx = incl - leaf_n;
    if (leaf_n > 0) {
        L.ray1[lane] = make_float4(d.y, d.z, closest, __int_as_float(leaf_first));
        L.prefix[lane] = pfx;
        L.key[lane] = ~0ull;
    }
    uint32_t carry = 0;   // owner + 1 of the last pair of the previous round
    for (int base = 0; base < total; base += 64) {
        if (COUNT || kProfilePass) cnt.round_slots++;
        if (leaf_n > 0 && pfx >= base && pfx < base + 64) L.owner_at[pfx - base] = (unsigned char)(lane + 1);
        wave_sync();
        const uint32_t mark = L.owner_at[lane];
        L.owner_at[lane] = 0;
        const uint32_t owner1 = max(wave_inclusive_max_scan_u(mark), carry);
        const int owner = (int)owner1 - 1;
        const int j = base + lane;
        if (j < total) {
            const float4 r0 = L.ray0[owner], r1 = L.ray1[owner];
            const int k = j - L.prefix[owner];
            const int p = __float_as_int(r1.w) + k;
            if (COUNT) cnt.tris++;
            if ((unsigned)p < (unsigned)n_prims) {
                int rank;
                const float t = tri_test(prims, p, v3(r0.x, r0.y, r0.z), v3(r0.w, r1.x, r1.y), r1.z, rank);
                if (t >= 0.f)
                    atomicMin(&L.key[owner], ((unsigned long long)__float_as_uint(t) << 32) | (0xffffffffu - (unsigned)rank));
            } else {
                atomicOr(err, 1u);
            }
        }
        carry = __builtin_amdgcn_readlane(owner1, 63);
        wave_sync();
    }
    if (leaf_n > 0) {
        const unsigned long long kk = L.key[lane];
        const float t = __uint_as_float((unsigned)(kk >> 32));
        const int rank = (int)(0xffffffffu - (unsigned)kk);
        if (kk != ~0ull && better(t, rank, closest, hit)) {
            closest = t;
            hit = rank;
        }
    }
}

// ------------------------------------------------------------------ 4-wide BVH (CRT_BVH_REBUILT)
// Node = 8 x float4 (128 B): child boxes as SoA rows (lo.x[4], hi.x[4], lo.y[4], hi.y[4], lo.z[4],
// hi.z[4]), then meta = (first_child, n_internal | n_slots << 8, leaf_first, 8-bit triangle count per
// slot), then padding.  Slots [0, n_internal) are internal children at node first_child + slot; the
// following slots are leaves whose primitives are consecutive from leaf_first in slot order; empty slots
// have a zero-thickness box far away (never hit).
// crt_render: variant 8 below 4 tiles per wave slot runs at occupancy 4 with the row prefetch when the probe's largest
// tile work exceeds CRT_CHAIN_RHO times the mean work per occupancy-6 wave slot (a chain-bound frame), else at 6
#ifndef CRT_CHAIN_RHO
#define CRT_CHAIN_RHO 1.6   // profiles/r06y: occupancy 4 won at rho 1.62-6.4 and lost at 0.79-1.55 (one exception, -2 % at 1.54)
#endif
constexpr int STACK_LDS = 16;   // per-lane traversal-stack entries kept in LDS; deeper entries go to P.ovf
#ifndef CRT_STACK6
#define CRT_STACK6 12           // entries at occupancy 6 (6 one-wave workgroups per SIMD within 160 KiB: <= 6144 B each)
#endif
#ifndef CRT_STACK7
#define CRT_STACK7 8            // entries at occupancy 7: LDS is allocated in 1-KiB steps, so 28 one-wave workgroups per
                                // CU need <= 5,120 B each (variant 8: 5,024 B; 9 entries, 5,280 B, stay at 6 per SIMD,
                                // profiles/r03ah)
#endif
// LDS stack entries per lane of the 4-wide kernels built for an occupancy target of minw waves per SIMD
constexpr int wide_stack_entries(int minw) { return minw >= 7 ? CRT_STACK7 : minw >= 6 ? CRT_STACK6 : STACK_LDS; }
// The renderer's default regeneration knobs of the 4-wide variants (crt_renderer_set_regen_threshold,
// crt_renderer_set_wave_drain).  The frozen render kernels (crt_render_body.inc) hold them as constants.
constexpr int REGEN_THRESHOLD_WIDE = 44;   // measured: 40 for variant 4, profiles/r01d; 44-48 for 8, r01af
constexpr int WAVE_DRAIN = 48;             // draining waves pass at 48/64 of their live lanes (profiles/r04n)
// Tail fill's automatic choice (render_tiles, crt_renderer_set_tail_fill with tiles < 0; measured: profiles/tail_fill):
// the first NUM/DEN of the cost order hold back spp / SPP_DEN samples (config C: the first half, 125 of 2000 samples,
// -3.3 %; 250 of them -2.7 %, 500 -2.2 %; a quarter or three quarters of the tiles at 250: -2.8 %).  Every part ends
// with its wave's own drain, whose share of the part grows as the part shrinks; the smallest part measured (15 samples,
// the first half of a 250-spp frame: -1.8 %) still gained, nothing below it was measured, so a render whose parts
// would hold fewer than MIN_SPP samples (one of fewer than 192 samples) keeps the plain launch.
#ifndef CRT_FILL_AUTO
#define CRT_FILL_AUTO 1
#endif
constexpr int CRT_FILL_TILES_NUM = 1, CRT_FILL_TILES_DEN = 2, CRT_FILL_SPP_DEN = 16, CRT_FILL_MIN_SPP = 12;

struct Wide4 {
    float tmin[4];
    bool hit[4];
};

// Slab test of the four child boxes against [0.001, tmax]: plane * inv - o * inv as one fma per plane (one operation
// where (lo - o) * inv takes two; measured -2.1 %, profiles/r01at).  Its error, about ulp(o) * |inv|
// in t, is of the same order as that of (lo - o) * inv and far inside the boxes' 1e-5 * max(1, |coord|) padding
// (DESIGN.md §2b).  inv must be finite AND o * inv / lo * inv must not overflow: an infinite product makes
// lo * inv - o * inv = inf - inf = NaN on a plane, and the min/max would then cull a box the ray runs inside of.
// The traversal's 1/d is therefore the exact 1/d clamped to +-2^64 (box_inv): a plane keeps its sign and a magnitude
// >= padding * 2^64, far above the rounding, and |coord| * 2^64 stays finite for every |coord| < 2^60, the bound
// crt_scene_create_ex enforces on the rebuilt tree's boxes (every later ray origin is a hit point inside them) and
// crt_renderer_set_camera on the primary rays' origins (camera origin + lens offset, below 2^59 + 2^58).
constexpr float BOX_INV_CLAMP = 0x1p64f;
__device__ __forceinline__ V3 box_inv(V3 inv) {
    return v3(__builtin_amdgcn_fmed3f(inv.x, -BOX_INV_CLAMP, BOX_INV_CLAMP),
              __builtin_amdgcn_fmed3f(inv.y, -BOX_INV_CLAMP, BOX_INV_CLAMP),
              __builtin_amdgcn_fmed3f(inv.z, -BOX_INV_CLAMP, BOX_INV_CLAMP));
}
// 1/d of a new ray, each component == 1.f / x bit for bit: rcp_newton when every active lane's three components lie in
// its verified range (a wave-uniform branch), else recip_exact_any per component (-0.33 %, profiles/r02av).
__device__ __forceinline__ V3 recip3_exact(V3 d) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const bool ok = ax >= RCP_FAST_MIN && ax < RCP_FAST_MAX && ay >= RCP_FAST_MIN && ay < RCP_FAST_MAX &&
                    az >= RCP_FAST_MIN && az < RCP_FAST_MAX;
    if (__builtin_amdgcn_ballot_w64(!ok) == 0) return v3(rcp_newton(d.x), rcp_newton(d.y), rcp_newton(d.z));
    __asm__ volatile("");
    return v3(recip_exact_any(d.x), recip_exact_any(d.y), recip_exact_any(d.z));
}
// The per-ray spheres' exact 1/d (their reference box test) from the traversal's box_inv: recomputed only when a
// component was clamped.
__device__ __forceinline__ V3 sphere_inv(V3 d, V3 binv) {
    if (fabsf(binv.x) == BOX_INV_CLAMP || fabsf(binv.y) == BOX_INV_CLAMP || fabsf(binv.z) == BOX_INV_CLAMP)
        return v3(recip_exact_any(d.x), recip_exact_any(d.y), recip_exact_any(d.z));
    return binv;
}
// Row k of 4-wide node n sits at 16-B slot k ^ (n & 7) of the node's 128-B record (swizzled at upload,
// crt_scene_create_ex).  One wave instruction loads row k of up to 64 different nodes; at a fixed slot every lane reads
// the same 16-B offset of its line, and the vector L1 then serves about one lane per cycle (tools/probes/l1_probe,
// profiles/r02c: 62 cycles per instruction for that shape against 38 for random offsets).  b = node_base(n).
__device__ __forceinline__ uint32_t node_base(int node) { return ((uint32_t)node << 7) | (((uint32_t)node & 7u) << 4); }
__device__ __forceinline__ float4 node_row(const float4* __restrict__ nodes, uint32_t b, uint32_t k) {
    return *rec_at(nodes, b ^ (k << 4));
}
// The slab test by the ray's direction signs: for axis a, the row of the four child planes the ray enters first (lo
// for inv >= 0, hi for inv < 0) is row 2a ^ sign_a, and the row it leaves by is the other one.  fma(plane, inv, -o*inv)
// is monotone in the plane, so the entry row's t values are exactly min(t_lo, t_hi) and the exit row's exactly
// max(t_lo, t_hi): the same box hits and tmin as the min/max form, bit for bit, without its 24 min/max per node.  The
// row choice is an address bit (the sign of inv, shifted to the row's 16-B slot), not a select.
__device__ __forceinline__ uint32_t sign_row(float inv) { return (__float_as_uint(inv) >> 27) & 16u; }
// The ray's entry-row offsets for the three axes, one byte each (row 2a ^ sign, in 16-B units), computed once per
// ray: a node step then needs one xor per row address instead of re-deriving the signs.
__device__ __forceinline__ uint32_t ray_rows(V3 inv) {
    return sign_row(inv.x) | ((32u ^ sign_row(inv.y)) << 8) | ((64u ^ sign_row(inv.z)) << 16);
}
__device__ __forceinline__ Wide4 wide_boxes_of(const float4& nxr, const float4& fxr, const float4& nyr, const float4& fyr,
                                               const float4& nzr, const float4& fzr, V3 o, V3 inv, float tmax);
__device__ __forceinline__ Wide4 wide_boxes(const float4* __restrict__ nodes, uint32_t b, uint32_t rows, V3 o, V3 inv,
                                            float tmax) {
    const uint32_t ex = b ^ (rows & 0xffu), ey = b ^ ((rows >> 8) & 0xffu), ez = b ^ (rows >> 16);
    const float4 nxr = *rec_at(nodes, ex), fxr = *rec_at(nodes, ex ^ 16u);
    const float4 nyr = *rec_at(nodes, ey), fyr = *rec_at(nodes, ey ^ 16u);
    const float4 nzr = *rec_at(nodes, ez), fzr = *rec_at(nodes, ez ^ 16u);
    return wide_boxes_of(nxr, fxr, nyr, fyr, nzr, fzr, o, inv, tmax);
}
// The rows of node b for the row prefetch of variant 8 at occupancy 4 (traverse_step4<.., true>): pf[0..5] = the ray's
// entry / exit rows per axis (the order wide_boxes_of takes), pf[6] = the link row.
__device__ __forceinline__ void load_node_rows(const float4* __restrict__ nodes, uint32_t b, uint32_t rows, float4* pf) {
    const uint32_t ex = b ^ (rows & 0xffu), ey = b ^ ((rows >> 8) & 0xffu), ez = b ^ (rows >> 16);
    pf[0] = *rec_at(nodes, ex); pf[1] = *rec_at(nodes, ex ^ 16u);
    pf[2] = *rec_at(nodes, ey); pf[3] = *rec_at(nodes, ey ^ 16u);
    pf[4] = *rec_at(nodes, ez); pf[5] = *rec_at(nodes, ez ^ 16u);
    pf[6] = *rec_at(nodes, b ^ (6u << 4));
}
__device__ __forceinline__ Wide4 wide_boxes_of(const float4& nxr, const float4& fxr, const float4& nyr, const float4& fyr,
                                               const float4& nzr, const float4& fzr, V3 o, V3 inv, float tmax) {
    // one v_fma_f32 per plane: a v_pk_fma_f32 costs the SIMD the same cycles as two (MI355X_MICROARCH.md) and needs
    // {inv, inv} / {-o*inv, -o*inv} register pairs, which made the persistent variant 7 spill in this step (the
    // scalar form: variant 8 -1.7 %, variant 7 -18 %, profiles/r02aa)
    const float nx = -(o.x * inv.x), ny = -(o.y * inv.y), nz = -(o.z * inv.z);
    Wide4 w;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float ax = __builtin_fmaf((&nxr.x)[s], inv.x, nx), bx = __builtin_fmaf((&fxr.x)[s], inv.x, nx);
        const float ay = __builtin_fmaf((&nyr.x)[s], inv.y, ny), by = __builtin_fmaf((&fyr.x)[s], inv.y, ny);
        const float az = __builtin_fmaf((&nzr.x)[s], inv.z, nz), bz = __builtin_fmaf((&fzr.x)[s], inv.z, nz);
        const float t0 = fmaxf(fmaxf(ax, ay), fmaxf(az, 0.001f));
        const float t1 = fminf(fminf(bx, by), fminf(bz, tmax));
        w.tmin[s] = t0;
        w.hit[s] = t0 < t1;
    }
    return w;
}

// Spheres kept out of a 4-wide BVH (scenes with few spheres) are tested once per ray, before the traversal;
// the hit rule is order-independent, so this is the same closest hit.  A sphere is reached only if the
// reference's scene-level boxes on its path pass AABB::hit against [0.001, inf) with the exact 1/d: the
// reference never tests a sphere whose box the ray's interval misses, and f32 roots of large spheres can
// land outside the sphere's own box (a ray leaving the radius-999 ground sphere at t just above 0.001).
// Every ancestor box contains the sphere's leaf box and AABB::hit is monotone in the box (f32 subtraction
// and multiplication are monotone), so the leaf box alone decides: record word 7 = its index in chain.
__device__ __forceinline__ bool ref_scene_box(float4 A, float4 B, V3 o, V3 inv) {
    const float t0x = (A.x - o.x) * inv.x, t0y = (A.y - o.y) * inv.y, t0z = (A.z - o.z) * inv.z;
    const float t1x = (A.w - o.x) * inv.x, t1y = (B.x - o.y) * inv.y, t1z = (B.y - o.z) * inv.z;
    float tmin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
    float tmax = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
    tmin = fmaxf(tmin, 0.001f);
    tmax = fminf(tmax, __builtin_inff());
    return !(tmax <= tmin);
}
// Sphere::hit's candidate root from its discriminant terms (Sphere.cuh:27-47 with closest = inf).
__device__ __forceinline__ float sphere_root(float qa, float hb, float disc) {
    if (disc < 0) return -1.f;
    const float sq = sqrt_exact_wave(disc);
    float root = (-hb - sq) / qa;
    if (root < 0.001f) {
        root = (-hb + sq) / qa;
        if (root < 0.001f) return -1.f;
    }
    return root;
}

// The per-ray spheres of the 4-wide variants are tested after the trace, against the trace's closest hit (the hit
// rule is order-independent, so the result is the same as testing them first).  A sphere whose near root is
// provably beyond that hit then skips the correctly rounded sqrt and division: with su >= sqrtf(disc) (raw
// v_sqrt_f32 is within 1 ulp, so 4 ulp of margin), fl(-hb - su) <= fl(-hb - sqrtf(disc)) by monotone rounding, and
// fl(-hb - su) > fl(closest * qa) * (1 + 1e-5) puts the exact root above nextafter(closest).  The far root is
// larger still.  (Testing them at ray start instead measured +2.1 %, profiles/r01ag.)
__device__ __forceinline__ bool sphere_beyond(float qa, float hb, float disc, float closest) {
    if (!(disc > 1e-30f) || !(closest < __builtin_inff())) return false;
    const float su = __builtin_amdgcn_sqrtf(disc) * (1.0f + 0x1p-21f);
    const float lb = -hb - su;
    return lb > (closest * qa) * (1.0f + 1e-5f);
}

// Two spheres at once (data from the kernel arguments): the reference box tests and the discriminant
// arithmetic (IEEE, the reference's operation order: (x*x + y*y) + z*z), roots and divisions per sphere.  In scalar
// f32: the packed form (v_pk_*) takes the same SIMD cycles and its register pairs cost the hot loop two spilled
// VGPRs (-1.2 % without, profiles/r02ab).
template <bool LATE = false>
__device__ __forceinline__ void ray_spheres2(const float* sa, const float* sb, V3 o, V3 d, V3 inv,
                                             float& closest, int& hit) {
    const float* sp[2] = {sa, sb};
    bool reach[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float* q = sp[s];
        const float4 lo = *reinterpret_cast<const float4*>(q + 4), hi = *reinterpret_cast<const float4*>(q + 8);
        const float t0x = (lo.x - o.x) * inv.x, t1x = (lo.w - o.x) * inv.x;
        const float t0y = (lo.y - o.y) * inv.y, t1y = (hi.x - o.y) * inv.y;
        const float t0z = (lo.z - o.z) * inv.z, t1z = (hi.y - o.z) * inv.z;
        float tmin = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
        float tmax = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
        tmin = fmaxf(tmin, 0.001f);
        reach[s] = !(tmax <= tmin);
    }
    if (!(reach[0] || reach[1])) return;
    const float qa = dot(d, d);
    float t[2];
    // (a wave-uniform skip of a sphere no lane reaches measured +0.9 % on config C and -0.8 % on B, profiles/r05e)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float4 c = *reinterpret_cast<const float4*>(sp[s]);
        const float ocx = o.x - c.x, ocy = o.y - c.y, ocz = o.z - c.z;
        const float hb = (ocx * d.x + ocy * d.y) + ocz * d.z;
        const float qc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - c.w;
        const float disc = hb * hb - qa * qc;
        t[s] = reach[s] && !(LATE && sphere_beyond(qa, hb, disc, closest)) ? sphere_root(qa, hb, disc) : -1.f;
    }
    const int ra = __float_as_int(sa[10]), rb = __float_as_int(sb[10]);
    if (t[0] >= 0.f && better(t[0], ra, closest, hit)) { closest = t[0]; hit = ra; }
    if (t[1] >= 0.f && better(t[1], rb, closest, hit)) { closest = t[1]; hit = rb; }
}

// inv: AABB::hit's 1/d, bit-exact (recip_exact_any), shared with the traversal.
template <bool LATE = false>
__device__ __forceinline__ void ray_spheres(const float4* __restrict__ prims, const float4* __restrict__ chain,
                                            int n_chain, int first, int n, V3 o, V3 d, V3 inv, float& closest,
                                            int& hit, const float* sph2 = nullptr) {
    if (n == 0) return;
    if (n == 2 && sph2) {
        ray_spheres2<LATE>(sph2, sph2 + 16, o, d, inv, closest, hit);
        return;
    }
    for (int s = 0; s < n; ++s) {
        const int p = first + s;
        const float4 f0 = prims[3 * p], f1 = prims[3 * p + 1];
        const int k = __float_as_int(f1.w);
        if (!ref_scene_box(chain[2 * k], chain[2 * k + 1], o, inv)) continue;
        const float t = sphere_candidate(f0, f1, o, d, __builtin_inff());
        const int rank = __float_as_int(f1.z);
        if (t >= 0.f && better(t, rank, closest, hit)) {
            closest = t;
            hit = rank;
        }
    }
}

__device__ __forceinline__ void cas(uint32_t& a, uint32_t& b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// Per-lane closest hit over a 4-wide BVH (diagnostic path: crt_scene_compare).  Returns the rank or -1.
__device__ int trace4(const float4* __restrict__ nodes, const float4* __restrict__ prims,
                      const float4* __restrict__ chain, int n_chain, int sphere_first, int n_spheres, V3 o, V3 d,
                      float& closest) {
    const V3 inv = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    closest = __builtin_inff();
    int hit = -1, node = 0, sp = 0;
    ray_spheres(prims, chain, n_chain, sphere_first, n_spheres, o, d, inv, closest, hit);
    int stack[64];
    while (node >= 0) {
        const uint32_t b = node_base(node);
        const Wide4 w = wide_boxes(nodes, b, ray_rows(box_inv(inv)), o, box_inv(inv), closest);
        const float4 mf = node_row(nodes, b, 6);
        const int first_child = __float_as_int(mf.x), n_int = __float_as_int(mf.y) & 0xff;
        const uint32_t counts = __float_as_uint(mf.w);
        int off = 0;
        const float entry = closest;
        for (int s = 0; s < 4; ++s) {
            const int c = (counts >> (8 * s)) & 0xff;
            if (s >= n_int && c > 0 && w.hit[s]) {
                for (int k = 0; k < c; ++k) {
                    int rank;
                    const float t = prim_test(prims, __float_as_int(mf.z) + off + k, o, d, entry, rank);
                    if (t >= 0.f && better(t, rank, closest, hit)) { closest = t; hit = rank; }
                }
            }
            off += c;
        }
        uint32_t k[4];
        for (int s = 0; s < 4; ++s) k[s] = (s < n_int && w.hit[s]) ? ((__float_as_uint(w.tmin[s]) & ~3u) | s) : ~0u;
        cas(k[0], k[1]); cas(k[2], k[3]); cas(k[0], k[2]); cas(k[1], k[3]); cas(k[1], k[2]);
        if (k[0] != ~0u) {
            node = first_child + (int)(k[0] & 3);
            for (int s = 3; s >= 1; --s)
                if (k[s] != ~0u && sp < 64) stack[sp++] = first_child + (int)(k[s] & 3);
        } else {
            node = sp > 0 ? stack[--sp] : -1;
        }
    }
    return hit;
}

// One wave traversal step over a 4-wide BVH (variant 4).  Every lane with a node tests its four child
// boxes; hit internal children are ordered near-first (u32 sort of (tmin bits | slot) keys), the nearest
// becomes the lane's next node and the others go onto its stack as ONE entry (children are consecutive
// nodes): first_child << 8 | remaining << 6 | slot0 << 4 | slot1 << 2 | slot2, slots in pop order.  A pop
// takes slot0 and rewrites the entry while slots remain, so the stack holds at most one entry per
// branching ancestor.  The primitives of the hit leaf children (one consecutive range) join this step's
// cooperative leaf rounds.  All 64 lanes call it.
// Overflow stack entry `at` of pixel `pix`: a 32-bit byte offset from the uniform base (the host keeps the
// region below 4 GiB), so the address is SGPR base + VGPR offset and nothing 64-bit stays live per lane.
__device__ __forceinline__ uint32_t* ovf_slot(const RenderParams& P, int at, size_t pix, size_t n_pix) {
    const uint32_t byte = ((uint32_t)(at - P.stack_lds) * (uint32_t)n_pix + (uint32_t)pix) << 2;
    return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(P.ovf) + byte);
}

// The lane id recomputed at the point of use (two VALU ops, no register kept across the loop): at the 80-VGPR
// budget of 6 waves/SIMD the allocator otherwise spills the lane's stack address and reloads it from scratch on
// every push and pop.
__device__ __forceinline__ int lane_fresh() {
    int l;
    __asm__ volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// A stack test of the push or pop, expected true where `likely` (a compile-time constant): in the frozen render
// kernels the LDS entry is the fall-through path and the overflow and error branches sit out of line (C -0.65 %,
// profiles/frozen_launch).  Elsewhere the test stands as written, so every other kernel keeps its code.  (A macro: the
// hint of a __builtin_expect returned from an inlined helper is lowered before the helper is inlined, and lost.)
#define CRT_STACK_LIKELY(likely, c) ((likely) ? __builtin_expect((c), 1) : (c))

// LDSL: the push and pop expect the LDS entries (CRT_STACK_LIKELY)
template <bool COUNT, bool PF = false, bool LDSL = false>
__device__ __forceinline__ void node_step4(const RenderParams& P, V3 o, V3 inv, uint32_t rows, int& node, int& sp, float closest,
                                           TraceCounts& cnt, uint32_t* __restrict__ stk, int lane, size_t pix,
                                           size_t n_pix, int& leaf_first, int& leaf_n, float4* pf = nullptr,
                                           bool have_pf = false) {
    leaf_n = 0;
    leaf_first = 0;
#ifdef CRT_PROFILE_ROWS
    uint64_t row_wait = 0;
#endif
    if (node >= 0) {
        const uint32_t b = node_base(node);
#ifdef CRT_PROFILE_ROWS
        // profiling build: the seven rows issued, then waited for between two timers
        const uint32_t ex = b ^ (rows & 0xffu), ey = b ^ ((rows >> 8) & 0xffu), ez = b ^ (rows >> 16);
        const uint64_t ra = shader_clock();
        const float4 mf = node_row(P.nodes, b, 6);
        const float4 nxr = *rec_at(P.nodes, ex), fxr = *rec_at(P.nodes, ex ^ 16u);
        const float4 nyr = *rec_at(P.nodes, ey), fyr = *rec_at(P.nodes, ey ^ 16u);
        const float4 nzr = *rec_at(P.nodes, ez), fzr = *rec_at(P.nodes, ez ^ 16u);
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
        __asm__ volatile("" : : "v"(mf.x), "v"(nxr.x), "v"(fxr.x), "v"(nyr.x), "v"(fyr.x), "v"(nzr.x), "v"(fzr.x) : "memory");
        row_wait = shader_clock() - ra;
        const Wide4 w = wide_boxes_of(nxr, fxr, nyr, fyr, nzr, fzr, o, inv, closest);
#else
        // PF: the rows are in pf when the previous step's first leaf round loaded them for this node (have_pf), else
        // they load here as without the prefetch
        if (PF && !have_pf) load_node_rows(P.nodes, b, rows, pf);
        const float4 mf = PF ? pf[6] : node_row(P.nodes, b, 6);
        const Wide4 w = PF ? wide_boxes_of(pf[0], pf[1], pf[2], pf[3], pf[4], pf[5], o, inv, closest)
                           : wide_boxes(P.nodes, b, rows, o, inv, closest);
#endif
        // keep the whole link row in the node's loads: left to itself the compiler loads leaf_first / counts
        // only inside the leaf branch, one more dependent load on a leaf step's critical path.  Pinned after the
        // box tests, so the wait it implies is the one the boxes need anyway (pinned before them, it made the six
        // box loads wait for the link row's round trip)
        __asm__ volatile("" : : "v"(mf.z), "v"(mf.w));
        const int first_child = __float_as_int(mf.x);
        const int meta = __float_as_int(mf.y);
        const uint32_t counts = __float_as_uint(mf.w);
        const int n_int = meta & 0xff;
        if (COUNT) cnt.boxes += (uint32_t)(meta >> 8);
        // leaf children: consecutive primitives; test the span from the first to the last hit leaf.  Slots
        // [n_int, n_slots) are leaves (count >= 1), empty slots are never hit, so the hit leaves are the hit bits
        // above n_int; counts * 0x01010101 holds the running ends in its bytes (at most 255 primitives per node,
        // checked by the builder).
        uint32_t hm = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) hm |= w.hit[s] ? (1u << s) : 0u;
        const uint32_t lm = hm & (0xfu << n_int);
        if (lm) {
            // counts * 0x01010101 (byte-wise running sums) as shift-adds: a 32-bit multiply is quarter rate (the empty
            // asm keeps the compiler from folding the shifts back into one)
            uint32_t c2 = counts + (counts << 8);
            __asm__("" : "+v"(c2));
            uint32_t ends = c2 + (c2 << 16);
            __asm__("" : "+v"(ends));
            const uint32_t first = (uint32_t)__builtin_ctz(lm), last = 31u - (uint32_t)__builtin_clz(lm);
            const int lo = (int)(((ends << 8) >> (8u * first)) & 0xffu);
            const int hi = (int)((ends >> (8u * last)) & 0xffu);
            leaf_n = hi - lo;
            leaf_first = __float_as_int(mf.z) + lo;
#ifdef CRT_CHECKED
            // the span must lie inside the primitive array.  emit4 guarantees it for every node it writes (checked there
            // on the host, once per node), so the fast build trusts the tree; the checked build re-checks it here once per
            // lane and step (before round 5 the fast build did too: one kernel-argument reload and wait per leaf step)
            if ((unsigned)leaf_first > (unsigned)P.n_prims || (unsigned)leaf_n > (unsigned)(P.n_prims - leaf_first)) {
                atomicOr(P.err, 1u);
                leaf_n = 0;
            }
#endif
        }
        uint32_t k[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) k[s] = (s < n_int && w.hit[s]) ? ((__float_as_uint(w.tmin[s]) & ~3u) | s) : ~0u;
        cas(k[0], k[1]); cas(k[2], k[3]); cas(k[0], k[2]); cas(k[1], k[3]); cas(k[1], k[2]);
        // sp counts stored entries only: an entry beyond the host's bound is dropped (and reported through P.err, the
        // frame is wrong) without advancing sp, so a pop never reads an entry that was not stored (reading one made
        // the traversal restart at the root, forever)
        auto store = [&](int at, uint32_t v) -> bool {
            if (CRT_STACK_LIKELY(LDSL, at < P.stack_lds)) stk[at * 64 + lane_fresh()] = v;
            else if (CRT_STACK_LIKELY(LDSL, at < P.stack_cap)) *ovf_slot(P, at, pix, n_pix) = v;
            else { atomicOr(P.err, 2u); return false; }
            return true;
        };
        if (k[0] != ~0u) {
            node = first_child + (int)(k[0] & 3);
            // the hit internal children but the nearest (k[s] != ~0u exactly for the hit slots below n_int), as one
            // popcount (-1.0 %, profiles/r02ap)
            const uint32_t n_rest = (uint32_t)__popc(hm & ((1u << n_int) - 1u)) - 1u;
            if (n_rest && store(sp, ((uint32_t)first_child << 8) | (n_rest << 6) | ((k[1] & 3) << 4) |
                                        ((k[2] & 3) << 2) | (k[3] & 3)))
                ++sp;
        } else if (sp > 0) {
            const int at = sp - 1;
            const uint32_t top = CRT_STACK_LIKELY(LDSL, at < P.stack_lds) ? stk[at * 64 + lane_fresh()]
                                                  : (at < P.stack_cap ? *ovf_slot(P, at, pix, n_pix) : 0u);
            const uint32_t rest = (top >> 6) & 3;
            node = (int)(top >> 8) + (int)((top >> 4) & 3);
            if (rest <= 1) sp = at;
            else store(at, (top & ~0xffu) | ((rest - 1) << 6) | ((top & 0xfu) << 2));
        } else {
            node = -1;
        }
    }
#ifdef CRT_PROFILE_ROWS
    {   // the wait of a lane that stepped (uniform among them: the timers are scalar)
        const uint64_t st = wave_ballot(row_wait != 0);
        if (st) cnt.cyc_rows += bcast64(row_wait, __builtin_ctzll(st));
    }
#endif
}

template <bool COUNT, bool PF = false, bool LDSL = false>
__device__ __forceinline__ void traverse_step4(const RenderParams& P, V3 o, V3 d, V3 inv, uint32_t rows, int& node, int& sp,
                                               float& closest, int& hit, TraceCounts& cnt, WaveLdsWide& L,
                                               uint32_t* __restrict__ stk, int lane, size_t pix, size_t n_pix,
                                               float4* pf = nullptr, int* pf_node = nullptr) {
    constexpr bool TIME = COUNT || kProfilePass;
    if (COUNT || kProfilePass) cnt.step_slots++;
    const uint64_t c0 = TIME ? shader_clock() : 0;
    int leaf_n, leaf_first;
    if constexpr (PF) {
        // pf holds node *pf_node's rows when the previous step's first leaf round loaded them (profiles/r06r)
        node_step4<COUNT, true, LDSL>(P, o, inv, rows, node, sp, closest, cnt, stk, lane, pix, n_pix, leaf_first, leaf_n, pf,
                                *pf_node == node);
        *pf_node = -1;
    } else
    node_step4<COUNT, false, LDSL>(P, o, inv, rows, node, sp, closest, cnt, stk, lane, pix, n_pix, leaf_first, leaf_n);
    const uint64_t c1 = TIME ? shader_clock() : 0;
    if (TIME) cnt.cyc_step += c1 - c0;
#ifdef CRT_PROFILE_PAIRS
    // profiling build (tools/pair_histogram.py): per wave step, the lanes stepping and the leaf pairs, log2 buckets
    {
        const uint32_t n_step = (uint32_t)__popcll(wave_ballot(node >= 0 || leaf_n > 0));
        const int tot = __builtin_amdgcn_readlane(wave_inclusive_scan(leaf_n, lane), 63);
        if (lane_fresh() == 0) {
            atomicAdd(&g_pair_hist[tot == 0 ? 0 : 1 + min(31 - __clz(tot), 14)], 1ull);
            atomicAdd(&g_pair_hist[16 + min(n_step >> 3, 8u)], 1ull);
        }
    }
#endif
    if (!wave_ballot(leaf_n > 0)) return;
    const int incl = wave_inclusive_scan_dpp(leaf_n);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    const int pfx = incl - leaf_n;
    {   // every lane writes its own slots, only the owners' are read: no branch (-0.8 %, profiles/r02ar)
        // leaf_first - prefix: a pair's primitive is ray1.w + its index j (-0.27 %, profiles/r02aq; round 1 measured
        // this +2.2 %, profiles/r01aj, before the round-2 changes to the round's code)
        L.ray1[lane] = make_float4(d.y, d.z, closest, __int_as_float(leaf_first - pfx));
#ifdef CRT_CHECKED
        L.prefix[lane] = pfx;
        L.span_n[lane] = leaf_n;
#endif
        // the empty key, materialised here: as a plain constant the register allocator keeps ~0ull live across
        // the loop and spills it (a scratch reload and a vmcnt(0) wait on every leaf step)
        uint32_t ones;
        __asm__ volatile("v_mov_b32 %0, -1" : "=v"(ones));
        L.key[lane] = ((unsigned long long)ones << 32) | ones;
    }
    uint32_t carry = 0;   // owner + 1 of the last pair of the previous round
    if constexpr (PF) {
        // The row prefetch (variant 8 at occupancy 4, profiles/r06r): the lane's next node is known before the leaf
        // rounds, and their hits only lower `closest`, which the rows do not depend on.  The first round loads every
        // lane's pair record (slots past the end: record 0), THEN the lane's next node's seven rows (node 0 for a lane
        // without one): vector-memory loads retire in order, so the round waits for its records only (rows loaded
        // before the records made the round wait for them too: +3.6 %, profiles/r06o).  The next node step finds the
        // rows in registers (28 VGPRs, which is why this needs occupancy 4's budget).
        auto round = [&](int base, auto first) {
            if (COUNT || kProfilePass) cnt.round_slots++;
            if (leaf_n > 0 && pfx >= base && pfx < base + 64) L.owner_at[pfx - base] = (unsigned char)(lane + 1);
            wave_sync();
            const uint32_t mark = L.owner_at[lane];
            L.owner_at[lane] = 0;
            const uint32_t owner1 = max(wave_inclusive_max_scan_u(mark), carry);
            const int owner = (int)owner1 - 1;   // >= 0 on every lane: slot 0 of round 0 carries a mark
            const int j = base + lane;
            const float4 r0 = L.ray0[owner], r1 = L.ray1[owner];
#ifdef CRT_CHECKED
            // checked build: the fast path's per-pair bounds re-checked, as in the rounds below
            const bool bad = j < total && ((unsigned)owner >= 64u || j < L.prefix[owner] ||
                                           j >= L.prefix[owner] + L.span_n[owner] ||
                                           (unsigned)(__float_as_int(r1.w) + j) >= (unsigned)P.n_prims);
            if (bad) atomicOr(P.err, 4u);
            const bool act = j < total && !bad;
#else
            const bool act = j < total;
#endif
            const int pp = act ? __float_as_int(r1.w) + j : 0;
            const float4* rr = rec_at(P.prims, __umul24((uint32_t)pp, 48u));
            const float4 f0 = rr[0], f1 = rr[1], f2 = rr[2];
            if constexpr (decltype(first)::value) {
                __asm__ volatile("" : : : "memory");   // the rows after the records
                load_node_rows(P.nodes, node_base(node >= 0 ? node : 0), rows, pf);
            }
            if (act) {
                if (COUNT) cnt.tris++;
                __asm__ volatile("" : : "v"(f2.y));   // the third row as one dwordx4 (prim_test)
                const V3 ro = v3(r0.x, r0.y, r0.z), rd = v3(r0.w, r1.x, r1.y);
                const int rank = __float_as_int(f2.z);
                const float t = (P.tree_spheres != 0 && __float_as_int(f2.w) == 1) ? sphere_candidate(f0, f1, ro, rd, r1.z)
                                                                                  : tri_test_flat(f0, f1, f2, ro, rd, r1.z);
                const unsigned long long kp = ((unsigned long long)__float_as_uint(t) << 32) | (0xffffffffu - (unsigned)rank);
                atomicMin(&L.key[owner], t >= 0.f ? kp : ~0ull);
            }
            carry = __builtin_amdgcn_readlane(owner1, 63);
            wave_sync();
        };
        round(0, std::true_type{});
        *pf_node = node;
        for (int base = 64; base < total; base += 64) round(base, std::false_type{});
    } else
    for (int base = 0; base < total; base += 64) {
        if (COUNT || kProfilePass) cnt.round_slots++;
        if (leaf_n > 0 && pfx >= base && pfx < base + 64) L.owner_at[pfx - base] = (unsigned char)(lane + 1);
        wave_sync();
        const uint32_t mark = L.owner_at[lane];
        L.owner_at[lane] = 0;
        const uint32_t owner1 = max(wave_inclusive_max_scan_u(mark), carry);
        const int owner = (int)owner1 - 1;
        const int j = base + lane;
#ifdef CRT_PROFILE_ROWS
        uint64_t prim_wait = 0;
#endif
        if (j < total) {
            const float4 r0 = L.ray0[owner], r1 = L.ray1[owner];
            const int p = __float_as_int(r1.w) + j;   // leaf_first - prefix + j: inside the owner's checked span
            if (COUNT) cnt.tris++;
            int rank;
#ifdef CRT_PROFILE_ROWS
            {   // profiling build: the pair's record loaded and waited for between two timers (prim_test reloads it
                // from the vector L1)
                const float4* rr = rec_at(P.prims, __umul24((uint32_t)p, 48u));
                const uint64_t pa = shader_clock();
                const float4 g0 = rr[0], g1 = rr[1], g2 = rr[2];
                __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
                __asm__ volatile("" : : "v"(g0.x), "v"(g1.x), "v"(g2.x) : "memory");
                prim_wait = shader_clock() - pa;
            }
#endif
#ifdef CRT_CHECKED
            // checked build (-DCRT_CHECKED, lib/checked/): the per-pair bounds the fast path proves once per lane and
            // step (node_step4), re-checked here with the owner lookup itself, so a stale LDS owner mark or a wrong
            // prefix reports through P.err instead of loading outside the primitive array
            const bool bad = (unsigned)owner >= 64u || j < L.prefix[owner] || j >= L.prefix[owner] + L.span_n[owner] ||
                             (unsigned)p >= (unsigned)P.n_prims;
            if (bad) atomicOr(P.err, 4u);
            rank = -1;
            const float t = bad ? -1.f : prim_test(P.prims, p, v3(r0.x, r0.y, r0.z), v3(r0.w, r1.x, r1.y), r1.z, rank,
                                                   P.tree_spheres != 0);
#else
            const float t = prim_test(P.prims, p, v3(r0.x, r0.y, r0.z), v3(r0.w, r1.x, r1.y), r1.z, rank,
                                      P.tree_spheres != 0);
#endif
            // a rejected pair offers the empty key (no effect on the min): one LDS atomic per pair, no branch
            // (-0.75 %, profiles/r02ar)
            const unsigned long long kp = ((unsigned long long)__float_as_uint(t) << 32) | (0xffffffffu - (unsigned)rank);
            atomicMin(&L.key[owner], t >= 0.f ? kp : ~0ull);
        }
#ifdef CRT_PROFILE_ROWS
        cnt.cyc_prims += bcast64(prim_wait, 0);   // lane 0's slot base + 0 < total is always tested
#endif
        carry = __builtin_amdgcn_readlane(owner1, 63);
        wave_sync();
    }
    {
        const unsigned long long kk = L.key[lane];
        const float t = __uint_as_float((unsigned)(kk >> 32));
        const int rank = (int)(0xffffffffu - (unsigned)kk);
        if (leaf_n > 0 && kk != ~0ull && better(t, rank, closest, hit)) {
            closest = t;
            hit = rank;
        }
    }
    if (TIME) cnt.cyc_round += shader_clock() - c1;
}

// The tree's top nodes held in LDS (CRT_TOP_LEVELS): the root and, at level 2, its internal children, copied once
// per workgroup with their rows unswizzled (row k at 16-B slot k).  Every ray starts at the root, and its first node
// steps are the same for every ray up to the direction signs, so a new ray takes them in the regeneration pass from
// LDS instead of in traversal steps that wait for L1/L2: the same box tests with the same operands (closest = inf,
// no leaf was tested yet), the same near-first order and stack entries, hence the same traversal bit for bit.
#ifndef CRT_TOP_LEVELS
#define CRT_TOP_LEVELS 1
#endif
constexpr int TOP_NODES = CRT_TOP_LEVELS >= 2 ? 5 : CRT_TOP_LEVELS >= 1 ? 1 : 0;

// One node step of node_step4 on an LDS record, for a lane whose ray has tested no leaf yet (closest = inf).  Returns
// false, changing nothing, when a leaf child is hit: the lane then takes this node through the regular step, whose
// leaf rounds test it.
template <bool COUNT, bool LDSL = false>
__device__ __forceinline__ bool top_step4(const RenderParams& P, const float4* rec, V3 o, V3 inv, uint32_t rows,
                                          int& node, int& sp, TraceCounts& cnt, uint32_t* __restrict__ stk,
                                          size_t pix, size_t n_pix) {
    const Wide4 w = wide_boxes(rec, 0u, rows, o, inv, __builtin_inff());
    const float4 mf = rec[6];
    const int first_child = __float_as_int(mf.x);
    const int meta = __float_as_int(mf.y);
    const int n_int = meta & 0xff;
    uint32_t hm = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) hm |= w.hit[s] ? (1u << s) : 0u;
    if (hm & (0xfu << n_int)) return false;
    if (COUNT) cnt.boxes += (uint32_t)(meta >> 8);
    uint32_t k[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) k[s] = (s < n_int && w.hit[s]) ? ((__float_as_uint(w.tmin[s]) & ~3u) | s) : ~0u;
    cas(k[0], k[1]); cas(k[2], k[3]); cas(k[0], k[2]); cas(k[1], k[3]); cas(k[1], k[2]);
    auto store = [&](int at, uint32_t v) -> bool {
        if (CRT_STACK_LIKELY(LDSL, at < P.stack_lds)) stk[at * 64 + lane_fresh()] = v;
        else if (CRT_STACK_LIKELY(LDSL, at < P.stack_cap)) *ovf_slot(P, at, pix, n_pix) = v;
        else { atomicOr(P.err, 2u); return false; }
        return true;
    };
    if (k[0] != ~0u) {
        node = first_child + (int)(k[0] & 3);
        const uint32_t n_rest = (uint32_t)__popc(hm & ((1u << n_int) - 1u)) - 1u;
        if (n_rest && store(sp, ((uint32_t)first_child << 8) | (n_rest << 6) | ((k[1] & 3) << 4) |
                                    ((k[2] & 3) << 2) | (k[3] & 3)))
            ++sp;
    } else if (sp > 0) {
        const int at = sp - 1;
        const uint32_t top = CRT_STACK_LIKELY(LDSL, at < P.stack_lds) ? stk[at * 64 + lane_fresh()]
                                              : (at < P.stack_cap ? *ovf_slot(P, at, pix, n_pix) : 0u);
        const uint32_t rest = (top >> 6) & 3;
        node = (int)(top >> 8) + (int)((top >> 4) & 3);
        if (rest <= 1) sp = at;
        else store(at, (top & ~0xffu) | ((rest - 1) << 6) | ((top & 0xfu) << 2));
    } else {
        node = -1;
    }
    return true;
}

// A new ray's first node steps from the LDS top nodes: the root, then (TOPN = 5) the internal child it continues to.
template <bool COUNT, int TOPN, bool LDSL = false>
__device__ __forceinline__ void top_steps(const RenderParams& P, const float4* top, V3 o, V3 inv, uint32_t rows,
                                          int& node, int& sp, TraceCounts& cnt, uint32_t* __restrict__ stk, size_t pix,
                                          size_t n_pix) {
    if (P.top_levels <= 0) return;   // uniform
    if (!top_step4<COUNT, LDSL>(P, top, o, inv, rows, node, sp, cnt, stk, pix, n_pix) || TOPN < 5 || P.top_levels < 2 ||
        node < 0)
        return;
    const int m = node - __float_as_int(top[6].x);   // node is an internal child of the root: slot m < 4
    if ((unsigned)m < 4u) top_step4<COUNT, LDSL>(P, top + 8 * (1 + m), o, inv, rows, node, sp, cnt, stk, pix, n_pix);
}

// Per-lane path state of one pixel (rayColor's locals, CUDAKernels.h:102-145, plus the sample loop).
struct PathState {
    Rng s;
    V3 pixel, o, d, thr;
    int remaining, bounce;
    bool need_new;
    uint32_t rays, paths;
#ifdef CRT_PROFILE_LOOPS
    uint32_t k1, k2, kr;   // this pass: unit-sphere candidates, unit-disk candidates, Russian-roulette draws
#endif
#ifdef CRT_PROFILE_SITES
    uint32_t site;         // this pass: SITE_* bits of the blocks the lane took
#endif
};
#ifdef CRT_PROFILE_SITES
// Profiling build only (tools/build_profile_lib.sh sites -DCRT_PROFILE_SITES, tools/pass_site_count.py): which lanes
// of a regeneration pass take the blocks that used to be issued once per lane set.  A lane marks the blocks it takes;
// variant 8 ballots the marks per pass.  CAM_ENTRY: came into next_ray without a path and starts a sample; CAM_KILLED:
// ended by the bounce limit or roulette inside next_ray and starts a sample (with the camera block ahead of those
// tests this was a second trip of next_ray's loop and a second camera block).  UNIT_*: the lane needs a vector
// normalised: the unit-sphere point (Lambert and metal), the direction for glass, the direction for the sky; REFL is
// metal's second normalisation, which stays in its branch.
constexpr uint32_t SITE_CAM_ENTRY = 1, SITE_CAM_KILLED = 2, SITE_UNIT_RUV = 4, SITE_UNIT_GLASS = 8, SITE_UNIT_SKY = 16,
                   SITE_UNIT_REFL = 32;
// Summed over variant 8's passes: [0] passes, [1] passes with a CAM_ENTRY lane, [2] with a CAM_KILLED lane, [3] with
// both (a camera block saved), [4]-[7] passes with a RUV / GLASS / SKY / REFL lane, [8] passes with any of RUV, GLASS,
// SKY (the shared unit() runs), [9] the number of those three present, summed (the unit() sites issued one per
// material), [10] parked lanes, [11] lanes that take the camera block
__device__ unsigned long long g_site_prof[12];
#endif
#ifdef CRT_PROFILE_LOOPS
// Profiling build only (tools/build_profile_lib.sh loops -DCRT_PROFILE_LOOPS, tools/loop_fusion_count.py): the
// regeneration pass's two rejection loops, counted from the XORWOW draw counter (d advances by 362437 per draw;
// 945708813 is its inverse mod 2^32).  Summed over variant 8's passes: [0] passes, [1] sum of the wave's max unit-sphere
// candidates, [2] max unit-disk candidates, [3] max over lanes of (sphere + disk candidates), the iteration count of
// one fused loop, [4] max over lanes of (sphere + RR + disk) draws-steps, [5] lane sum of sphere candidates, [6] lane
// sum of disk candidates, [7] parked lanes
__device__ unsigned long long g_loop_prof[8];
__device__ __forceinline__ uint32_t draws_since(uint32_t d0, uint32_t d1) { return (d1 - d0) * 945708813u; }
#endif

struct CamRegs {
    V3 pos, llc, hor, ver, right, up;
    float lens, fw, fh;
    float rfw, rfh;   // RN(1 / fw), RN(1 / fh) (host IEEE division)
    int fast_uv;      // uv_div is verified exact for this frame size (crt_renderer_create): no IEEE division
};
__device__ __forceinline__ CamRegs cam_regs(const crt_camera_desc& Cd, int width, int height, float rcp_w, float rcp_h,
                                            int fast_uv) {
    CamRegs C;
    C.pos = v3(Cd.origin[0], Cd.origin[1], Cd.origin[2]);
    C.llc = v3(Cd.lower_left[0], Cd.lower_left[1], Cd.lower_left[2]);
    C.hor = v3(Cd.horizontal[0], Cd.horizontal[1], Cd.horizontal[2]);
    C.ver = v3(Cd.vertical[0], Cd.vertical[1], Cd.vertical[2]);
    C.right = v3(Cd.right[0], Cd.right[1], Cd.right[2]);
    C.up = v3(Cd.up[0], Cd.up[1], Cd.up[2]);
    C.lens = Cd.lens_radius;
    C.fw = (float)width;
    C.fh = (float)height;
    C.rfw = rcp_w;
    C.rfh = rcp_h;
    C.fast_uv = fast_uv;
    return C;
}

// Phase 1: give the lane a ray to trace — Camera::getRay for a new sample, the bounce-limit exit and
// Russian roulette (CUDAKernels.h:110-121).  Returns false when the pixel has no samples left.
//
// A wave instruction costs its issue slot whatever the number of lanes that run it, so the camera block is written to
// be issued once per call: the lanes that still have a path take the bounce-limit test and the roulette draw FIRST,
// and the lanes those end join the lanes that came in without a path for one Camera::getRay.  (With the camera block
// first, a wave holding both kinds of lane ran it twice, for disjoint lanes.)  Each lane's own sequence of draws is
// the reference's: roulette, then the disk candidates, then the two pixel uniforms.  A new sample has bounce 0 and
// leaves at once; only max_bounces <= 0 ends it on the spot, and the loop round the camera block is for that case alone.
__device__ __forceinline__ bool next_ray(PathState& S, const CamRegs& C, int x, int y, int max_bounces) {
#ifdef CRT_PROFILE_SITES
    if (S.need_new && S.remaining != 0) S.site |= SITE_CAM_ENTRY;
#endif
    if (!S.need_new) {
        if (S.bounce >= max_bounces) {                      // loop exhausted: final_color = 0
            S.pixel = S.pixel + v3(0.0f, 0.0f, 0.0f);
            ++S.paths;
            S.need_new = true;
        } else if (S.bounce >= 3) {
            float p = fmaxf(S.thr.x, fmaxf(S.thr.y, S.thr.z));
            p = fminf(p, 0.95f);
#ifdef CRT_PROFILE_LOOPS
            S.kr += 1u;
#endif
            if (uniform(S.s) > p) {
                S.pixel = S.pixel + v3(0.0f, 0.0f, 0.0f);
                ++S.paths;
                S.need_new = true;
            } else {
                S.thr = recip_exact_wave(p) * S.thr;   // 1 / p, exact (crt_device.h)
            }
        }
        if (!S.need_new) return true;
#ifdef CRT_PROFILE_SITES
        if (S.remaining != 0) S.site |= SITE_CAM_KILLED;
#endif
    }
    for (;;) {
        if (S.remaining == 0) return false;
        --S.remaining;
        float da, db;                                    // Utility::randomPointInUnitDisk
#ifdef CRT_PROFILE_LOOPS
        const uint32_t pd0 = S.s.d;
#endif
        for (;;) {
            da = rand_pm1(S.s);
            db = rand_pm1(S.s);
            if (len2(v3(da, db, 0)) >= 1) continue;
            break;
        }
#ifdef CRT_PROFILE_LOOPS
        S.k2 += draws_since(pd0, S.s.d) / 2u;
#endif
        const V3 rd = C.lens * v3(da, db, 0);
        const V3 off = v3(C.right.x * rd.x, C.right.y * rd.x, C.right.z * rd.x) +
                       v3(C.up.x * rd.y, C.up.y * rd.y, C.up.z * rd.y);
        const float au = (float)x + uniform(S.s);
        const float av = (float)y + uniform(S.s);
        float u, v;
        if (C.fast_uv) {
            u = uv_div(au, C.fw, C.rfw);
            v = uv_div(av, C.fh, C.rfh);
        } else {
            __asm__ volatile("");   // a real branch: no if-conversion that would run both divisions
            u = au / C.fw;
            v = av / C.fh;
        }
        S.o = C.pos + off;
        S.d = (((C.llc + u * C.hor) + v * C.ver) - C.pos) - off;
        S.thr = v3(1.0f, 1.0f, 1.0f);
        S.bounce = 0;
        S.need_new = false;
        if (max_bounces > 0) return true;                   // uniform
        S.pixel = S.pixel + v3(0.0f, 0.0f, 0.0f);           // max_bounces <= 0: the sample ends at the bounce limit
        ++S.paths;
        S.need_new = true;
    }
}

// The state of a lane that starts one new camera sample on the RNG state `s` and has no path: next_ray(S, C, x, y, 1)
// on it runs the camera block alone and leaves the ray in S.o, S.d and the advanced state in S.s.  For the callers
// that keep no PathState of their own (the path kernels of crt_paths.h, the geometry self-test).
__device__ __forceinline__ PathState new_sample_state(Rng s) {
    PathState S{};
    S.s = s;
    S.pixel = v3(0.f, 0.f, 0.f);
    S.thr = v3(1.f, 1.f, 1.f);
    S.remaining = 1; S.bounce = 0; S.need_new = true; S.rays = 0; S.paths = 0;
    return S;
}

// Dielectric::scatter's total-internal-reflection test in double, as the reference computes it (Material.cuh:115-118):
//   cannot = RN(ri * RN(sqrt(y))) > 1,   y = RN(1 - c * c)   (c * c is exact in double: two 24-bit factors).
// sqrt and the product are correctly rounded and monotone, so ri^2 * y decides the outcome unless it is within a hair
// of 1.  z = RN(RN(ri * ri) * y) is within a relative 2^-52 of ri^2 * y.  If z > 1 + 2^-40, then ri * sqrt(y) >
// 1 + 2^-43, and the two roundings (a relative 2^-53 each) keep RN(ri * RN(sqrt(y))) above 1 + 2^-53, so it rounds
// above 1.  If z < 1 - 2^-40, the product stays below 1.  Only a wave with a lane in between (or a NaN) runs the
// reference's f64 sqrt; the f64 sqrt sequence is otherwise the most expensive part of the glass shading.
__device__ __forceinline__ bool cannot_refract_exact(float cos_theta, float ri) {
    const double c = cos_theta, r = ri;
    const double y = __builtin_fma(-c, c, 1.0);          // == RN(1.0 - c * c): the product is exact
    const double z = (r * r) * y;
    const bool above = z > 1.0 + 0x1p-40, below = z < 1.0 - 0x1p-40;
    if (__builtin_amdgcn_ballot_w64(!(above || below)) == 0) return above;
    // keeps the f64 sqrt behind the branch: without it the compiler if-converts the uniform branch and computes the
    // sqrt sequence in every wave with a glass hit, then selects
    __asm__ volatile("");
    return r * sqrt(y) > 1.0;
}

// Phase 3: material scatter / emit / sky (CUDAKernels.h:123-142, Material.cuh:66-146).  The hit's normal and
// material come from its shading record (crt_device.h): one pair of independent loads per hit.
// shade_rec: the same with the hit's shading record rows 0-1 already loaded (r0, m); a sphere's row 2 (1 / radius) is
// inv_r when `staged`, else loaded here.  crt_paths.h's scatter_step() is its twin on a crt_hit record, kept apart: one
// shared core changes the assembly of 51 of the 58 kernels (profiles/shared_scatter/kernels_unchanged.txt).
__device__ __forceinline__ void shade_rec(PathState& S, const RenderParams& P, int hit_rank, float t, float4 r0,
                                          float4 m, bool staged, float inv_r);
__device__ __forceinline__ void shade(PathState& S, const RenderParams& P, int hit_rank, float t) {
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), m = r0;
    if (hit_rank >= 0) {
        const float4* R = P.shade + 3u * (uint32_t)hit_rank;   // 32-bit index (ranks < 2^30): no 64-bit multiply
        r0 = R[0];
        m = R[1];
    }
    shade_rec(S, P, hit_rank, t, r0, m, false, 0.f);
}
__device__ __forceinline__ void shade_rec(PathState& S, const RenderParams& P, int hit_rank, float t, float4 r0,
                                          float4 m, bool staged, float inv_r) {
    // A miss has no record (r0 = m = 0); SHADE_MISS keeps it out of every material's branch below
    constexpr uint32_t SHADE_MISS = 15;
    const bool miss = hit_rank < 0;
    const uint32_t kind = __float_as_uint(r0.w);
    const V3 hp = S.o + t * S.d;                         // Ray::pointAtDistance
    V3 outward = v3(r0.x, r0.y, r0.z);                   // triangle: unit(cross(e1, e2)), Mesh.cuh:303-304
    if (!miss && (kind & SHADE_SPHERE)) {                // Sphere.cuh:44: (1 / radius) * (p - center)
        const float ir = staged ? inv_r : P.shade[3u * (uint32_t)hit_rank + 2u].x;
        outward = ir * (hp - outward);
    }
    const bool front = dot(S.d, outward) < 0;            // HitInfo::setFaceNormal
    const V3 n = front ? outward : -outward;
    const uint32_t code = miss ? SHADE_MISS : kind & 15u;
    // One normalisation for the whole pass.  Four places of the reference normalise a vector first: randomUnitVector
    // (Lambertian and Metal, their only draws: one rejection loop for both), Dielectric::scatter and the sky the ray's
    // direction.  Issued once per material they cost the wave one unit() each, for disjoint lanes; here every lane
    // picks its vector, one unit() runs over the union of those lanes, and the materials go on from its result.  The
    // square root and the reciprocal choose their fast or their IEEE sequence by a ballot over the lanes that run
    // them; both sequences are correctly rounded, so the wider lane set changes no bit.
    V3 q = S.d;                                          // dielectric, sky (CRTUtility.cuh:35)
#ifdef CRT_PROFILE_LOOPS
    const uint32_t pd0 = S.s.d;
#endif
    if (code == SHADE_LAMBERT || code == SHADE_METAL) q = rand_in_unit_sphere(S.s);
#ifdef CRT_PROFILE_LOOPS
    S.k1 += draws_since(pd0, S.s.d) / 3u;
#endif
#ifdef CRT_PROFILE_SITES
    S.site |= code <= SHADE_METAL ? SITE_UNIT_RUV : code == SHADE_DIELECTRIC ? SITE_UNIT_GLASS : miss ? SITE_UNIT_SKY : 0u;
    if (code == SHADE_METAL) S.site |= SITE_UNIT_REFL;
#endif
    V3 uq = q;
    if (code <= SHADE_DIELECTRIC || miss) uq = unit(q);  // Lambert, metal, dielectric, sky
    if (miss) {                                          // :137-142
        S.pixel = S.pixel + S.thr * sky_unit(uq);
        ++S.paths;
        S.need_new = true;
    } else if (code == SHADE_INVALID) {                  // :127 invalid material: same ray again
        ++S.bounce;
    } else if (code == SHADE_LAMBERT) {                  // Material.cuh:66-77
        V3 sd = n + uq;
        if (fabsf(sd.x) < 1e-8f && fabsf(sd.y) < 1e-8f && fabsf(sd.z) < 1e-8f) sd = n;
        S.thr = S.thr * v3(m.x, m.y, m.z);
        S.o = hp;
        S.d = sd;
        ++S.bounce;
    } else if (code == SHADE_METAL) {                    // :89-96
        V3 refl = reflect(S.d, n);
        refl = unit(refl) + (m.w * uq);
        if (dot(refl, n) > 0) {
            S.thr = S.thr * v3(m.x, m.y, m.z);
            S.o = hp;
            S.d = refl;
            ++S.bounce;
        } else {                                         // absorbed: return Material::emit() = 0
            S.pixel = S.pixel + v3(0.0f, 0.0f, 0.0f);
            ++S.paths;
            S.need_new = true;
        }
    } else if (code == SHADE_DIELECTRIC) {               // :109-128
        const float ri = front ? m.y : m.x;              // 1.0f / ior (front face) or ior, from the shading record
        const float r0 = front ? m.z : m.w;              // Schlick's r0 for that ri
        const V3 ud = uq;                                // unit(S.d)
        const float cos_theta = fminf(dot(-ud, n), 1.0f);
        const bool cannot_refract = cannot_refract_exact(cos_theta, ri);
        V3 dir;
        if (cannot_refract || schlick_r0(cos_theta, r0) > uniform(S.s))
            dir = reflect(ud, n);
        else
            dir = refract(ud, n, ri);
        S.o = hp;
        S.d = dir;
        ++S.bounce;   // attenuation (1,1,1): thr unchanged (x*1 == x)
    } else {                                             // DiffuseLight: return emit() raw
        const V3 em = code == SHADE_LIGHT ? v3(m.x, m.y, m.z) : v3(0.0f, 0.0f, 0.0f);
        S.pixel = S.pixel + em;
        ++S.paths;
        S.need_new = true;
    }
}

// A parked lane's end of trace in the regeneration pass (4-wide variants): the per-ray spheres (Sphere::hit behind the
// reference's sphere box, ray_spheres) and then shade.  The trace's own hit record is loaded before the sphere test,
// behind a compiler barrier, so its latency hides behind that test (-0.6 %, profiles/r03aa); when a per-ray sphere
// wins, its record comes from the LDS copy of the two per-ray spheres' records (or from HBM for other sphere counts).
template <bool COUNT>
__device__ __forceinline__ void finish_ray(PathState& S, const RenderParams& P, V3 inv, float closest, int hit,
                                           const float* sph_lds, const float4* shd_lds, TraceCounts& cnt, uint64_t s0) {
    const int h0 = hit;
    float4 e0 = make_float4(0.f, 0.f, 0.f, 0.f), e1 = e0;
    if (h0 >= 0) {
        const float4* Rh = P.shade + 3u * (uint32_t)h0;
        e0 = Rh[0];
        e1 = Rh[1];
    }
    __asm__ volatile("" : : : "memory");   // keep the loads ahead of the sphere test
    ray_spheres<true>(P.prims, P.sphere_chain, P.n_chain, P.sphere_first, P.n_ray_spheres, S.o, S.d,
                      sphere_inv(S.d, inv), closest, hit, sph_lds);
    if (COUNT || kProfilePass) cnt.cyc_sph += shader_clock() - s0;
    bool staged = false;
    float inv_r = 0.f;
    if (hit != h0 && hit >= 0) {   // a per-ray sphere won: its record from LDS (two spheres) or HBM
        if (P.n_ray_spheres == 2) {
            const int k = hit == __float_as_int(sph_lds[26]) ? 3 : 0;
            e0 = shd_lds[k];
            e1 = shd_lds[k + 1];
            inv_r = shd_lds[k + 2].x;
            staged = true;
        } else {
            const float4* Rh = P.shade + 3u * (uint32_t)hit;
            e0 = Rh[0];
            e1 = Rh[1];
        }
    }
    shade_rec(S, P, hit, closest, e0, e1, staged, inv_r);
}

// VARIANT 0: per-lane traversal (leaf loops inside the lane).  VARIANT 1: cooperative leaves.
// VARIANT 2: cooperative leaves + traversal-step scheduling.  MINW: occupancy target (waves per SIMD)
// handed to the register allocator through __launch_bounds__.
#ifdef CRT_PROFILE_WAVE_TIMES
// Profiling build only (tools/build_profile_lib.sh): per-wave start/end of the last render launch
// (s_memrealtime, 100 MHz), read with crt_profile_wave_times — the occupancy timeline of the launch.
__device__ unsigned long long g_wave_prof[2 * 4 * 65536];
#endif
#ifdef CRT_PROFILE_CRIT_TRACE
// Profiling build only (tools/crit_trace.py): the first workgroup of a variant-8 launch (the most expensive tile) logs
// s_memrealtime and its live / parked lane counts every 16 loop iterations, and every wave logs where it ran (HW_ID,
// XCC_ID), so the critical wave's iteration rate can be set against the waves sharing its SIMD over time
__device__ unsigned long long g_crit_trace[2 * 16384];
__device__ unsigned g_wave_hw[2 * 4 * 65536];
#endif

// ---- tail fill: the prologue and epilogue of a variant-8 block (crt_render_body.inc) ----
// A launch with tail fill has fill_heads + fill_tiles blocks.  Block b < fill_heads is the head of the tile at rank b
// of the cost order: for b < fill_tiles it renders the first spp - fill_spp samples of its pixels, stores their sums
// and RNG state as every block does and sets the rank's flag to 1.  Block fill_heads + k is the tail part of rank k:
// it continues those pixels from the stored sums and state over the last fill_spp samples, exactly as a render with
// CRT_RENDER_ACCUMULATE continues a frame, and sets the flag to 2.  Blocks are dispatched in index order, so the tail
// parts arrive when the launch starts to drain, as small items of tiles that ended long before.  A tail part whose
// flag is not 1 returns at once and touches nothing: no block ever waits for another (no loop in these helpers,
// tests/test_tail_fill_cpu.py), and the sweep launch that follows on the stream (fill_heads = 0: tail parts only)
// renders what is left.  The flag's release and acquire are at agent scope: a head and its tail part usually run
// on different XCDs, whose L2s are not coherent with each other.
// fill_prologue: the block's rank, sample count and whether it continues stored sums; false = return at once.  `note`
// (LDS of the wave) keeps for fill_epilogue the flag to set and its value (0: none), so that nothing of this, not
// even the launch argument that holds the flags, is live in a register across the render loop.
struct FillNote {
    uint32_t* flag;    // the rank's flag
    uint32_t* done;    // the launch's count of rendered tail parts
    uint32_t set;      // 0: nothing to set; 1: a head that held samples back; 2: a tail part
};
__device__ __forceinline__ bool fill_prologue(const RenderParams& P, uint32_t b, uint32_t& rank, int& spp, int& accumulate,
                                              FillNote* note) {
    rank = b;
    spp = P.spp;
    accumulate = P.accumulate;
    uint32_t set = 0;
    if (P.queue) {
        if (b >= fill_heads(P)) {
            rank = b - fill_heads(P);
            const uint32_t f = __hip_atomic_load(fill_flags(P) + rank, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (__builtin_amdgcn_readfirstlane(f) != 1u) return false;
            spp = fill_spp(P);
            accumulate = 1;
            set = 2;
        } else if (b < fill_tiles(P)) {
            spp = P.spp - fill_spp(P);
            set = 1;
        }
    }
    if (threadIdx.x == 0) {
        note->flag = set ? fill_flags(P) + rank : nullptr;
        note->done = set ? fill_done(P) : nullptr;
        note->set = set;
    }
    return true;
}
// fill_epilogue: after the block stored its pixels' sums and state.  The barrier orders every lane's stores before
// lane 0's release (one wave per workgroup).
__device__ __forceinline__ void fill_epilogue(const FillNote* note, int lane) {
    const uint32_t set = __builtin_amdgcn_readfirstlane(note->set);
    if (set == 0) return;
    __syncthreads();
    if (lane == 0) {
        __hip_atomic_store(note->flag, set, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (set == 2u) atomicAdd(note->done, 1u);
    }
}
// ---- end of the tail-fill helpers ----

// Waves per workgroup: 4 (16x16 pixels), or 1 for variant 8 (one 8x8 tile per workgroup, so a finished wave frees
// its slot at once instead of holding it until its three siblings end).
template <int VARIANT> struct KernelShape { static constexpr int waves = VARIANT == 8 || VARIANT == 10 ? 1 : 4; };

// The render kernel of (COUNT, VARIANT, MINW); its body is crt_render_body.inc.  The plain variant-8 kernels are built
// twice from that body: under this name the frozen twin, in which the knobs that never move in a default launch of a
// reference-shaped scene are constants instead of kernel arguments tested in every step and pass (which frees the
// scalar registers their tests held), and crt_render_open_kernel, the open twin, which reads every
// knob from P.  The host launches the frozen twin only where all its facts hold (render_launch_frozen), so both give
// the same bits.  (The body is an include and not a __device__ function: called from the kernels, by reference or by
// value, it changed the assembly of 44 or 45 of the 45 other render kernels, profiles/frozen_launch.)
// Phase priority of the frozen twins (crt_render_body.inc, DESIGN.md §5b, profiles/phase_priority): a wave's s_setprio
// level while it traverses (CRT_PRIO_TRAVERSAL) and while it runs a regeneration pass (CRT_PRIO_PASS); equal levels
// emit no s_setprio at all.  Traversal over pass gains where the launch is bound by throughput (config C at occupancy
// 7: -2.3 %; the reverse order, the control, +2.4 %) and loses where it is bound by the sample chains of its most
// expensive tiles, whose waves' passes then wait (config B at occupancy 4: +4.6 %).  So, by kernel:
//   MINW >= CRT_PRIO_KEEP_BELOW (7)   every wave lowers itself for its passes;
//   below it (5, 6)                   a wave that is draining (n_live < regen_t) or renders a critical tile keeps the
//                                     traversal level through its passes (chain-bound or not: -1.5 % and -3.7 %);
//   MINW < CRT_PRIO_MIN_W (4)         no phase priority: the kernel a chain-bound frame is given keeps its text.
// Compile-time only: a candidate is a library of its own (CRT_HIP_LIB).
#ifndef CRT_PRIO_TRAVERSAL
#define CRT_PRIO_TRAVERSAL 2
#endif
#ifndef CRT_PRIO_PASS
#define CRT_PRIO_PASS 0
#endif
#ifndef CRT_PRIO_MIN_W
#define CRT_PRIO_MIN_W 5
#endif
#ifndef CRT_PRIO_KEEP_BELOW
#define CRT_PRIO_KEEP_BELOW 7
#endif
template <bool COUNT, int VARIANT, int MINW>
__global__ __launch_bounds__(64 * KernelShape<VARIANT>::waves, MINW) void crt_render_kernel(RenderParams P) {
    constexpr bool FROZEN = VARIANT == 8 && !COUNT;
#include "crt_render_body.inc"
}
// crt_render_kernel<false, 8, MINW> with every knob read from P
// (VARIANT = 8 only; a template parameter so that the body's other variants stay discarded statements)
template <int VARIANT, int MINW>
__global__ __launch_bounds__(64 * KernelShape<VARIANT>::waves, MINW) void crt_render_open_kernel(RenderParams P) {
    static_assert(VARIANT == 8, "only the plain variant-8 kernels have twins");
    constexpr bool COUNT = false, FROZEN = false;
#include "crt_render_body.inc"
}

struct CompareParams {
    RenderParams A;
    const float4* __restrict__ nodes_b;
    const float4* __restrict__ prims_b;
    int n_nodes_b, n_layouts_b;
    int width_a, width_b;
    int sphere_first_b, n_spheres_b;
    const float4* chain_b;
    int n_chain_b;
    float* dump;          // optional: up to max_dump differing rays, 10 floats each
    int max_dump;
};

__global__ __launch_bounds__(256) void crt_compare_kernel(CompareParams Q) {
    const RenderParams& P = Q.A;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= P.width || y >= P.height) return;
    const int pix = y * P.width + x;
    PathState S;
    const uint32_t* r = P.rng + 6 * (size_t)pix;
    S.s = rng_load(r);
    S.pixel = v3(0.f, 0.f, 0.f);
    S.o = v3(0, 0, 0); S.d = v3(0, 0, 1); S.thr = v3(1, 1, 1);
    S.remaining = P.spp; S.bounce = 0; S.need_new = true; S.rays = 0; S.paths = 0;
    const CamRegs C = cam_regs(P.cam, P.width, P.height, P.rcp_w, P.rcp_h, P.fast_uv);
    TraceCounts cnt{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long n_rank = 0, n_t = 0, n_bmiss = 0, n_amiss = 0;
    while (next_ray(S, C, x, y, P.max_bounces)) {
        ++S.rays;
        float ta, tb;
        const int ha = Q.width_a == 4 ? trace4(P.nodes, P.prims, P.sphere_chain, P.n_chain, P.sphere_first, P.n_ray_spheres,
                                               S.o, S.d, ta)
                                      : trace<false>(P.nodes, P.prims, P.n_nodes, layout_base(S.d, P.n_layouts, P.n_nodes),
                                                     S.o, S.d, ta, cnt);
        const int hb = Q.width_b == 4 ? trace4(Q.nodes_b, Q.prims_b, Q.chain_b, Q.n_chain_b, Q.sphere_first_b, Q.n_spheres_b,
                                               S.o, S.d, tb)
                                      : trace<false>(Q.nodes_b, Q.prims_b, Q.n_nodes_b,
                                                     layout_base(S.d, Q.n_layouts_b, Q.n_nodes_b), S.o, S.d, tb, cnt);
        if (ha != hb) {
            ++n_rank;
            n_bmiss += (hb < 0);
            n_amiss += (ha < 0);
            if (Q.dump) {
                const unsigned slot = atomicAdd(reinterpret_cast<unsigned*>(P.counters + 6), 1u);
                if ((int)slot < Q.max_dump) {
                    float* q = Q.dump + 10 * (size_t)slot;
                    q[0] = S.o.x; q[1] = S.o.y; q[2] = S.o.z; q[3] = S.d.x; q[4] = S.d.y; q[5] = S.d.z;
                    q[6] = __int_as_float(ha); q[7] = __int_as_float(hb); q[8] = ta; q[9] = tb;
                }
            }
        } else if (ha >= 0 && __float_as_uint(ta) != __float_as_uint(tb)) {
            ++n_t;
        }
        shade(S, P, ha, ta);
    }
    atomicAdd(&P.counters[0], (unsigned long long)S.rays);
    if (n_rank) atomicAdd(&P.counters[1], n_rank);
    if (n_t) atomicAdd(&P.counters[2], n_t);
    if (n_bmiss) atomicAdd(&P.counters[3], n_bmiss);
    if (n_amiss) atomicAdd(&P.counters[4], n_amiss);
}

// curand_init(seed, subsequence_base + pixel, 0) (CUDAKernels.h:18-26): scrambled seed, then
// v <- A^(2^67 * subsequence) v with seq[k] = A^(2^67 * 4^k) (one base-4 digit per matrix).
__global__ __launch_bounds__(256) void crt_init_rand_kernel(uint32_t* __restrict__ rng, const uint32_t* __restrict__ seq,
                                                            int n_pix, unsigned long long seed,
                                                            unsigned long long subseq_base) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n_pix) return;
    const uint32_t s0 = ((uint32_t)seed) ^ 0xaad26b49u;
    const uint32_t s1 = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    const uint32_t t0 = 1099087573u * s0;
    const uint32_t t1 = 2591861531u * s1;
    uint32_t v[5] = {123456789u + t0, 362436069u ^ t0, 521288629u + t1, 88675123u ^ t1, 5783321u + t0};
    const uint32_t dd = 6615241u + t1 + t0;
    unsigned long long n = subseq_base + (unsigned long long)pix;
    for (int k = 0; n; ++k, n >>= 2) {
        const uint32_t reps = (uint32_t)(n & 3u);
        const uint32_t* m = seq + 800 * k;
        for (uint32_t q = 0; q < reps; ++q) {
            uint32_t r[5] = {0, 0, 0, 0, 0};
            for (int i = 0; i < 5; ++i) {
                const uint32_t w = v[i];
#pragma unroll 4
                for (int j = 0; j < 32; ++j) {
                    const uint32_t msk = 0u - ((w >> j) & 1u);
                    const uint32_t* col = m + (i * 32 + j) * 5;
#pragma unroll
                    for (int c = 0; c < 5; ++c) r[c] ^= msk & col[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 5; ++c) v[c] = r[c];
        }
    }
    uint32_t* o = rng + 6 * (size_t)pix;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; o[4] = v[4]; o[5] = dd;
}

// writeColor(data, idx, m_PixelSampleScale * pixel_color) (CUDAKernels.h:164, CRTUtility.cuh:21-32)
__global__ __launch_bounds__(256) void crt_resolve_kernel(const float* __restrict__ sum, uint8_t* __restrict__ rgba,
                                                          int n_pix, float scale) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n_pix) return;
    const float r = scale * sum[3 * (size_t)pix];
    const float g = scale * sum[3 * (size_t)pix + 1];
    const float b = scale * sum[3 * (size_t)pix + 2];
    uchar4 o;
    o.x = to_u8(r); o.y = to_u8(g); o.z = to_u8(b); o.w = 255;
    reinterpret_cast<uchar4*>(rgba)[pix] = o;
}

__global__ void crt_selftest_math_kernel(const float* a, const float* b, int n, float* out, double* out64) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i], y = b[i];
    out[4 * i] = x / y;
    out[4 * i + 1] = sqrtf(fabsf(x));
    out[4 * i + 2] = 1.0f / x;
    const double dx = fabs((double)x * (double)y);
    out[4 * i + 3] = (float)sqrt((double)fabsf(x));
    out64[2 * i] = sqrt(dx);
    out64[2 * i + 1] = 1.0 - dx * dx;
}

// Exhaustive check of rcp_newton against IEEE 1.f/x over bit patterns [lo, hi) of positive floats
// (the negative half is the mirror image: both rcp and the FMAs are sign-symmetric, still checked).
__global__ __launch_bounds__(256) void crt_selftest_rcp_kernel(uint32_t lo, uint32_t hi, unsigned long long* bad,
                                                               uint32_t* first_bad) {
    const uint32_t stride = gridDim.x * blockDim.x;
    unsigned long long nbad = 0;
    for (uint32_t b = lo + blockIdx.x * blockDim.x + threadIdx.x; b < hi && b >= lo; b += stride) {
        const float x = __uint_as_float(b);
        const float a = rcp_newton(x), c = 1.0f / x;
        const float an = rcp_newton(-x), cn = 1.0f / -x;
        if (__float_as_uint(a) != __float_as_uint(c) || __float_as_uint(an) != __float_as_uint(cn)) {
            ++nbad;
            atomicMin(first_bad, b);
        }
        if (b > 0xffffffffu - stride) break;
    }
    if (nbad) atomicAdd(bad, nbad);
}

__global__ __launch_bounds__(256) void crt_selftest_sqrt_kernel(uint32_t lo, uint32_t hi, unsigned long long* bad,
                                                                uint32_t* first_bad) {
    const uint32_t stride = gridDim.x * blockDim.x;
    unsigned long long nbad = 0;
    for (uint32_t b = lo + blockIdx.x * blockDim.x + threadIdx.x; b < hi && b >= lo; b += stride) {
        const float x = __uint_as_float(b);
        if (__float_as_uint(sqrt_rsq(x)) != __float_as_uint(sqrtf(x))) {
            ++nbad;
            atomicMin(first_bad, b);
        }
        if (b > 0xffffffffu - stride) break;
    }
    if (nbad) atomicAdd(bad, nbad);
}

// unit() as shade_rec runs it: one call for all the lanes of a wave (in: n x 3 floats, one wave per 64 vectors), so the
// wave-uniform choice between the fast and the IEEE square root and reciprocal is made over whatever mix of lengths
// the caller puts into a wave.
__global__ __launch_bounds__(64) void crt_selftest_unit_kernel(const float* __restrict__ in, int n,
                                                               float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 u = unit(v3(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
    out[3 * i] = u.x; out[3 * i + 1] = u.y; out[3 * i + 2] = u.z;
}

// Exhaustive check of next_ray's division for one frame dimension b: every float a in [lo, hi] (all values (x + U) can
// take) through uv_div against IEEE a / b.
__global__ __launch_bounds__(256) void crt_uv_div_check_kernel(float b, float r, uint32_t lo, uint32_t hi,
                                                               unsigned long long* bad) {
    const uint32_t stride = gridDim.x * blockDim.x;
    unsigned long long nbad = 0;
    for (uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x; i <= hi && i >= lo; i += stride) {
        const float a = __uint_as_float(i);
        if (__float_as_uint(uv_div(a, b, r)) != __float_as_uint(a / b)) ++nbad;
        if (i > 0xffffffffu - stride) break;
    }
    if (nbad) atomicAdd(bad, nbad);
}

__global__ __launch_bounds__(64) void crt_selftest_scan_kernel(const int* in, int* out, int n_waves) {
    const int w = blockIdx.x;
    if (w >= n_waves) return;
    const int lane = threadIdx.x;
    const int x = in[64 * w + lane];
    out[3 * (64 * w + lane)] = wave_inclusive_scan(x, lane);
    out[3 * (64 * w + lane) + 1] = wave_inclusive_scan_shfl(x, lane);
    // the kernels' max-scan runs on owner + 1 (0 = none); inputs here are >= -1
    out[3 * (64 * w + lane) + 2] = (int)wave_inclusive_max_scan_u((uint32_t)(x + 1)) - 1;
}

// Known-answer self-test of the render path's own primitive functions (tests/golden/primitives.json):
// kind 0 = tri_test_rec (Möller–Trumbore, window [0.001, tmax]), 1 = ref_scene_box (AABB::hit against
// [0.001, inf) with the exact 1/d), 2 = sphere_candidate (Sphere::hit, window [0.001, tmax]), 3 = next_ray's
// Camera::getRay for a new sample.
__global__ void crt_selftest_geometry_kernel(int kind, const float* __restrict__ in, int n, float* __restrict__ out,
                                             uint32_t* __restrict__ rng, crt_camera_desc cam, int w, int h, float rcp_w,
                                             float rcp_h, int fast_uv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (kind == 0) {
        const float* q = in + 17 * i;
        const V3 o = v3(q[0], q[1], q[2]), d = v3(q[3], q[4], q[5]);
        const float e1[3] = {q[9] - q[6], q[10] - q[7], q[11] - q[8]}, e2[3] = {q[12] - q[6], q[13] - q[7], q[14] - q[8]};
        const float4 f0 = make_float4(q[6], q[7], q[8], e1[0]), f1 = make_float4(e1[1], e1[2], e2[0], e2[1]);
        const float4 f2 = make_float4(e2[2], 0.f, 0.f, 0.f);
        out[i] = tri_test_rec(f0, f1, f2, o, d, q[16]);
    } else if (kind == 1) {
        const float* q = in + 14 * i;
        const V3 o = v3(q[0], q[1], q[2]), d = v3(q[3], q[4], q[5]);
        const V3 inv = v3(recip_exact_any(d.x), recip_exact_any(d.y), recip_exact_any(d.z));
        out[i] = ref_scene_box(make_float4(q[6], q[7], q[8], q[9]), make_float4(q[10], q[11], 0.f, 0.f), o, inv) ? 1.f : 0.f;
    } else if (kind == 2) {
        const float* q = in + 12 * i;
        const V3 o = v3(q[0], q[1], q[2]), d = v3(q[3], q[4], q[5]);
        out[i] = sphere_candidate(make_float4(q[6], q[7], q[8], q[9]), make_float4(q[9] * q[9], 0.f, 0.f, 0.f), o, d,
                                  q[11]);
    } else if (kind == 4) {   // the per-ray spheres' skip test (sphere_beyond) against closest = q[10]
        const float* q = in + 12 * i;
        const float ocx = q[0] - q[6], ocy = q[1] - q[7], ocz = q[2] - q[8];
        const float qa = dot(v3(q[3], q[4], q[5]), v3(q[3], q[4], q[5]));
        const float hb = (ocx * q[3] + ocy * q[4]) + ocz * q[5];
        const float qc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - q[9] * q[9];
        const float disc = hb * hb - qa * qc;
        out[i] = sphere_beyond(qa, hb, disc, q[10]) ? 1.f : 0.f;
    } else {
        const int* xy = reinterpret_cast<const int*>(in);
        const CamRegs C = cam_regs(cam, w, h, rcp_w, rcp_h, fast_uv);
        uint32_t* r = rng + 6 * (size_t)i;
        PathState S = new_sample_state(rng_load(r));
        next_ray(S, C, xy[2 * i], xy[2 * i + 1], 1);
        rng_store(r, S.s);
        float* o6 = out + 6 * (size_t)i;
        o6[0] = S.o.x; o6[1] = S.o.y; o6[2] = S.o.z; o6[3] = S.d.x; o6[4] = S.d.y; o6[5] = S.d.z;
    }
}

// Known-answer self-test of the render kernels' material step (tests/golden/scatter_kat.npz): shade_rec() on a
// hand-made shading record, then next_ray() with no samples left, so that only the bounce limit and the roulette of the
// bounce that follows run.  64-lane blocks: the order of the records is the composition of the waves.
//   in : 32 words per record: o3 d3 t hit | r0 (outward normal3, SHADE_* code) | payload4 | throughput3 bounce |
//        max_bounces rng6 (hit, the code, bounce and max_bounces are integers)
//   out: 20 words per record: ended | o3 d3 | throughput3 | bounce | what the path added to its pixel | rng6
__global__ __launch_bounds__(64) void crt_selftest_shade_kernel(const float* __restrict__ in, int n,
                                                                float* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* q = in + 32 * (size_t)i;
    const uint32_t* qi = reinterpret_cast<const uint32_t*>(q);
    PathState S = new_sample_state(rng_load(qi + 21));
    S.o = v3(q[0], q[1], q[2]);
    S.d = v3(q[3], q[4], q[5]);
    S.thr = v3(q[16], q[17], q[18]);
    S.bounce = (int)qi[19];
    S.remaining = 0;
    S.need_new = false;
    const RenderParams P{};
    shade_rec(S, P, qi[7] ? 0 : -1, q[6], make_float4(q[8], q[9], q[10], q[11]), make_float4(q[12], q[13], q[14], q[15]),
              true, 0.f);
    next_ray(S, CamRegs{}, 0, 0, (int)qi[20]);
    float* o = out + 20 * (size_t)i;
    uint32_t* oi = reinterpret_cast<uint32_t*>(o);
    oi[0] = S.need_new ? 1u : 0u;
    o[1] = S.o.x; o[2] = S.o.y; o[3] = S.o.z; o[4] = S.d.x; o[5] = S.d.y; o[6] = S.d.z;
    o[7] = S.thr.x; o[8] = S.thr.y; o[9] = S.thr.z;
    oi[10] = (uint32_t)S.bounce;
    o[11] = S.pixel.x; o[12] = S.pixel.y; o[13] = S.pixel.z;
    rng_store(oi + 14, S.s);
}

__global__ void crt_selftest_rng_kernel(const uint32_t* st_in, int n, int n_draw, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng s = rng_load(st_in + 6 * i);
    for (int k = 0; k < n_draw; ++k) out[(size_t)i * n_draw + k] = uniform(s);
}

// ------------------------------------------------------------------ variant 7: pixel order from the probe
// Most expensive pixels first (longest-processing-time order), so the pixels whose sample sequences take
// longest start at once and the launch ends on cheap ones.  Counting sort of the probe's per-pixel ray
// counts (keys clamped to 1023), descending; within a key the order is arbitrary (scheduling only).
constexpr int ORDER_KEYS = 1024;
constexpr int ORDER_ITEMS = 1024;   // pixels per workgroup of the sort passes
__device__ __forceinline__ uint32_t order_bucket(uint32_t cost) { return ORDER_KEYS - 1 - min(cost, (uint32_t)ORDER_KEYS - 1); }
__global__ __launch_bounds__(256) void crt_order_hist_kernel(const uint32_t* __restrict__ cost, int n,
                                                             uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[ORDER_KEYS];
    for (int i = threadIdx.x; i < ORDER_KEYS; i += 256) h[i] = 0;
    __syncthreads();
    const int b0 = blockIdx.x * ORDER_ITEMS;
    for (int i = b0 + threadIdx.x; i < min(n, b0 + ORDER_ITEMS); i += 256) atomicAdd(&h[order_bucket(cost[i])], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < ORDER_KEYS; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}
__global__ __launch_bounds__(ORDER_KEYS) void crt_order_scan_kernel(uint32_t* __restrict__ hist) {
    __shared__ uint32_t part[ORDER_KEYS];
    const int t = threadIdx.x;
    const uint32_t c = hist[t];
    part[t] = c;
    __syncthreads();
    for (int o = 1; o < ORDER_KEYS; o <<= 1) {
        const uint32_t add = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    hist[t] = part[t] - c;   // exclusive offsets
}
__global__ __launch_bounds__(256) void crt_order_scatter_kernel(const uint32_t* __restrict__ cost, int n,
                                                                uint32_t* __restrict__ hist,
                                                                uint32_t* __restrict__ order, uint32_t base) {
    __shared__ uint32_t h[ORDER_KEYS];
    for (int i = threadIdx.x; i < ORDER_KEYS; i += 256) h[i] = 0;
    __syncthreads();
    const int b0 = blockIdx.x * ORDER_ITEMS;
    uint32_t rank[ORDER_ITEMS / 256];
    for (int k = 0; k < ORDER_ITEMS / 256; ++k) {
        const int i = b0 + threadIdx.x + 256 * k;
        rank[k] = i < n ? atomicAdd(&h[order_bucket(cost[i])], 1u) : 0u;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ORDER_KEYS; i += 256)   // reserve this block's run of every key
        if (h[i]) h[i] = atomicAdd(&hist[i], h[i]);
    __syncthreads();
    for (int k = 0; k < ORDER_ITEMS / 256; ++k) {
        const int i = b0 + threadIdx.x + 256 * k;
        if (i < n) order[h[order_bucket(cost[i])] + rank[k]] = base + (uint32_t)i;
    }
}
// XCD regions (crt_renderer_set_xcd_regions): MI355X deals workgroups round-robin over its 8 XCDs, so blocks b and b + 8
// share an XCD and its 4 MiB L2 (MI355X_MICROARCH.md §Workgroup dispatch; which XCD is not fixed, and nothing depends on
// it for correctness).  This reorders the cost-sorted tile list so that the blocks of one XCD group (b % 8 == k) render
// one screen region: 8 vertical strips of equal probe cost (column sums of the tile keys), each in descending cost
// (a stable partition of the sorted list).  Every group gets n/8 blocks (+1 for the first n % 8 groups): a strip with more
// tiles than that hands its cheapest tail to a shared pool, from which the groups with fewer tiles take their last
// blocks.  One workgroup of 1024 threads; `part` and `pool` are scratch of n entries each.  Results never depend on
// the order (each pixel is one lane's sequential chain).
constexpr int XCD_GROUPS = 8;
__global__ __launch_bounds__(1024) void crt_xcd_order_kernel(uint32_t* __restrict__ order, const uint32_t* __restrict__ key,
                                                             int n, int tiles_x, uint32_t* __restrict__ part,
                                                             uint32_t* __restrict__ pool) {
    __shared__ uint32_t col_region[2048];              // tiles_x <= 2048 (checked by the host)
    __shared__ unsigned long long col_cost[2048];
    __shared__ uint32_t wave_cnt[16][XCD_GROUPS];
    __shared__ uint32_t reg_n[XCD_GROUPS], reg_off[XCD_GROUPS], run[XCD_GROUPS];
    __shared__ uint32_t cap[XCD_GROUPS], exc_off[XCD_GROUPS], def_off[XCD_GROUPS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int c = t; c < tiles_x; c += 1024) col_cost[c] = 0;
    if (t < XCD_GROUPS) run[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += 1024)   // a tile weighs its clamped key + 1, as the counting sort sees it
        atomicAdd(&col_cost[i % tiles_x], (unsigned long long)(min(key[i], (uint32_t)ORDER_KEYS - 1) + 1u));
    __syncthreads();
    if (t == 0) {   // strips of equal cost: column c joins the strip its cost midpoint falls in
        unsigned long long tot = 0;
        for (int c = 0; c < tiles_x; ++c) tot += col_cost[c];
        unsigned long long acc = 0;
        for (int c = 0; c < tiles_x; ++c) {
            const unsigned long long mid = acc + col_cost[c] / 2;
            col_region[c] = (uint32_t)min((unsigned long long)XCD_GROUPS - 1, mid * XCD_GROUPS / (tot ? tot : 1));
            acc += col_cost[c];
        }
    }
    __syncthreads();
    // stable partition of the sorted list by strip (ballot ranks inside a wave, wave totals across the workgroup)
    for (int b0 = 0; b0 < n; b0 += 1024) {
        const int i = b0 + t;
        const uint32_t tile = i < n ? order[i] : 0u;
        const uint32_t r = i < n ? col_region[tile % (uint32_t)tiles_x] : 0xffu;
        uint32_t rank = 0;
        for (int g = 0; g < XCD_GROUPS; ++g) {
            const uint64_t m = __builtin_amdgcn_ballot_w64(r == (uint32_t)g);
            if (r == (uint32_t)g) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wave_cnt[wv][g] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (r < (uint32_t)XCD_GROUPS) {
            uint32_t before = run[r];
            for (int w = 0; w < wv; ++w) before += wave_cnt[w][r];
            part[(size_t)r * n + before + rank] = tile;   // strip r's list at part[r * n ...]
        }
        __syncthreads();
        if (t < XCD_GROUPS)
            for (int w = 0; w < 16; ++w) run[t] += wave_cnt[w][t];
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t q = (uint32_t)n / XCD_GROUPS, e = (uint32_t)n % XCD_GROUPS;
        uint32_t eo = 0, dd = 0;
        for (int g = 0; g < XCD_GROUPS; ++g) {
            reg_n[g] = run[g];
            cap[g] = q + ((uint32_t)g < e ? 1u : 0u);
            exc_off[g] = eo;
            def_off[g] = dd;
            if (run[g] > cap[g]) eo += run[g] - cap[g];
            else dd += cap[g] - run[g];
        }
        (void)reg_off;
    }
    __syncthreads();
    for (int g = 0; g < XCD_GROUPS; ++g)   // the strips' tails beyond their group's share, concatenated
        for (uint32_t i = cap[g] + (uint32_t)t; i < reg_n[g]; i += 1024) pool[exc_off[g] + i - cap[g]] = part[(size_t)g * n + i];
    __syncthreads();
    for (int b = t; b < n; b += 1024) {
        const int g = b % XCD_GROUPS;
        const uint32_t i = (uint32_t)(b / XCD_GROUPS);
        order[b] = i < reg_n[g] ? part[(size_t)g * n + i] : pool[def_off[g] + i - reg_n[g]];
    }
}

// Variant 8: the key of an 8x8 tile is its most expensive pixel (the wave ends with its slowest lane);
// key_mode 1 adds the mean pixel (ties between tiles with equal maxima); key_mode 2 raises a tile to 3/4 of
// the largest key among its 8 neighbours (a 4-spp probe underestimates some tiles next to expensive ones, and an
// underestimated tile dispatched late becomes the launch's tail).
// stats (optional, zeroed by the caller): [0] the largest tile work, [1] the sum of the tile works, both in probe cost units
// over the probed pixels (a tile's work = the sum of its probed pixels' costs); the host's occupancy choice (crt_render)
__global__ void crt_tile_cost_kernel(const uint32_t* __restrict__ pix_cost, int width, int height, int tiles_x,
                                     int n_tiles, uint32_t* __restrict__ tile_cost, int key_mode, int stride,
                                     unsigned long long* __restrict__ stats) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const int x0 = (t % tiles_x) * 8, y0 = (t / tiles_x) * 8;
    uint32_t m = 0, sum = 0, k = 0;
    for (int y = y0; y < min(height, y0 + 8); y += stride)   // a subsampled probe wrote pixels with x, y % stride == 0
        for (int x = x0; x < min(width, x0 + 8); x += stride) {
            const uint32_t c = pix_cost[(size_t)y * width + x];
            m = max(m, c);
            sum += c;
            ++k;
        }
    tile_cost[t] = key_mode == 1 ? m + sum / max(1u, k) : m;
    if (stats) {
        atomicMax(&stats[0], (unsigned long long)sum);
        atomicAdd(&stats[1], (unsigned long long)sum);
    }
}
__global__ void crt_tile_neighbour_kernel(const uint32_t* __restrict__ key_in, int tiles_x, int n_tiles,
                                          uint32_t* __restrict__ key_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const int tx = t % tiles_x, ty = t / tiles_x, tiles_y = (n_tiles + tiles_x - 1) / tiles_x;
    uint32_t nb = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int x = tx + dx, y = ty + dy;
            if ((dx || dy) && x >= 0 && x < tiles_x && y >= 0 && y < tiles_y && y * tiles_x + x < n_tiles)
                nb = max(nb, key_in[y * tiles_x + x]);
        }
    key_out[t] = max(key_in[t], (nb * 3u) / 4u);
}

// No probe: 8x8 tiles in row order, pixels row-major inside a tile (a wave's first 64 slots are one tile, so
// its primary rays are coherent); slots of partial edge tiles hold ~0.
// Pixel sharding (crt_renderer_set_pixel_shard): the tiles of other shards get key 0 and this shard's keys + 1, so
// the descending cost order puts exactly this shard's tiles first, whatever order the counting sort gives equal keys.
__global__ void crt_tile_shard_mask_kernel(uint32_t* __restrict__ key, int n_tiles, int shard, int shards) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const uint32_t k = key[t];
    key[t] = t % shards == shard ? (k < 0xffffffffu ? k + 1u : k) : 0u;
}

// Pixel sharding without the probe: slot k holds tile k * shards + shard.
__global__ void crt_shard_tiles_kernel(uint32_t* __restrict__ order, int n_tiles, int shard, int shards) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k * shards + shard < n_tiles) order[k] = (uint32_t)(k * shards + shard);
}

// Variant 7 with the temporal order (crt_renderer_set_temporal_order): slots of 8x8 tiles in the order tile_order
// holds (the tiles most expensive first by the previous frame's rays per pixel), pixels row-major inside a tile.
__global__ void crt_expand_tile_order_kernel(const uint32_t* __restrict__ tile_order, uint32_t* __restrict__ order,
                                             int width, int height, int n_slots) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const int tiles_x = (width + 7) / 8, tile = (int)tile_order[s >> 6], q = s & 63;
    const int x = (tile % tiles_x) * 8 + (q & 7), y = (tile / tiles_x) * 8 + (q >> 3);
    order[s] = (x < width && y < height) ? (uint32_t)(y * width + x) : 0xffffffffu;
}
__global__ void crt_order_tiles_kernel(uint32_t* __restrict__ order, int width, int height, int n_slots) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const int tiles_x = (width + 7) / 8, tile = s >> 6, q = s & 63;
    const int x = (tile % tiles_x) * 8 + (q & 7), y = (tile / tiles_x) * 8 + (q >> 3);
    order[s] = (x < width && y < height) ? (uint32_t)(y * width + x) : 0xffffffffu;
}

// ------------------------------------------------------------------ the host half, then the features
// Here because they launch or instantiate the device functions above, in order of dependence: the core's host half, one
// responsibility per header (the core's kernels all stay above), then each feature's kernels and host code.
#include "crt_handles.h"    // the handles, the per-handle states, the shared host helpers, the entries without a handle
#include "crt_scene.h"      // scene creation: flattening, the host SAH build, the 4-wide collapse, export
#include "crt_renderer.h"   // renderer creation, setters, synchronise, reads, getters, compare, resolve
#include "crt_dispatch.h"   // the render dispatch: the launch table, the schedules, crt_renderer_render
#include "crt_selftest.h"   // the host side of the self-tests
#include "crt_trace.h"
#include "crt_paths.h"
#include "crt_adaptive.h"
#include "crt_denoise.h"
#include "crt_reproject.h"
#include "crt_variance.h"
