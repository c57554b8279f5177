// crt_trace.h — batch ray queries (closest hit, occlusion) over a device scene: kernels + C ABI.
//
// Textually part of crt_hip.hip (included at its end): the kernels instantiate that file's traversal functions
// unchanged -- traverse_step4 / top_steps / ray_spheres for 4-wide scenes, trace / trace4 per lane -- so a query sees
// exactly the boxes, primitives and hit rule the render kernels see.  Nothing here is used by a render kernel.
//
//   crt_trace_kernel<ANY, COUNT>   4-wide scenes, the hot path: variant 7's persistent loop with the pixel replaced by
//                                  a ray index and no shading state.  One wave per workgroup; a lane without a node is
//                                  idle; a refill pass finishes the idle lanes' rays (per-ray spheres, record store)
//                                  and hands them the next indices of one global counter.  All global loads of rays
//                                  and stores of results sit in the pass, never in the step loop (the
//                                  removed wavefront variant 5 paid a vmcnt wait per node load for them).
//   crt_trace_lane_kernel<COUNT>   every scene: one ray per lane through trace<> (threaded) or trace4 (4-wide), the
//                                  bit-exact baseline the stream kernel is measured against; no early exit.
//   crt_trace_indirect_kernel<ANY, COUNT>, crt_trace_lane_indirect_kernel<COUNT>
//                                  the same two bodies (crt_trace_stream_body.inc, crt_trace_lane_body.inc) with the
//                                  number of rays read from a device word and clamped to the launch's capacity
//                                  (DESIGN.md §18).
#pragma once

struct TraceParams {
    RenderParams P;                        // the scene's arrays, stack split, per-ray spheres, error word
    const float4* __restrict__ rays;       // 2 rows per ray: (o.xyz, tmax) (d.xyz, -)
    float4* __restrict__ hits;             // 2 rows per ray, or null
    unsigned char* __restrict__ occ;       // 1 byte per ray, or null
    const int4* __restrict__ ident;        // per rank: (object, primitive, material, 0)
    uint32_t n;                            // rays of this launch (< 2^31)
    uint32_t* __restrict__ next;           // stream kernel: the next unreserved ray index
    uint32_t block;                        // stream kernel: indices a wave reserves per atomicAdd (a multiple of 64)
    unsigned long long* __restrict__ stats;// COUNT: rays, boxes, triangles, spheres, step lane slots, active lanes
    int refill_threshold;                  // stream kernel: idle lanes that trigger a refill pass
    int width;                             // lane kernel: 2 = threaded nodes, 4 = 4-wide nodes
};

// The hit record (crt_hit) and / or the occlusion byte of ray i.  (t, rank) is the traversal's closest hit over
// [0.001, inf); tmax filters it.  Identity from the rank's identity row, the normal from its shading record's first
// row (triangle: the stored unit normal; sphere: (1 / r) * (P - c), Sphere.cuh:44, as shade_rec computes it).
__device__ __forceinline__ void trace_store(const TraceParams& T, uint32_t i, V3 o, V3 d, float tmax, float t, int hit) {
    const bool ok = hit >= 0 && t <= tmax;
    if (T.hits) {
        float4 a = make_float4(-1.f, 0.f, 0.f, 0.f), b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) {
            const int4 id = T.ident[hit];
            const float4* R = T.P.shade + 3u * (uint32_t)hit;
            const float4 r0 = R[0];
            V3 nrm = v3(r0.x, r0.y, r0.z);
            if (__float_as_uint(r0.w) & SHADE_SPHERE) {
                const float ir = R[2].x;
                const V3 hp = o + t * d;                    // Ray::pointAtDistance
                nrm = ir * (hp - nrm);
            }
            const bool front = dot(d, nrm) < 0;             // HitInfo::setFaceNormal
            a = make_float4(t, __int_as_float(id.x), __int_as_float(id.y), __int_as_float(id.z));
            b = make_float4(nrm.x, nrm.y, nrm.z, __int_as_float(front ? 1 : 0));
        }
        T.hits[2 * (size_t)i] = a;
        T.hits[2 * (size_t)i + 1] = b;
    }
    if (T.occ) T.occ[i] = ok ? (unsigned char)1 : (unsigned char)0;
}

__device__ __forceinline__ void trace_add_stats(const TraceParams& T, int lane, uint64_t rays, const TraceCounts& cnt,
                                                uint64_t active) {
    const uint64_t v[6] = {rays, cnt.boxes, cnt.tris, cnt.spheres, cnt.step_slots, active};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint64_t s = wave_sum_u64(v[k]);
        if (lane == 0 && s) atomicAdd(&T.stats[k], (unsigned long long)s);
    }
}

template <bool ANY, bool COUNT>
__global__ __launch_bounds__(64, 6) void crt_trace_kernel(TraceParams T) {
#define TRACE_BODY_N T.n
#define TRACE_BODY_BLOCK T.block
#include "crt_trace_stream_body.inc"
#undef TRACE_BODY_N
#undef TRACE_BODY_BLOCK
}

// The indirect forms: the number of rays is a device word the kernel reads when it runs, clamped to the
// capacity the host sized the launch by (T.n).  No row at or beyond min(*d_n, T.n) is read or written.
struct TraceIndirectParams {
    TraceParams T;                         // n: the capacity; block is not used
    const uint32_t* __restrict__ d_n;      // the ray count, on the device
};

template <bool ANY, bool COUNT>
__global__ __launch_bounds__(64, 6) void crt_trace_indirect_kernel(TraceIndirectParams I) {
    const TraceParams& T = I.T;
    const uint32_t n = min(*I.d_n, T.n);
    // trace_enqueue's rule for the indices per reservation, on the count read here and this kernel's own grid
    const uint32_t block = 64u * min(8u, max(1u, n / (64u * gridDim.x)));
#define TRACE_BODY_N n
#define TRACE_BODY_BLOCK block
#include "crt_trace_stream_body.inc"
#undef TRACE_BODY_N
#undef TRACE_BODY_BLOCK
}

template <bool COUNT>
__global__ __launch_bounds__(256) void crt_trace_lane_kernel(TraceParams T) {
#define TRACE_BODY_N T.n
#include "crt_trace_lane_body.inc"
#undef TRACE_BODY_N
}

template <bool COUNT>
__global__ __launch_bounds__(256) void crt_trace_lane_indirect_kernel(TraceIndirectParams I) {
    const TraceParams& T = I.T;
    const uint32_t n = min(*I.d_n, T.n);
#define TRACE_BODY_N n
#include "crt_trace_lane_body.inc"
#undef TRACE_BODY_N
}

// ------------------------------------------------------------------ host side
constexpr int TRACE_ERR_WORD = 6;            // d_stats word of the device error flags (RenderParams::err)
constexpr int TRACE_STAT_WORDS = 8;
constexpr int64_t TRACE_LAUNCH_RAYS = (int64_t)1 << 30;   // rays per launch (the ray counter is 32-bit)
constexpr int64_t TRACE_STAGE_RAYS = (int64_t)1 << 20;    // rays per chunk of the host-pointer entries
constexpr int64_t TRACE_STREAM_MIN_RAYS = (int64_t)1 << 20;   // automatic mode: queries from this size take the stream kernel
constexpr int TRACE4_STACK = 64;             // trace4's per-lane stack (int stack[64] in crt_hip.hip)

namespace {

// The scratch is allocated on first use and initialised on `st`, the stream its first user goes on to enqueue on.
int trace_scratch(crt_scene* S, hipStream_t st, TraceScratch** out) {
    return first_use(S->trace, "the trace scratch of this scene could not be allocated", out, [&](TraceScratch* X) -> int {
        HIP_TRY(X->d_next.alloc(1));
        HIP_TRY(X->d_stats.alloc(TRACE_STAT_WORDS));
        HIP_TRY(hipMemsetAsync(X->d_stats.get(), 0, TRACE_STAT_WORDS * sizeof(unsigned long long), st));
        HIP_TRY(X->ev0.create());
        HIP_TRY(X->ev1.create());
        HIP_TRY(hipDeviceGetAttribute(&X->n_cus, hipDeviceAttributeMultiprocessorCount, S->device));
        // the persistent grid fills the device once: CUs x the stream kernel's resident workgroups per CU
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, crt_trace_kernel<false, false>, 64, 0) != hipSuccess || nb <= 0)
            nb = 4 * 6;
        X->wg_per_cu = nb;
        return CRT_OK;
    });
}

// One query over device pointers, enqueued on st.  d_n null: rays [0, n).  Otherwise the indirect query: n is the
// capacity (at most one launch's rays) that the grid, the persistent grid and automatic mode's choice are sized by, and
// the kernel traces rays [0, min(*d_n, n)).  d_err: the word the kernels OR their error flags into; null: the handle's
// own, which every query clears.
int trace_enqueue(crt_scene* S, const crt_ray* d_rays, int64_t n, const crt_trace_options* opts, crt_hit* d_hits,
                  uint8_t* d_occ, unsigned flags, hipStream_t st, const uint32_t* d_n = nullptr, unsigned* d_err = nullptr) {
    crt_trace_options o{};
    if (opts) o = *opts;
    if (o.mode < 0 || o.mode > 2) return set_error(CRT_ERR_INVALID_ARGUMENT, "trace mode must be 0, 1 or 2");
    if (o.grid_waves < 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "grid_waves must be >= 0");
    if (o.stack_lds < 0 || o.stack_lds > 16) return set_error(CRT_ERR_INVALID_ARGUMENT, "stack_lds must be 0..16");
    if (o.refill_threshold < 0 || o.refill_threshold > 64)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "refill_threshold must be 0..64");
    if (o.mode == 2 && S->width != 4)
        return set_error(CRT_ERR_UNSUPPORTED, "the stream kernel (mode 2) needs a 4-wide rebuilt scene");
    // The lane kernel over 4-wide nodes is trace4, whose per-lane stack holds TRACE4_STACK entries and takes up to
    // three per branching ancestor (the stream kernel's encoding takes one): it drops what does not fit without a
    // report, so a tree whose bound could overflow it never goes through it.
    const bool lane_ok = S->width != 4 || 3 * (int64_t)S->stack_bound <= TRACE4_STACK;
    if (o.mode == 1 && !lane_ok)
        return set_error(CRT_ERR_UNSUPPORTED, "mode 1: the tree's stack bound exceeds the lane kernel's 64-entry stack "
                                              "(3 entries per level); use mode 0 or 2");
    // automatic: the stream kernel for large queries over 4-wide nodes (3.7 M rays: 1.08x the lane kernel's rate on
    // primary rays, 1.3x on bounce rays), the lane kernel below that (200 k rays: the persistent grid's ramp and tail
    // cost more than its lane fill gains, 0.10 ms against 0.07 ms; nothing was measured in between); the records are
    // the same either way
    const int mode = o.mode ? o.mode : (S->width == 4 && (n >= TRACE_STREAM_MIN_RAYS || !lane_ok) ? 2 : 1);
    if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "ray and hit arrays must be 16-byte aligned");
    HIP_TRY(hipSetDevice(S->device));
    TraceScratch* X = nullptr;
    if (int rc = trace_scratch(S, st, &X)) return rc;
    const bool cnt = (flags & CRT_TRACE_COUNT_WORK) != 0;

    TraceParams T{};
    RenderParams& P = T.P;
    P.nodes = S->d_nodes.get(); P.prims = S->d_prims.get(); P.mats = S->d_mats.get(); P.shade = S->d_shade.get();
    P.n_nodes = S->n_nodes; P.n_mats = S->n_mats; P.n_prims = S->n_prims; P.n_layouts = S->layouts;
    P.err = d_err ? d_err : reinterpret_cast<unsigned*>(X->d_stats.get() + TRACE_ERR_WORD);
    P.top_levels = CRT_TOP_LEVELS;
    P.stack_cap = S->stack_cap;
    P.sphere_first = S->sphere_first;
    P.n_ray_spheres = S->n_ray_spheres;
    P.sphere_chain = S->d_chain.get();
    P.n_chain = S->n_chain;
    P.tree_spheres = S->tree_spheres;
    std::memcpy(P.sph2, S->sph2, sizeof P.sph2);
    T.ident = S->d_ident.get();
    T.next = X->d_next.get();
    T.stats = X->d_stats.get();
    T.refill_threshold = o.refill_threshold ? o.refill_threshold : 44;   // the 4-wide render variants' threshold
    T.width = S->width;
    // the stream kernel's stack split: CRT_STACK6 entries per lane in LDS at the most, the rest per grid lane in HBM
    P.stack_lds = std::min(o.stack_lds ? o.stack_lds : CRT_STACK6, CRT_STACK6);
    if (S->stack_cap > 0) P.stack_lds = std::min(P.stack_lds, S->stack_cap);
    const int64_t full_grid = (int64_t)X->n_cus * X->wg_per_cu;
    if (mode == 2 && S->stack_cap > P.stack_lds) {
        const size_t need = (size_t)(S->stack_cap - P.stack_lds) * (size_t)full_grid * 64 * 4;
        if (need >= ((size_t)1 << 32))
            return set_error(CRT_ERR_INVALID_ARGUMENT, "traversal-stack overflow region would exceed 4 GiB");
        if (need / 4 > X->d_ovf.size()) {
            HIP_TRY(hipStreamSynchronize(st));
            HIP_TRY(X->d_ovf.grow(need / 4));
        }
        P.ovf = X->d_ovf.get();
    }
    // the counts and the error word of this query (crt_scene_trace_last_stats)
    HIP_TRY(hipMemsetAsync(X->d_stats.get(), 0, TRACE_STAT_WORDS * sizeof(unsigned long long), st));
    const bool any = d_hits == nullptr;   // only the occlusion byte is wanted: lanes retire at the first accepted hit
    for (int64_t at = 0; at < n; at += TRACE_LAUNCH_RAYS) {
        const int64_t m = std::min(n - at, TRACE_LAUNCH_RAYS);
        T.rays = reinterpret_cast<const float4*>(d_rays + at);
        T.hits = d_hits ? reinterpret_cast<float4*>(d_hits + at) : nullptr;
        T.occ = d_occ ? d_occ + at : nullptr;
        T.n = (uint32_t)m;
        if (mode == 2) {
            int64_t waves = std::min(full_grid, (m + 63) / 64);
            if (o.grid_waves > 0) waves = std::min<int64_t>(waves, o.grid_waves);
            const dim3 grid((unsigned)std::max<int64_t>(waves, 1)), block(64);
            // indices per reservation: 64 x k, k = the refills a lane gets from an even share of the query, at most 8
            // (measured on 3.7 M primary / bounce rays over the full grid: 128 -> 0.59 / 0.49 ms, 256 -> 0.45 / 0.36,
            // 512 -> 0.38 / 0.34, 1024 -> 0.38 / 0.39, 2048 -> 0.44 / 0.53: larger blocks leave the last waves a tail)
            T.block = 64u * (uint32_t)std::min<int64_t>(8, std::max<int64_t>(1, m / (64 * std::max<int64_t>(waves, 1))));
            HIP_TRY(hipMemsetAsync(X->d_next.get(), 0, 4, st));
            if (at == 0) HIP_TRY(hipEventRecord(X->ev0.get(), st));   // kernel_ms: from the first kernel, after the counter's reset
            if (d_n) {                           // T.block stays unused: the kernel derives it from the count it reads
                const TraceIndirectParams I{T, d_n};
                if (any) {
                    if (cnt) hipLaunchKernelGGL((crt_trace_indirect_kernel<true, true>), grid, block, 0, st, I);
                    else hipLaunchKernelGGL((crt_trace_indirect_kernel<true, false>), grid, block, 0, st, I);
                } else {
                    if (cnt) hipLaunchKernelGGL((crt_trace_indirect_kernel<false, true>), grid, block, 0, st, I);
                    else hipLaunchKernelGGL((crt_trace_indirect_kernel<false, false>), grid, block, 0, st, I);
                }
            } else if (any) {
                if (cnt) hipLaunchKernelGGL((crt_trace_kernel<true, true>), grid, block, 0, st, T);
                else hipLaunchKernelGGL((crt_trace_kernel<true, false>), grid, block, 0, st, T);
            } else {
                if (cnt) hipLaunchKernelGGL((crt_trace_kernel<false, true>), grid, block, 0, st, T);
                else hipLaunchKernelGGL((crt_trace_kernel<false, false>), grid, block, 0, st, T);
            }
        } else {
            const dim3 grid((unsigned)((m + 255) / 256)), block(256);
            if (at == 0) HIP_TRY(hipEventRecord(X->ev0.get(), st));
            if (d_n) {
                const TraceIndirectParams I{T, d_n};
                if (cnt) hipLaunchKernelGGL((crt_trace_lane_indirect_kernel<true>), grid, block, 0, st, I);
                else hipLaunchKernelGGL((crt_trace_lane_indirect_kernel<false>), grid, block, 0, st, I);
            } else if (cnt) hipLaunchKernelGGL((crt_trace_lane_kernel<true>), grid, block, 0, st, T);
            else hipLaunchKernelGGL((crt_trace_lane_kernel<false>), grid, block, 0, st, T);
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(X->ev1.get(), st));
    X->traced = true;
    return CRT_OK;
}

int trace_take_error(TraceScratch* X) {
    unsigned long long word = 0;
    HIP_TRY(hipMemcpy(&word, X->d_stats.get() + TRACE_ERR_WORD, sizeof word, hipMemcpyDeviceToHost));
    if (!word) return CRT_OK;
    // the callers waited for their stream before this read; the clear is a null-stream operation and is waited for, so
    // that a query the caller enqueues next on any stream cannot have its report cleared
    HIP_TRY(hipMemset(X->d_stats.get() + TRACE_ERR_WORD, 0, sizeof word));
    HIP_TRY(hipStreamSynchronize(0));
    std::string m = "trace kernel reported an internal error:";
    if (word & 1u) m += " primitive index out of range;";
    if (word & 2u) m += " traversal stack deeper than the scene's stack bound (entries dropped);";
    if (word & 4u) m += " leaf-round pair outside its owner's span (checked build);";
    return set_error(CRT_ERR_HIP, m + " the results are invalid");
}

// The host-pointer entries: validate, then chunks through the handle's staging buffers on the null stream.
int trace_host(const crt_scene* Sc, const crt_ray* rays, int64_t n, const crt_trace_options* opts, crt_hit* hits,
               uint8_t* occ) {
    if (!Sc || n < 0 || (n > 0 && (!rays || (!hits && !occ)))) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument or n < 0");
    if (n > 0x7fffffffll) return set_error(CRT_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 rays");
    if (n == 0) return CRT_OK;
    if (int rc = crt_trace_validate_rays(rays, n, nullptr)) return rc;
    crt_scene* S = const_cast<crt_scene*>(Sc);   // the scratch belongs to the handle (handles are not thread-safe)
    HIP_TRY(hipSetDevice(S->device));
    TraceScratch* X = nullptr;
    if (int rc = trace_scratch(S, 0, &X)) return rc;
    const int64_t chunk = std::min(n, TRACE_STAGE_RAYS);
    const size_t c = (size_t)chunk;
    if (c > X->d_rays.size() || c > X->d_hits.size() || c > X->d_occ.size()) {   // the three grow together
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(X->d_rays.grow(c));
        HIP_TRY(X->d_hits.grow(c));
        HIP_TRY(X->d_occ.grow(c));
    }
    for (int64_t at = 0; at < n; at += chunk) {
        const int64_t m = std::min(n - at, chunk);
        HIP_TRY(hipMemcpy(X->d_rays.get(), rays + at, (size_t)m * sizeof(crt_ray), hipMemcpyHostToDevice));
        if (int rc = trace_enqueue(S, X->d_rays.get(), m, opts, hits ? X->d_hits.get() : nullptr,
                                   occ ? X->d_occ.get() : nullptr, 0, nullptr))
            return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        if (hits) HIP_TRY(hipMemcpy(hits + at, X->d_hits.get(), (size_t)m * sizeof(crt_hit), hipMemcpyDeviceToHost));
        if (occ) HIP_TRY(hipMemcpy(occ + at, X->d_occ.get(), (size_t)m, hipMemcpyDeviceToHost));
        if (int rc = trace_take_error(X)) return rc;
    }
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_trace_validate_rays(const crt_ray* rays, int64_t n, int64_t* first_bad) {
    if (n < 0 || (n > 0 && !rays)) return set_error(CRT_ERR_INVALID_ARGUMENT, "null rays or n < 0");
    for (int64_t i = 0; i < n; ++i) {
        const crt_ray& r = rays[i];
        const char* why = nullptr;
        for (int a = 0; a < 3 && !why; ++a) {
            if (!std::isfinite(r.origin[a])) why = "origin is not finite";
            else if (!(std::fabs(r.origin[a]) < 0x1p59f)) why = "|origin| is 2^59 or more";
            else if (!std::isfinite(r.dir[a])) why = "direction is not finite";
        }
        if (!why && r.dir[0] == 0.f && r.dir[1] == 0.f && r.dir[2] == 0.f) why = "direction is all zero";
        if (!why && r.tmax != r.tmax) why = "tmax is NaN";
        if (why) {
            if (first_bad) *first_bad = i;
            return set_error(CRT_ERR_INVALID_ARGUMENT, "ray " + std::to_string(i) + ": " + why);
        }
    }
    return CRT_OK;
}

int crt_scene_trace(const crt_scene* S, const crt_ray* rays, int64_t n, const crt_trace_options* opts, crt_hit* hits_out) {
    if (n > 0 && !hits_out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null hits_out");
    return trace_host(S, rays, n, opts, hits_out, nullptr);
}

int crt_scene_occluded(const crt_scene* S, const crt_ray* rays, int64_t n, const crt_trace_options* opts, uint8_t* out) {
    if (n > 0 && !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null out");
    return trace_host(S, rays, n, opts, nullptr, out);
}

int crt_scene_trace_device(const crt_scene* S, const crt_ray* d_rays, int64_t n, const crt_trace_options* opts,
                           crt_hit* d_hits, uint8_t* d_occluded, unsigned flags, void* stream) {
    if (!S || n < 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "null scene or n < 0");
    if (n == 0) return CRT_OK;
    if (!d_rays || (!d_hits && !d_occluded)) return set_error(CRT_ERR_INVALID_ARGUMENT, "null rays, or neither hits nor occluded");
    return trace_enqueue(const_cast<crt_scene*>(S), d_rays, n, opts, d_hits, d_occluded, flags, (hipStream_t)stream);
}

int crt_scene_trace_indirect_device(const crt_scene* S, const crt_ray* d_rays, const uint32_t* d_n, int64_t capacity,
                                    const crt_trace_options* opts, crt_hit* d_hits, uint8_t* d_occluded, unsigned flags,
                                    void* stream) {
    if (!S) return set_error(CRT_ERR_INVALID_ARGUMENT, "indirect trace: null scene");
    if (capacity < 0 || capacity > TRACE_LAUNCH_RAYS)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "indirect trace: capacity must be in [0, 2^30] (one launch serves one query)");
    if (!d_n || ((uintptr_t)d_n & 3u))
        return set_error(CRT_ERR_INVALID_ARGUMENT, "indirect trace: the count must be a non-null, 4-byte aligned device word");
    if (capacity == 0) return CRT_OK;
    if (!d_rays || (!d_hits && !d_occluded))
        return set_error(CRT_ERR_INVALID_ARGUMENT, "indirect trace: null rays, or neither hits nor occluded");
    return trace_enqueue(const_cast<crt_scene*>(S), d_rays, capacity, opts, d_hits, d_occluded, flags, (hipStream_t)stream, d_n);
}

int crt_scene_trace_last_stats(const crt_scene* S, crt_trace_stats* out) {
    if (!S || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    *out = crt_trace_stats{};
    TraceScratch* X = S->trace.get();
    if (!X || !X->traced) return set_error(CRT_ERR_INVALID_ARGUMENT, "no trace on this scene yet");
    HIP_TRY(hipSetDevice(S->device));
    HIP_TRY(hipEventSynchronize(X->ev1.get()));
    HIP_TRY(hipEventElapsedTime(&out->kernel_ms, X->ev0.get(), X->ev1.get()));
    unsigned long long w[TRACE_STAT_WORDS];
    HIP_TRY(hipMemcpy(w, X->d_stats.get(), sizeof w, hipMemcpyDeviceToHost));
    out->rays = w[0]; out->box_tests = w[1]; out->tri_tests = w[2]; out->sphere_tests = w[3];
    out->step_lane_slots = w[4]; out->step_active_lanes = w[5];
    return trace_take_error(X);
}

}  // extern "C"
