// crt_paths.h — path steps over ray batches: camera rays and one bounce of material scattering, kernels + C ABI.
//
// Textually part of crt_hip.hip (included at its end, after crt_trace.h): the kernels call that file's and
// crt_device.h's device functions unchanged -- cam_regs, new_sample_state and next_ray's camera block, the XORWOW draws,
// unit, reflect, refract, schlick_r0, cannot_refract_exact, recip_exact_wave, sky_unit, rand_in_unit_sphere -- so a
// batch step computes what the render kernels compute between two traces, bit for bit.  Nothing here is used by a
// render or trace kernel.
//
//   crt_camera_rays_kernel   one lane per pixel of the batch: next_ray() for a new sample on the pixel's RNG stream.
//   scatter_step()           one bounce of one path, the one copy both kernels below call: shade_rec()'s body on the
//                            crt_hit record instead of the per-rank shading record (the normal, the face and the
//                            material index come from the record, the material's code and payload from the scene's
//                            per-material rows), then next_ray()'s bounce-limit test and Russian roulette for the
//                            bounce that follows.
//   crt_path_step_kernel     one lane per path: scatter_step() in place.
//   crt_path_advance_kernel, crt_path_advance_indirect_kernel
//                            further down: step, regenerate and compact, and the same body
//                            (crt_path_advance_body.inc) over a device-side entry count (§18).
//   crt_path_finish_kernel   after those: one lane per path, run to the end of its pixel's samples with the lane
//                            kernels' trace in the lane (§19).
//
// unit(), the reciprocal and the glass test pick their fast or IEEE sequence by a ballot over the lanes that run them;
// both sequences are correctly rounded, so the lanes a wave happens to hold (a partial last wave, entries that came in
// ended) change no bit of any lane's result.
#pragma once

struct CameraRaysParams {
    crt_camera_desc cam;
    int width, height;
    float rcp_w, rcp_h;
    int fast_uv;
    const int32_t* __restrict__ pixels;    // null: entry k is pixel k
    uint32_t n;
    uint32_t* __restrict__ rng;            // 6 words per pixel of the frame
    float4* __restrict__ rays;             // 2 rows per entry
    float4* __restrict__ paths;            // 2 rows per entry
};

__global__ __launch_bounds__(256) void crt_camera_rays_kernel(CameraRaysParams Q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= Q.n) return;
    const int pix = Q.pixels ? Q.pixels[i] : (int)i;
    const float INF = __builtin_inff();
    if ((uint32_t)pix >= (uint32_t)(Q.width * Q.height)) {   // not a pixel of the frame: nothing drawn, an ended path
        Q.rays[2 * (size_t)i] = make_float4(0.f, 0.f, 0.f, INF);
        Q.rays[2 * (size_t)i + 1] = make_float4(0.f, 0.f, 1.f, 0.f);
        Q.paths[2 * (size_t)i] = make_float4(0.f, 0.f, 0.f, __int_as_float(0));
        Q.paths[2 * (size_t)i + 1] = make_float4(__int_as_float(pix), __int_as_float(CRT_PATH_ENDED), 0.f, 0.f);
        return;
    }
    const CamRegs C = cam_regs(Q.cam, Q.width, Q.height, Q.rcp_w, Q.rcp_h, Q.fast_uv);
    uint32_t* r = Q.rng + 6 * (size_t)pix;
    PathState S = new_sample_state(rng_load(r));
    next_ray(S, C, pix % Q.width, pix / Q.width, 1);       // a new sample: the camera block alone
    rng_store(r, S.s);
    Q.rays[2 * (size_t)i] = make_float4(S.o.x, S.o.y, S.o.z, INF);
    Q.rays[2 * (size_t)i + 1] = make_float4(S.d.x, S.d.y, S.d.z, 0.f);
    Q.paths[2 * (size_t)i] = make_float4(1.f, 1.f, 1.f, __int_as_float(0));
    Q.paths[2 * (size_t)i + 1] = make_float4(__int_as_float(pix), __int_as_float(CRT_PATH_ACTIVE), 0.f, 0.f);
}

struct PathStepParams {
    float4* __restrict__ rays;             // 2 rows per entry, in place
    const float4* __restrict__ hits;       // 2 rows per entry
    float4* __restrict__ paths;            // 2 rows per entry, in place
    const float4* __restrict__ rows;       // per material: (code, 0, 0, 0) (payload)
    uint32_t* __restrict__ rng;            // 6 words per pixel
    float* __restrict__ linear;            // 3 floats per pixel
    uint32_t n, n_pix;
    int n_mats, max_bounces;
};

// One bounce of one path: what the render kernels do between two traces.  Everything goes in by value and comes
// back in one struct by value: with the state passed by reference both kernels below need 4 more VGPRs and the
// advance kernel loses a wave per SIMD (profiles/shared_scatter/kernels_unchanged.txt).
struct Scattered {
    Rng s;
    V3 o, d, thr;
    int bounce;
    bool ended;
    V3 add;                                // what an ended path adds to its pixel
};
__device__ __forceinline__ Scattered scatter_step(float4 h0, float4 h1, const float4* __restrict__ rows, int n_mats,
                                                  int max_bounces, Rng s, V3 o, V3 d, V3 thr, int bounce) {
    // ---- rayColor's loop body after the hit query: shade_rec() on the hit record
    constexpr uint32_t SHADE_MISS = 15;
    const float t = h0.x;
    const bool miss = t < 0;
    uint32_t code = SHADE_MISS;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!miss) {
        const uint32_t mat = __float_as_uint(h0.w);
        code = SHADE_INVALID;                                // CUDAKernels.h:127
        if (mat < (uint32_t)n_mats) {
            code = __float_as_uint(rows[2u * mat].x);
            m = rows[2u * mat + 1u];
        }
    }
    const V3 hp = o + t * d;                                 // Ray::pointAtDistance
    const V3 outward = v3(h1.x, h1.y, h1.z);
    const bool front = __float_as_int(h1.w) != 0;            // HitInfo::setFaceNormal, as the query stored it
    const V3 n = front ? outward : -outward;
    bool ended = false;
    V3 add = v3(0.0f, 0.0f, 0.0f);                           // what an ending path adds to its pixel
    V3 q = d;                                                // dielectric, sky (CRTUtility.cuh:35)
    if (code == SHADE_LAMBERT || code == SHADE_METAL) q = rand_in_unit_sphere(s);
    V3 uq = q;
    if (code <= SHADE_DIELECTRIC || miss) uq = unit(q);      // one normalisation for all four users, as shade_rec
    if (miss) {                                              // :137-142
        add = thr * sky_unit(uq);
        ended = true;
    } else if (code == SHADE_INVALID) {                      // :127 invalid material: same ray again
        ++bounce;
    } else if (code == SHADE_LAMBERT) {                      // Material.cuh:66-77
        V3 sd = n + uq;
        if (fabsf(sd.x) < 1e-8f && fabsf(sd.y) < 1e-8f && fabsf(sd.z) < 1e-8f) sd = n;
        thr = thr * v3(m.x, m.y, m.z);
        o = hp;
        d = sd;
        ++bounce;
    } else if (code == SHADE_METAL) {                        // :89-96
        V3 refl = reflect(d, n);
        refl = unit(refl) + (m.w * uq);
        if (dot(refl, n) > 0) {
            thr = thr * v3(m.x, m.y, m.z);
            o = hp;
            d = refl;
            ++bounce;
        } else {                                             // absorbed: return Material::emit() = 0
            ended = true;
        }
    } else if (code == SHADE_DIELECTRIC) {                   // :109-128
        const float ri = front ? m.y : m.x;
        const float r0 = front ? m.z : m.w;
        const V3 ud = uq;
        const float cos_theta = fminf(dot(-ud, n), 1.0f);
        const bool cannot_refract = cannot_refract_exact(cos_theta, ri);
        V3 dir;
        if (cannot_refract || schlick_r0(cos_theta, r0) > uniform(s))
            dir = reflect(ud, n);
        else
            dir = refract(ud, n, ri);
        o = hp;
        d = dir;
        ++bounce;
    } else {                                                 // DiffuseLight: return emit() raw; unknown type: 0
        if (code == SHADE_LIGHT) add = v3(m.x, m.y, m.z);
        ended = true;
    }

    // ---- the next iteration's head (CUDAKernels.h:110-121), next_ray()'s first block
    if (!ended) {
        if (bounce >= max_bounces) {                       // loop exhausted: final_color = 0
            ended = true;
        } else if (bounce >= 3) {
            float p = fmaxf(thr.x, fmaxf(thr.y, thr.z));
            p = fminf(p, 0.95f);
            if (uniform(s) > p) ended = true;
            else thr = recip_exact_wave(p) * thr;            // 1 / p, exact (crt_device.h)
        }
    }
    return Scattered{s, o, d, thr, bounce, ended, add};
}

__global__ __launch_bounds__(256) void crt_path_step_kernel(PathStepParams Q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= Q.n) return;
    const float4 p0 = Q.paths[2 * (size_t)i], p1 = Q.paths[2 * (size_t)i + 1];
    const uint32_t pix = __float_as_uint(p1.x);
    if (__float_as_int(p1.y) != CRT_PATH_ACTIVE || pix >= Q.n_pix) return;
    const float4 ray0 = Q.rays[2 * (size_t)i], ray1 = Q.rays[2 * (size_t)i + 1];
    const float4 h0 = Q.hits[2 * (size_t)i], h1 = Q.hits[2 * (size_t)i + 1];
    uint32_t* rp = Q.rng + 6 * (size_t)pix;
    const float INF = __builtin_inff();
    const Scattered r = scatter_step(h0, h1, Q.rows, Q.n_mats, Q.max_bounces, rng_load(rp), v3(ray0.x, ray0.y, ray0.z),
                                     v3(ray1.x, ray1.y, ray1.z), v3(p0.x, p0.y, p0.z), __float_as_int(p0.w));
    rng_store(rp, r.s);
    if (r.ended) {
        float* L = Q.linear + 3 * (size_t)pix;
        const V3 sum = v3(L[0], L[1], L[2]) + r.add;         // pixel_color += ..., the (0, 0, 0) of a killed path too
        L[0] = sum.x; L[1] = sum.y; L[2] = sum.z;
    } else {
        Q.rays[2 * (size_t)i] = make_float4(r.o.x, r.o.y, r.o.z, INF);
        Q.rays[2 * (size_t)i + 1] = make_float4(r.d.x, r.d.y, r.d.z, 0.f);
    }
    Q.paths[2 * (size_t)i] = make_float4(r.thr.x, r.thr.y, r.thr.z, __int_as_float(r.bounce));
    Q.paths[2 * (size_t)i + 1] = make_float4(p1.x, __int_as_float(r.ended ? CRT_PATH_ENDED : CRT_PATH_ACTIVE), p1.z, p1.w);
}

// ------------------------------------------------------------------ step, regenerate, compact
// crt_path_advance_kernel   one lane per entry of a read-only input batch: scatter_step(), the function
//                           crt_path_step_kernel calls, then the entry's fate in the same lane.  A path that goes on
//                           is appended to the output batch.  One that ended adds its contribution to its pixel's sum
//                           and, while remaining[pixel] > 0, takes one of the pixel's samples and draws its camera ray
//                           with next_ray()'s camera block on the RNG state the lane already holds: one load and one
//                           store of the state per entry.  Entries that came in ended or name no pixel of the frame
//                           draw, add and append nothing.
//
// Compaction: the lanes that append are counted with a wave ballot, a lane's place among them is the popcount of the
// ballot below it, and output slots are reserved with atomicAdd on one device counter, CRT_ADVANCE_ENTRIES input
// entries per reservation: 64 = one reservation per wave (no LDS), 256 = one per workgroup, 512 / 768 / 1024 = one per
// workgroup that loops over 2 / 3 / 4 chunks of 256 entries and holds their results in registers until the base is
// known.  The order of the output across reservations is whatever order the atomics ran in; no result depends on it.
// 512 is the measured choice (profiles/wavefront/reservation_sweep.txt: the frame's 128 advance calls take 11.0 ms at
// 64, 4.65 ms at 256, 4.05 ms at 512 and 4.16 ms at 1024, where 87 VGPRs leave 5 waves per SIMD).
#ifndef CRT_ADVANCE_ENTRIES
#define CRT_ADVANCE_ENTRIES 512
#endif
constexpr int ADV_ENTRIES = CRT_ADVANCE_ENTRIES;
static_assert(ADV_ENTRIES == 64 || (ADV_ENTRIES % 256 == 0 && ADV_ENTRIES >= 256 && ADV_ENTRIES <= 1024),
              "entries per reservation: a wave, or 1 to 4 chunks of a 256-lane workgroup");
constexpr int ADV_CHUNKS = ADV_ENTRIES == 64 ? 1 : ADV_ENTRIES / 256;   // chunks of 256 entries per workgroup
constexpr bool ADV_PER_WAVE = ADV_ENTRIES == 64;

struct PathAdvanceParams {
    const float4* __restrict__ rays;       // 2 rows per entry, read only
    const float4* __restrict__ hits;
    const float4* __restrict__ paths;
    const float4* __restrict__ rows;       // per material: (code, 0, 0, 0) (payload)
    uint32_t* __restrict__ rng;            // 6 words per pixel
    float* __restrict__ linear;            // 3 floats per pixel
    int32_t* __restrict__ remaining;       // per pixel: samples not yet started; null: never regenerate
    float4* __restrict__ rays_out;         // n entries
    float4* __restrict__ paths_out;
    uint32_t* __restrict__ count;          // entries appended; zeroed on the stream before the launch
    uint32_t n, n_pix;
    int n_mats, max_bounces;
    crt_camera_desc cam;
    int width, height;
    float rcp_w, rcp_h;
    int fast_uv;
};

// What a lane appends: the four rows of its entry.
struct AdvanceRows {
    float4 r0, r1, p0, p1;
};

// One entry: true when `out` is to be appended.
__device__ __forceinline__ bool advance_entry(const PathAdvanceParams& Q, uint32_t i, AdvanceRows& out) {
    const float4 p0 = Q.paths[2 * (size_t)i], p1 = Q.paths[2 * (size_t)i + 1];
    const uint32_t pix = __float_as_uint(p1.x);
    if (__float_as_int(p1.y) != CRT_PATH_ACTIVE || pix >= Q.n_pix) return false;
    const float4 ray0 = Q.rays[2 * (size_t)i], ray1 = Q.rays[2 * (size_t)i + 1];
    const float4 h0 = Q.hits[2 * (size_t)i], h1 = Q.hits[2 * (size_t)i + 1];
    uint32_t* rp = Q.rng + 6 * (size_t)pix;
    const float INF = __builtin_inff();
    const Scattered r = scatter_step(h0, h1, Q.rows, Q.n_mats, Q.max_bounces, rng_load(rp), v3(ray0.x, ray0.y, ray0.z),
                                     v3(ray1.x, ray1.y, ray1.z), v3(p0.x, p0.y, p0.z), __float_as_int(p0.w));
    Rng s = r.s;
    V3 o = r.o, d = r.d, thr = r.thr;
    int bounce = r.bounce;

    // ---- the entry's fate
    bool keep = !r.ended;
    float4 q1 = make_float4(p1.x, __int_as_float(CRT_PATH_ACTIVE), p1.z, p1.w);
    if (r.ended) {
        float* L = Q.linear + 3 * (size_t)pix;
        const V3 sum = v3(L[0], L[1], L[2]) + r.add;         // pixel_color += ..., the (0, 0, 0) of a killed path too
        L[0] = sum.x; L[1] = sum.y; L[2] = sum.z;
        int32_t left = 0;
        if (Q.remaining) left = Q.remaining[pix];
        if (left > 0) {                                      // the pixel's next sample, as crt_camera_rays_kernel draws it
            Q.remaining[pix] = left - 1;
            const CamRegs C = cam_regs(Q.cam, Q.width, Q.height, Q.rcp_w, Q.rcp_h, Q.fast_uv);
            PathState S = new_sample_state(s);
            next_ray(S, C, (int)(pix % (uint32_t)Q.width), (int)(pix / (uint32_t)Q.width), 1);
            s = S.s;
            o = S.o;
            d = S.d;
            thr = v3(1.f, 1.f, 1.f);
            bounce = 0;
            q1 = make_float4(p1.x, __int_as_float(CRT_PATH_ACTIVE), 0.f, 0.f);
            keep = true;
        }
    }
    rng_store(rp, s);
    out.r0 = make_float4(o.x, o.y, o.z, INF);
    out.r1 = make_float4(d.x, d.y, d.z, 0.f);
    out.p0 = make_float4(thr.x, thr.y, thr.z, __int_as_float(bounce));
    out.p1 = q1;
    return keep;
}

__device__ __forceinline__ void advance_store(const PathAdvanceParams& Q, uint32_t slot, const AdvanceRows& out) {
    if (slot >= Q.n) return;                                 // cannot happen with a counter that started at 0
    Q.rays_out[2 * (size_t)slot] = out.r0;
    Q.rays_out[2 * (size_t)slot + 1] = out.r1;
    Q.paths_out[2 * (size_t)slot] = out.p0;
    Q.paths_out[2 * (size_t)slot + 1] = out.p1;
}

__global__ __launch_bounds__(256) void crt_path_advance_kernel(PathAdvanceParams Q) {
#define ADVANCE_BODY_N Q.n
#include "crt_path_advance_body.inc"
#undef ADVANCE_BODY_N
}

// The indirect form: the number of input entries is a device word the kernel reads when it runs, clamped
// to the capacity the host sized the grid and the arrays by (Q.n).  Workgroups beyond the count do nothing.
struct PathAdvanceIndirectParams {
    PathAdvanceParams Q;                   // n: the capacity
    const uint32_t* __restrict__ d_n;      // the entry count, on the device
    unsigned long long* __restrict__ totals;   // null, or [0] += the clamped count, [1] += 1 if it is not 0
};

__global__ __launch_bounds__(256) void crt_path_advance_indirect_kernel(PathAdvanceIndirectParams I) {
    const PathAdvanceParams& Q = I.Q;
    const uint32_t n = min(*I.d_n, Q.n);
    if (I.totals && blockIdx.x == 0 && threadIdx.x == 0) {   // kernels of one stream are ordered: one lane, plain adds
        I.totals[0] += n;
        I.totals[1] += n ? 1u : 0u;
    }
    if (blockIdx.x * (256u * (uint32_t)ADV_CHUNKS) >= n) return;
#define ADVANCE_BODY_N n
#include "crt_path_advance_body.inc"
#undef ADVANCE_BODY_N
}

// ------------------------------------------------------------------ finish
// crt_path_finish_kernel    one lane per entry of a read-only input batch (rays, paths; no hits): the lane runs its
//                           pixel's trace / advance rounds to the end by itself.  It loads the RNG state, the pixel's sum
//                           and remaining[pixel] once, then per ray: the lane kernels' trace (trace4, or trace<> on the
//                           ray's layout), the hit record by trace_store's rule in registers, scatter_step(), and on an
//                           end the sum's addition and, while samples are left, next_ray()'s camera block on the state
//                           it holds, exactly advance_entry()'s.  Three stores at the end: the state, the sum, 0 samples
//                           left.  Every iteration increments the bounce or ends the path, and an ended path takes one
//                           of the pixel's samples or leaves: at most (remaining + 1) * max_bounces rays per lane.
//
// One wave per workgroup: the batches this is for are a few thousand entries, which so spread over the CUs, and the
// kernel's time is its longest lane's chain of traces.  The entry count is Q.n, or min(*Q.d_n, Q.n) with *Q.d_n read
// here (§18's rule).  Entries that come in ended, name no pixel of the frame or lie at or beyond the count read and
// write nothing.  The functions that pick a fast or an IEEE sequence by ballot are correctly rounded either way, so the
// divergent loop changes no bit (see the head of this file).
struct PathFinishParams {
    const float4* __restrict__ rays;       // 2 rows per entry, read only
    const float4* __restrict__ paths;
    const float4* __restrict__ nodes;      // the scene, as TraceParams carries it
    const float4* __restrict__ prims;
    const float4* __restrict__ chain;
    const float4* __restrict__ shade;
    const int4* __restrict__ ident;
    const float4* __restrict__ rows;       // per material: (code, 0, 0, 0) (payload)
    int n_nodes, n_layouts, n_chain, sphere_first, n_ray_spheres;
    int scene_width;                       // 2 = threaded nodes (trace<>), 4 = 4-wide nodes (trace4)
    uint32_t* __restrict__ rng;            // 6 words per pixel
    float* __restrict__ linear;            // 3 floats per pixel
    int32_t* __restrict__ remaining;       // per pixel: samples not yet started; null: never regenerate
    const uint32_t* __restrict__ d_n;      // null, or the entry count on the device
    unsigned long long* __restrict__ totals;   // null, or [0] += rays traced, [1] += 1 if the count is not 0
    uint32_t n, n_pix;                     // n: the entries, or their capacity with d_n
    int n_mats, max_bounces;
    crt_camera_desc cam;
    int width, height;
    float rcp_w, rcp_h;
    int fast_uv;
};

__global__ __launch_bounds__(64) void crt_path_finish_kernel(PathFinishParams Q) {
    const uint32_t n = Q.d_n ? min(*Q.d_n, Q.n) : Q.n;
    if (blockIdx.x * 64u >= n) return;                       // the whole wave: the lanes below stay together for the sum
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const float INF = __builtin_inff();
    uint64_t traced = 0;
    float4 p1 = make_float4(0.f, __int_as_float(CRT_PATH_ENDED), 0.f, 0.f);
    if (i < n) p1 = Q.paths[2 * (size_t)i + 1];
    const uint32_t pix = __float_as_uint(p1.x);
    if (i < n && __float_as_int(p1.y) == CRT_PATH_ACTIVE && pix < Q.n_pix) {
        const float4 p0 = Q.paths[2 * (size_t)i];
        const float4 ray0 = Q.rays[2 * (size_t)i], ray1 = Q.rays[2 * (size_t)i + 1];
        uint32_t* rp = Q.rng + 6 * (size_t)pix;
        float* L = Q.linear + 3 * (size_t)pix;
        Rng s = rng_load(rp);
        V3 sum = v3(L[0], L[1], L[2]);
        int32_t left = Q.remaining ? Q.remaining[pix] : 0;
        V3 o = v3(ray0.x, ray0.y, ray0.z), d = v3(ray1.x, ray1.y, ray1.z), thr = v3(p0.x, p0.y, p0.z);
        int bounce = __float_as_int(p0.w);
        float tmax = ray0.w;                                 // the entry's first ray keeps its row's; +inf afterwards
        for (;;) {
            // ---- the lane kernels' trace (crt_trace_lane_body.inc)
            float t;
            TraceCounts cnt{};
            const int hit = Q.scene_width == 4 ? trace4(Q.nodes, Q.prims, Q.chain, Q.n_chain, Q.sphere_first,
                                                        Q.n_ray_spheres, o, d, t)
                                               : trace<false>(Q.nodes, Q.prims, Q.n_nodes,
                                                              layout_base(d, Q.n_layouts, Q.n_nodes), o, d, t, cnt);
            ++traced;
            // ---- its record, by trace_store()'s rule
            float4 h0 = make_float4(-1.f, 0.f, 0.f, 0.f), h1 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (hit >= 0 && t <= tmax) {
                const int4 id = Q.ident[hit];
                const float4* R = Q.shade + 3u * (uint32_t)hit;
                const float4 r0 = R[0];
                V3 nrm = v3(r0.x, r0.y, r0.z);
                if (__float_as_uint(r0.w) & SHADE_SPHERE) {
                    const float ir = R[2].x;
                    const V3 hp = o + t * d;                 // Ray::pointAtDistance
                    nrm = ir * (hp - nrm);
                }
                const bool front = dot(d, nrm) < 0;          // HitInfo::setFaceNormal
                h0 = make_float4(t, __int_as_float(id.x), __int_as_float(id.y), __int_as_float(id.z));
                h1 = make_float4(nrm.x, nrm.y, nrm.z, __int_as_float(front ? 1 : 0));
            }
            tmax = INF;
            const Scattered r = scatter_step(h0, h1, Q.rows, Q.n_mats, Q.max_bounces, s, o, d, thr, bounce);
            s = r.s;
            o = r.o; d = r.d; thr = r.thr;
            bounce = r.bounce;
            if (r.ended) {                                   // ---- the entry's fate, as advance_entry()
                sum = sum + r.add;                           // pixel_color += ..., the (0, 0, 0) of a killed path too
                if (left <= 0) break;
                --left;                                      // the pixel's next sample, as crt_camera_rays_kernel draws it
                const CamRegs C = cam_regs(Q.cam, Q.width, Q.height, Q.rcp_w, Q.rcp_h, Q.fast_uv);
                PathState S = new_sample_state(s);
                next_ray(S, C, (int)(pix % (uint32_t)Q.width), (int)(pix / (uint32_t)Q.width), 1);
                s = S.s;
                o = S.o;
                d = S.d;
                thr = v3(1.f, 1.f, 1.f);
                bounce = 0;
            }
        }
        rng_store(rp, s);
        L[0] = sum.x; L[1] = sum.y; L[2] = sum.z;
        if (Q.remaining) Q.remaining[pix] = 0;
    }
    if (Q.totals) {
        const uint64_t rays = wave_sum_u64(traced);
        if (threadIdx.x == 0) {
            if (rays) atomicAdd(&Q.totals[0], (unsigned long long)rays);
            if (blockIdx.x == 0) atomicAdd(&Q.totals[1], 1ull);   // n != 0: this workgroup did not leave above
        }
    }
}

// ------------------------------------------------------------------ host side
namespace {

// The argument checks both device entries share; they come before any device use.
int path_batch_args(const char* what, int64_t n, const void* a, const void* b, const void* c) {
    if (n < 0 || n >= ((int64_t)1 << 31))
        return set_error(CRT_ERR_INVALID_ARGUMENT, std::string(what) + ": n must be in [0, 2^31)");
    if (n == 0) return CRT_OK;
    if (!a || !b || !c) return set_error(CRT_ERR_INVALID_ARGUMENT, std::string(what) + ": null array");
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u)
        return set_error(CRT_ERR_INVALID_ARGUMENT, std::string(what) + ": ray, hit and path arrays must be 16-byte aligned");
    return CRT_OK;
}

// The advance entries: the argument checks, the count's reset and the launch.  d_n null: entries [0, n).  Otherwise the
// indirect call: n is the capacity, the kernel advances entries [0, min(*d_n, n)) and adds to d_totals (optional).
int advance_enqueue(const std::string& what, const crt_scene* S, crt_renderer* R, const crt_ray* d_rays,
                    const crt_hit* d_hits, const crt_path* d_paths, const uint32_t* d_n, int64_t n, int max_bounces,
                    uint32_t* d_rng, float* d_linear, int32_t* d_remaining, crt_ray* d_rays_out, crt_path* d_paths_out,
                    uint32_t* d_count, uint64_t* d_totals, void* stream) {
    if (!S) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": null scene");
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": null renderer");
    if (int rc = path_batch_args(what.c_str(), n, d_rays, d_hits, d_paths)) return rc;
    if (max_bounces < 1) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": max_bounces must be >= 1");
    if (!d_count) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": null count");
    if (d_n && d_n == d_count)
        return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": the output count overlaps the input count");
    if (n > 0) {
        if (!d_rays_out || !d_paths_out) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": null output array");
        if (((uintptr_t)d_rays_out | (uintptr_t)d_paths_out) & 15u)
            return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": output arrays must be 16-byte aligned");
        const uintptr_t bytes = (uintptr_t)n * 32u;          // every batch array holds n 32-B entries
        const uintptr_t in[3] = {(uintptr_t)d_rays, (uintptr_t)d_hits, (uintptr_t)d_paths};
        const uintptr_t out[2] = {(uintptr_t)d_rays_out, (uintptr_t)d_paths_out};
        for (uintptr_t a : out)
            for (uintptr_t b : in)
                if (a < b + bytes && b < a + bytes)
                    return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": an output array overlaps an input array");
        if (out[0] < out[1] + bytes && out[1] < out[0] + bytes)
            return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": the output arrays overlap");
    }
    if (((uintptr_t)d_rng | (uintptr_t)d_linear | (uintptr_t)d_remaining | (uintptr_t)d_count | (uintptr_t)d_n) & 3u)
        return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": RNG state, sums, remaining and counts must be 4-byte aligned");
    if ((uintptr_t)d_totals & 7u) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": totals must be 8-byte aligned");
    if (S->device != R->device) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": scene and renderer on different devices");
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": the renderer has no camera (crt_renderer_set_camera)");
    HIP_TRY(hipSetDevice(S->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_count, 0, 4, st));
    if (n == 0) return CRT_OK;
    PathAdvanceParams Q{};
    Q.rays = reinterpret_cast<const float4*>(d_rays);
    Q.hits = reinterpret_cast<const float4*>(d_hits);
    Q.paths = reinterpret_cast<const float4*>(d_paths);
    Q.rows = S->d_mat_rows.get();
    Q.rng = d_rng ? d_rng : R->d_rng.get();
    Q.linear = d_linear ? d_linear : R->d_sum;
    Q.remaining = d_remaining;
    Q.rays_out = reinterpret_cast<float4*>(d_rays_out);
    Q.paths_out = reinterpret_cast<float4*>(d_paths_out);
    Q.count = d_count;
    Q.n = (uint32_t)n;
    Q.n_pix = (uint32_t)(R->width * R->height);
    Q.n_mats = S->n_mats;
    Q.max_bounces = max_bounces;
    set_camera_frame(Q, R);
    const int64_t per_group = 256 * (int64_t)ADV_CHUNKS;
    const dim3 grid((unsigned)((n + per_group - 1) / per_group));
    if (d_n) {
        const PathAdvanceIndirectParams I{Q, d_n, reinterpret_cast<unsigned long long*>(d_totals)};
        hipLaunchKernelGGL(crt_path_advance_indirect_kernel, grid, dim3(256), 0, st, I);
    } else {
        hipLaunchKernelGGL(crt_path_advance_kernel, grid, dim3(256), 0, st, Q);
    }
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

// trace_enqueue's lane_ok: trace4's per-lane stack takes up to three entries per branching ancestor and drops what does
// not fit without a report, so a 4-wide tree whose bound could overflow it never goes through the finish kernel.
bool finish_lane_ok(const crt_scene* S) { return S->width != 4 || 3 * (int64_t)S->stack_bound <= TRACE4_STACK; }

}  // namespace

extern "C" {

int crt_renderer_camera_rays_device(crt_renderer* R, const int32_t* d_pixels, int64_t n, uint32_t* d_rng,
                                    crt_ray* d_rays, crt_path* d_paths, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "camera rays: null renderer");
    if (int rc = path_batch_args("camera rays", n, d_rays, d_paths, d_rays)) return rc;
    if (n == 0) return CRT_OK;
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, "camera rays: the renderer has no camera (crt_renderer_set_camera)");
    if (((uintptr_t)d_pixels | (uintptr_t)d_rng) & 3u)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "camera rays: pixel and RNG arrays must be 4-byte aligned");
    HIP_TRY(hipSetDevice(R->device));
    CameraRaysParams Q{};
    set_camera_frame(Q, R);
    Q.pixels = d_pixels;
    Q.n = (uint32_t)n;
    Q.rng = d_rng ? d_rng : R->d_rng.get();
    Q.rays = reinterpret_cast<float4*>(d_rays);
    Q.paths = reinterpret_cast<float4*>(d_paths);
    hipLaunchKernelGGL(crt_camera_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

int crt_scene_path_step_device(const crt_scene* S, crt_ray* d_rays, const crt_hit* d_hits, crt_path* d_paths, int64_t n,
                               int max_bounces, uint32_t* d_rng, float* d_linear, int64_t n_pixels, void* stream) {
    if (!S) return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: null scene");
    if (int rc = path_batch_args("path step", n, d_rays, d_hits, d_paths)) return rc;
    if (max_bounces < 1) return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: max_bounces must be >= 1");
    if (n_pixels < 0 || n_pixels > ((int64_t)1 << 31) / 6)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: n_pixels must be in [0, 2^31 / 6]");
    if (n == 0) return CRT_OK;
    if (!d_rng || !d_linear) return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: null RNG state or sums");
    if (((uintptr_t)d_rng | (uintptr_t)d_linear) & 3u)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: RNG state and sums must be 4-byte aligned");
    HIP_TRY(hipSetDevice(S->device));
    PathStepParams Q{};
    Q.rays = reinterpret_cast<float4*>(d_rays);
    Q.hits = reinterpret_cast<const float4*>(d_hits);
    Q.paths = reinterpret_cast<float4*>(d_paths);
    Q.rows = S->d_mat_rows.get();
    Q.rng = d_rng;
    Q.linear = d_linear;
    Q.n = (uint32_t)n;
    Q.n_pix = (uint32_t)n_pixels;
    Q.n_mats = S->n_mats;
    Q.max_bounces = max_bounces;
    hipLaunchKernelGGL(crt_path_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

int crt_scene_path_advance_device(const crt_scene* S, crt_renderer* R, const crt_ray* d_rays, const crt_hit* d_hits,
                                  const crt_path* d_paths, int64_t n, int max_bounces, uint32_t* d_rng, float* d_linear,
                                  int32_t* d_remaining, crt_ray* d_rays_out, crt_path* d_paths_out, uint32_t* d_count,
                                  void* stream) {
    return advance_enqueue("path advance", S, R, d_rays, d_hits, d_paths, nullptr, n, max_bounces, d_rng, d_linear,
                           d_remaining, d_rays_out, d_paths_out, d_count, nullptr, stream);
}

int crt_scene_path_advance_indirect_device(const crt_scene* S, crt_renderer* R, const crt_ray* d_rays, const crt_hit* d_hits,
                                           const crt_path* d_paths, const uint32_t* d_n, int64_t capacity, int max_bounces,
                                           uint32_t* d_rng, float* d_linear, int32_t* d_remaining, crt_ray* d_rays_out,
                                           crt_path* d_paths_out, uint32_t* d_count, uint64_t* d_totals, void* stream) {
    if (!d_n) return set_error(CRT_ERR_INVALID_ARGUMENT, "indirect path advance: null input count");
    return advance_enqueue("indirect path advance", S, R, d_rays, d_hits, d_paths, d_n, capacity, max_bounces, d_rng,
                           d_linear, d_remaining, d_rays_out, d_paths_out, d_count, d_totals, stream);
}

int crt_path_advance_entries(void) { return ADV_ENTRIES; }

int crt_scene_path_finish_device(const crt_scene* S, crt_renderer* R, const crt_ray* d_rays, const crt_path* d_paths,
                                 const uint32_t* d_n, int64_t capacity, int max_bounces, uint32_t* d_rng, float* d_linear,
                                 int32_t* d_remaining, uint64_t* d_totals, void* stream) {
    const std::string what = "path finish";
    if (!S) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": null scene");
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": null renderer");
    if (int rc = path_batch_args(what.c_str(), capacity, d_rays, d_paths, d_rays)) return rc;
    if (max_bounces < 1) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": max_bounces must be >= 1");
    if (((uintptr_t)d_rng | (uintptr_t)d_linear | (uintptr_t)d_remaining | (uintptr_t)d_n) & 3u)
        return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": RNG state, sums, remaining and the count must be 4-byte aligned");
    if ((uintptr_t)d_totals & 7u) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": totals must be 8-byte aligned");
    if (S->device != R->device) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": scene and renderer on different devices");
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, what + ": the renderer has no camera (crt_renderer_set_camera)");
    if (!finish_lane_ok(S))
        return set_error(CRT_ERR_UNSUPPORTED, what + ": the tree's stack bound exceeds the in-lane traversal's 64-entry "
                                              "stack (3 entries per level)");
    if (capacity == 0) return CRT_OK;
    HIP_TRY(hipSetDevice(S->device));
    PathFinishParams Q{};
    Q.rays = reinterpret_cast<const float4*>(d_rays);
    Q.paths = reinterpret_cast<const float4*>(d_paths);
    Q.nodes = S->d_nodes.get(); Q.prims = S->d_prims.get(); Q.chain = S->d_chain.get(); Q.shade = S->d_shade.get();
    Q.ident = S->d_ident.get();
    Q.rows = S->d_mat_rows.get();
    Q.n_nodes = S->n_nodes; Q.n_layouts = S->layouts; Q.n_chain = S->n_chain;
    Q.sphere_first = S->sphere_first; Q.n_ray_spheres = S->n_ray_spheres;
    Q.scene_width = S->width;
    Q.rng = d_rng ? d_rng : R->d_rng.get();
    Q.linear = d_linear ? d_linear : R->d_sum;
    Q.remaining = d_remaining;
    Q.d_n = d_n;
    Q.totals = reinterpret_cast<unsigned long long*>(d_totals);
    Q.n = (uint32_t)capacity;
    Q.n_pix = (uint32_t)(R->width * R->height);
    Q.n_mats = S->n_mats;
    Q.max_bounces = max_bounces;
    set_camera_frame(Q, R);
    hipLaunchKernelGGL(crt_path_finish_kernel, dim3((unsigned)((capacity + 63) / 64)), dim3(64), 0, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

}  // extern "C"

constexpr int QUEUE_WORDS = 8, QUEUE_ERR = 2, QUEUE_TOTALS = 4;   // WavefrontScratch::d_queue
// crt_renderer_render_wavefront_queued's sync_every = 0: iterations enqueued between two host waits
// (profiles/indirect/path_bench.jsonl)
constexpr int QUEUE_SYNC_EVERY = 32;
// crt_renderer_render_wavefront_finish's finish_below = -1: batches of at most this many entries go to the finish kernel.
// The fastest setting of the sweep (profiles/finish/path_bench.jsonl): the 921,600 pixels of its
// 1280x720 frame, the whole frame through the finish kernel (15.5 ms against 27.5 ms at 0).  Larger frames were not measured.
constexpr int64_t QUEUE_FINISH_BELOW = 921600;

namespace {

int wavefront_scratch(crt_renderer* R, WavefrontScratch** out) {
    return first_use(R->wavefront, "the wavefront scratch of this renderer could not be allocated", out, [&](WavefrontScratch* X) -> int {
        const size_t n_pix = (size_t)R->width * R->height;
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(X->rays[k].alloc(n_pix));
            HIP_TRY(X->paths[k].alloc(n_pix));
        }
        HIP_TRY(X->hits.alloc(n_pix));
        HIP_TRY(X->remaining.alloc(n_pix));
        HIP_TRY(X->d_count.alloc(1));
        HIP_TRY(X->h_count.alloc(4));
        HIP_TRY(X->d_queue.alloc(QUEUE_WORDS));
        HIP_TRY(X->h_queue.alloc(QUEUE_WORDS));
        HIP_TRY(X->ev0.create());
        HIP_TRY(X->ev1.create());
        return CRT_OK;
    });
}

// What the two wavefront loops check of their arguments, in one order.  queued: the loop of
// crt_renderer_render_wavefront_queued and _finish, which also checks sync_every, its pixel limit and finish_below.
int wavefront_check(const crt_renderer* R, const crt_scene* Sc, int spp, int max_bounces, unsigned flags, bool queued,
                    int sync_every, int64_t finish_below) {
    if (!R || !Sc) return set_error(CRT_ERR_INVALID_ARGUMENT, "render wavefront: null argument");
    if (spp < 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "render wavefront: negative spp");
    if (max_bounces < 1) return set_error(CRT_ERR_INVALID_ARGUMENT, "render wavefront: max_bounces must be >= 1");
    if (queued && sync_every < 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "render wavefront: sync_every must be >= 0");
    if (flags & ~(CRT_RENDER_ACCUMULATE | CRT_RENDER_COUNT_WORK))
        return set_error(CRT_ERR_INVALID_ARGUMENT, "render wavefront: unknown flag");
    if (Sc->device != R->device) return set_error(CRT_ERR_INVALID_ARGUMENT, "render wavefront: scene and renderer on different devices");
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, "render wavefront: camera not set");
    if (flags & CRT_RENDER_COUNT_WORK)
        return set_error(CRT_ERR_UNSUPPORTED, "render wavefront: work counters are the render kernels' (crt_renderer_render)");
    if (R->tile_shards > 1) return set_error(CRT_ERR_UNSUPPORTED, "render wavefront: pixel sharding is crt_renderer_render's");
    const int64_t n_pix = (int64_t)R->width * R->height;
    if (n_pix >= ((int64_t)1 << 31)) return set_error(CRT_ERR_UNSUPPORTED, "render wavefront: 2^31 pixels or more");
    if (!queued) return CRT_OK;
    if (n_pix > TRACE_LAUNCH_RAYS) return set_error(CRT_ERR_UNSUPPORTED, "render wavefront: the queued loop takes at most 2^30 pixels");
    if (finish_below > 0 && !finish_lane_ok(Sc))
        return set_error(CRT_ERR_UNSUPPORTED, "render wavefront: finish_below needs a tree whose stack bound fits the "
                                              "in-lane traversal's 64-entry stack (3 entries per level)");
    return CRT_OK;
}

// The start of a frame of either loop, on `stream`: the sums cleared unless the frame accumulates, the handle's scratch,
// every pixel's remaining samples, the queued loop's device words, ev0 and the camera rays into batch 0.  A frame of no
// sample or no pixel is done here: the stream is waited for, the stats are zero and *out stays null.
int wavefront_begin(crt_renderer* R, int spp, unsigned flags, bool queued, crt_wavefront_stats* stats_out, void* stream,
                    WavefrontScratch** out) {
    const int64_t n_pix = (int64_t)R->width * R->height;
    HIP_TRY(hipSetDevice(R->device));
    hipStream_t st = (hipStream_t)stream;
    if (!(flags & CRT_RENDER_ACCUMULATE))
        HIP_TRY(hipMemsetAsync(R->d_sum, 0, (size_t)n_pix * 3 * sizeof(float), st));
    if (spp == 0 || n_pix == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        if (stats_out) *stats_out = crt_wavefront_stats{};
        return CRT_OK;
    }
    WavefrontScratch* X = nullptr;
    if (int rc = wavefront_scratch(R, &X)) return rc;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)X->remaining.get(), spp - 1, (size_t)n_pix, st));
    if (queued) {   // the error word and the totals are cleared once per call; the first batch is every pixel
        uint32_t* const d_queue = X->d_queue.get();
        HIP_TRY(hipMemsetAsync(d_queue, 0, QUEUE_WORDS * 4, st));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_queue, (int)n_pix, 1, st));
    }
    HIP_TRY(hipEventRecord(X->ev0.get(), st));
    if (int rc = crt_renderer_camera_rays_device(R, nullptr, n_pix, nullptr, X->rays[0].get(), X->paths[0].get(), stream))
        return rc;
    *out = X;
    return CRT_OK;
}

// The end of a frame of either loop: ev1, the elapsed time and the stats.  `word`: the trace error word the loop read; a
// non-zero one goes into the handle's own word, for trace_take_error's report.
int wavefront_end(crt_scene* S, WavefrontScratch* X, hipStream_t st, crt_wavefront_stats stats, unsigned long long word,
                  crt_wavefront_stats* stats_out) {
    HIP_TRY(hipEventRecord(X->ev1.get(), st));
    HIP_TRY(hipEventSynchronize(X->ev1.get()));
    HIP_TRY(hipEventElapsedTime(&stats.ms, X->ev0.get(), X->ev1.get()));
    if (stats_out) *stats_out = stats;
    if (word) HIP_TRY(hipMemcpy(S->trace->d_stats.get() + TRACE_ERR_WORD, &word, 8, hipMemcpyHostToDevice));
    // a frame handed over before its first round ran no query: a scene that was never traced has no scratch to ask
    return S->trace ? trace_take_error(S->trace.get()) : CRT_OK;
}

}  // namespace

extern "C" {

int crt_renderer_render_wavefront(crt_renderer* R, const crt_scene* Sc, int spp, int max_bounces, unsigned flags,
                                  const crt_trace_options* trace_opts, crt_wavefront_stats* stats_out, void* stream) {
    if (int rc = wavefront_check(R, Sc, spp, max_bounces, flags, false, 0, 0)) return rc;
    crt_scene* S = const_cast<crt_scene*>(Sc);   // the trace scratch belongs to the handle (handles are not thread-safe)
    hipStream_t st = (hipStream_t)stream;
    WavefrontScratch* X = nullptr;
    if (int rc = wavefront_begin(R, spp, flags, false, stats_out, stream, &X)) return rc;
    if (!X) return CRT_OK;
    const int64_t n_pix = (int64_t)R->width * R->height;
    uint32_t* const h_count = X->h_count.get();
    crt_wavefront_stats stats{};
    int cur = 0;
    int64_t m = n_pix;
    while (m > 0) {
        stats.rays += (uint64_t)m;
        ++stats.iterations;
        if (int rc = trace_enqueue(S, X->rays[cur].get(), m, trace_opts, X->hits.get(), nullptr, 0, st)) return rc;
        if (int rc = crt_scene_path_advance_device(S, R, X->rays[cur].get(), X->hits.get(), X->paths[cur].get(), m,
                                                   max_bounces, nullptr, nullptr, X->remaining.get(),
                                                   X->rays[cur ^ 1].get(), X->paths[cur ^ 1].get(), X->d_count.get(),
                                                   stream))
            return rc;
        // the size of the next batch and this query's error word (the next query clears it), then the loop's one host wait
        HIP_TRY(hipMemcpyAsync(h_count, X->d_count.get(), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_count + 2, S->trace->d_stats.get() + TRACE_ERR_WORD, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        m = std::min<int64_t>(h_count[0], n_pix);
        cur ^= 1;
        if (h_count[2] | h_count[3]) break;                  // reported by wavefront_end, as trace_take_error words it
    }
    unsigned long long word;
    std::memcpy(&word, h_count + 2, sizeof word);
    return wavefront_end(S, X, st, stats, word, stats_out);
}

}  // extern "C"

namespace {

// The queued loop (crt_renderer_render_wavefront_queued) and its hand-off (crt_renderer_render_wavefront_finish):
// whenever the host holds a batch size m <= finish_below, the current batch goes to crt_scene_path_finish_device and
// the frame is done after one more copy and wait.  finish_below 0: never.
int wavefront_queued(crt_renderer* R, const crt_scene* Sc, int spp, int max_bounces, unsigned flags,
                     const crt_trace_options* trace_opts, int sync_every, int64_t finish_below,
                     crt_wavefront_stats* stats_out, void* stream) {
    if (int rc = wavefront_check(R, Sc, spp, max_bounces, flags, true, sync_every, finish_below)) return rc;
    const int block = sync_every ? sync_every : QUEUE_SYNC_EVERY;
    crt_scene* S = const_cast<crt_scene*>(Sc);   // the trace scratch belongs to the handle (handles are not thread-safe)
    hipStream_t st = (hipStream_t)stream;
    WavefrontScratch* X = nullptr;
    if (int rc = wavefront_begin(R, spp, flags, true, stats_out, stream, &X)) return rc;
    if (!X) return CRT_OK;
    uint32_t *const d_queue = X->d_queue.get(), *const h_queue = X->h_queue.get();
    unsigned* d_err = d_queue + QUEUE_ERR;
    uint64_t* d_totals = reinterpret_cast<uint64_t*>(d_queue + QUEUE_TOTALS);
    int cur = 0;
    // A batch is never larger than the one before it (an input entry appends at most one output entry), so the last
    // count the host read bounds every later one: it is the capacity of the whole block.  Iterations enqueued after the
    // count reached 0 trace nothing and append nothing.
    int64_t m = (int64_t)R->width * R->height;
    while (m > 0) {
        if (m <= finish_below) {                             // the hand-off: the lanes run their pixels to the end
            if (int rc = crt_scene_path_finish_device(S, R, X->rays[cur].get(), X->paths[cur].get(), d_queue + cur, m,
                                                      max_bounces, nullptr, nullptr, X->remaining.get(), d_totals, stream))
                return rc;
            HIP_TRY(hipMemcpyAsync(h_queue, d_queue, QUEUE_WORDS * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            break;
        }
        for (int k = 0; k < block; ++k) {
            if (int rc = trace_enqueue(S, X->rays[cur].get(), m, trace_opts, X->hits.get(), nullptr, 0, st, d_queue + cur,
                                       d_err))
                return rc;
            if (int rc = crt_scene_path_advance_indirect_device(S, R, X->rays[cur].get(), X->hits.get(),
                                                                X->paths[cur].get(), d_queue + cur, m, max_bounces, nullptr,
                                                                nullptr, X->remaining.get(), X->rays[cur ^ 1].get(),
                                                                X->paths[cur ^ 1].get(), d_queue + (cur ^ 1), d_totals,
                                                                stream))
                return rc;
            cur ^= 1;
        }
        // the block's one copy (the counts, the error word, the totals) and its one host wait
        HIP_TRY(hipMemcpyAsync(h_queue, d_queue, QUEUE_WORDS * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        m = std::min<int64_t>(h_queue[cur], m);
        if (h_queue[QUEUE_ERR]) break;                          // reported by wavefront_end, as trace_take_error words it
    }
    uint64_t totals[2];
    std::memcpy(totals, h_queue + QUEUE_TOTALS, sizeof totals);
    crt_wavefront_stats stats{};
    stats.rays = totals[0];
    stats.iterations = (uint32_t)totals[1];
    return wavefront_end(S, X, st, stats, h_queue[QUEUE_ERR], stats_out);
}

}  // namespace

extern "C" {

int crt_renderer_render_wavefront_queued(crt_renderer* R, const crt_scene* Sc, int spp, int max_bounces, unsigned flags,
                                         const crt_trace_options* trace_opts, int sync_every,
                                         crt_wavefront_stats* stats_out, void* stream) {
    return wavefront_queued(R, Sc, spp, max_bounces, flags, trace_opts, sync_every, 0, stats_out, stream);
}

int crt_renderer_render_wavefront_finish(crt_renderer* R, const crt_scene* Sc, int spp, int max_bounces, unsigned flags,
                                         const crt_trace_options* trace_opts, int sync_every, int64_t finish_below,
                                         crt_wavefront_stats* stats_out, void* stream) {
    if (finish_below < -1)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "render wavefront: finish_below must be >= 0, or -1 for the default");
    // the default never refuses a scene: a tree the finish kernel cannot take keeps the queued loop
    if (finish_below < 0) finish_below = Sc && finish_lane_ok(Sc) ? QUEUE_FINISH_BELOW : 0;
    return wavefront_queued(R, Sc, spp, max_bounces, flags, trace_opts, sync_every, finish_below, stats_out, stream);
}

int crt_scene_export_shade_rows(const crt_scene_desc* D, float* out, int64_t* n_materials) {
    if (!D || !n_materials) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    if (D->n_materials < 0 || (D->n_materials > 0 && !D->materials)) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad materials");
    *n_materials = D->n_materials;
    if (out) {
        const std::vector<float4> rows = material_shade_rows(D);
        if (!rows.empty()) std::memcpy(out, rows.data(), rows.size() * sizeof(float4));
    }
    return CRT_OK;
}

}  // extern "C"
