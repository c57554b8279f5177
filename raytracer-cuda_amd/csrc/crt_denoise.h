// Edge-avoiding a-trous denoiser (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) guided by first-hit
// buffers.  Included by crt_hip.hip after crt_adaptive.h.  Nothing here is used by a render kernel.
//
// Guides: one record of two 16-B rows per pixel, (normal.xyz, t) (position.xyz, key), from the pixel-centre rays
// (RayQuery::centreRays' operations), crt_scene_trace_device and a pack kernel.  The filter: one launch per iteration
// i with stride 1 << i over colours kept as one 16-B row per pixel, ping-ponging between two buffers; the last
// iteration writes the W*H*3 `denoised` buffer.  Every operation is f32 and uncontracted and in the order the header
// states, so tests/helpers/denoise_model.py reproduces the bits.  Two kernels share one tap loop (denoise_taps): the
// direct one loads every tap from global memory, the tiled one from rows staged in LDS.  The variance-guided filter of
// crt_variance.h is the same tap loop, bodies and host launch loop in their other mode (VAR).
#pragma once

constexpr int DENOISE_MISS_KEY = 0x7fffffff;

struct GuideRayParams {
    crt_camera_desc cam;
    int width, height;
    float4* __restrict__ rays;
};

// RayQuery::centreRays on the device, operation for operation: u = ((float)x + 0.5f) / (float)W, v likewise (the
// build's correctly rounded division), dir = ((lower_left + u * horizontal) + v * vertical) - origin, lens offset 0.
__global__ __launch_bounds__(256) void crt_guide_rays_kernel(GuideRayParams G) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= G.width * G.height) return;
    const int x = pix % G.width, y = pix / G.width;
    const float u = ((float)x + 0.5f) / (float)G.width, v = ((float)y + 0.5f) / (float)G.height;
    float d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        d[a] = ((G.cam.lower_left[a] + u * G.cam.horizontal[a]) + v * G.cam.vertical[a]) - G.cam.origin[a];
    G.rays[2 * (size_t)pix] = make_float4(G.cam.origin[0], G.cam.origin[1], G.cam.origin[2], __builtin_inff());
    G.rays[2 * (size_t)pix + 1] = make_float4(d[0], d[1], d[2], 0.f);
}

// The guide record of every pixel from its ray and its crt_hit: the hit's own (geometric, unflipped) normal and t,
// position = o + t * d (V3's operators: a multiply, then an add), key = object; a miss is (0, 0, 0, -1) (0, 0, 0,
// DENOISE_MISS_KEY).  Lane 0 of every wave stores how many of its pixels hit (no atomics).
__global__ __launch_bounds__(256) void crt_guide_pack_kernel(const float4* __restrict__ rays, const float4* __restrict__ hits,
                                                             float4* __restrict__ guides, uint32_t* __restrict__ wave_hits,
                                                             int n_pix) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (pix < n_pix) {
        const float4 ha = hits[2 * (size_t)pix], hb = hits[2 * (size_t)pix + 1];
        float4 g0 = make_float4(0.f, 0.f, 0.f, -1.f), g1 = make_float4(0.f, 0.f, 0.f, __int_as_float(DENOISE_MISS_KEY));
        hit = !(ha.x < 0.f);
        if (hit) {
            const float4 ra = rays[2 * (size_t)pix], rb = rays[2 * (size_t)pix + 1];
            const V3 p = v3(ra.x, ra.y, ra.z) + ha.x * v3(rb.x, rb.y, rb.z);
            g0 = make_float4(hb.x, hb.y, hb.z, ha.x);
            g1 = make_float4(p.x, p.y, p.z, ha.y);      // ha.y: the object index as int bits
        }
        guides[2 * (size_t)pix] = g0;
        guides[2 * (size_t)pix + 1] = g1;
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && pix < n_pix) wave_hits[pix >> 6] = (uint32_t)__popcll(m);   // pix: the wave's first
}

// c0 = scale * sum per channel, as a 16-B row; tile_spp non-null: scale = 1.f / (float)tile_spp[tile], as
// crt_resolve_adaptive_kernel forms it.
__global__ __launch_bounds__(256) void crt_denoise_input_kernel(const float* __restrict__ sum, float4* __restrict__ col,
                                                                const int32_t* __restrict__ tile_spp, int width, int n_pix,
                                                                int tiles_x, float scale) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= n_pix) return;
    if (tile_spp) {
        const int x = pix % width, y = pix / width;
        scale = 1.f / (float)tile_spp[(y >> 3) * tiles_x + (x >> 3)];
    }
    col[pix] = make_float4(scale * sum[3 * (size_t)pix], scale * sum[3 * (size_t)pix + 1], scale * sum[3 * (size_t)pix + 2], 0.f);
}

__device__ __forceinline__ float variance_lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

// One struct for the plain and the variance-guided kernels (crt_variance.h).
struct DenoiseParams {
    const float4* __restrict__ in;      // c_i (variance: (c_i, v_i)), 1 row per pixel
    const float4* __restrict__ guides;  // 2 rows per pixel
    float4* __restrict__ out;           // c_{i+1} as rows, or null on the last iteration
    float* __restrict__ out3;           // the last iteration's output, 3 floats per pixel
    int width, height, stride;
    float k_c;                          // plain: 1 / sigma_color^2 of this level; variance: sigma_luminance as given
    float inv_n, inv_x;                 // 1 / sigma^2
    int on_c, on_n, on_x;               // 0: the term is off (sigma = +inf), never computed
};

// exp(-X) for 0 <= X < 80 (crt_hip.h has the steps): k = rint(X * log2 e); r = X - k ln 2 in two parts, the first
// product exact; a degree-6 polynomial in t = -r; 2^-k by an integer subtraction from the exponent field.
__device__ __forceinline__ float denoise_exp_neg(float X) {
    const float k = rintf(X * 0x1.715476p+0f);
    const float r = (X - k * 0.693359375f) - k * -0x1.bd0106p-13f;
    const float t = -r;
    float p = 0x1.6c16c2p-10f * t + 0x1.111112p-7f;
    p = p * t + 0x1.555556p-5f;
    p = p * t + 0x1.555556p-3f;
    p = p * t + 0.5f;
    p = p * t + 1.f;
    p = p * t + 1.f;
    return __int_as_float(__float_as_int(p) - ((int)k << 23));
}

__device__ __forceinline__ float denoise_dist2(float4 a, float4 b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// The tap loop all four kernels share.  Pixel (x, y) with its own rows (c, g0, g1); fetch(dy, dx, qx, qy, which)
// returns row `which` (0 colour, 1 guide row 0, 2 guide row 1) of tap q = (x + dx s, y + dy s), and is only called for
// a q inside the frame.  dy outer, dx inner, the centre in its place with w = 1; a tap outside the frame, with another
// key, or with !(X < 80) is skipped.  VAR (the variance-guided filter): the luminance term, as wide as the 3 x 3
// prefiltered variance says, stands in the colour term's place, and the variance c.w is accumulated beside the colours;
// vfetch(dy, dx, qx, qy) returns (v, key as float bits) of the prefilter's tap (x + dx, y + dy), called only inside
// the frame.
template <bool VAR, class Fetch, class VFetch>
__device__ __forceinline__ float4 denoise_taps(const DenoiseParams& D, int x, int y, float4 c, float4 g0, float4 g1,
                                               Fetch fetch, VFetch vfetch) {
    constexpr float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const int key = __float_as_int(g1.w);
    float inv_den = 0.f, lc = 0.f;
    if constexpr (VAR) {
        constexpr float hg[3] = {0.25f, 0.5f, 0.25f};
        if (D.on_c) {
            float gs = 0.f, gw = 0.f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const float kg = hg[dy + 1] * hg[dx + 1];
                    if (dy == 0 && dx == 0) { gs = gs + kg * c.w; gw = gw + kg; continue; }
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= D.width || qy < 0 || qy >= D.height) continue;
                    const float2 vk = vfetch(dy, dx, qx, qy);
                    if (__float_as_int(vk.y) != key) continue;
                    gs = gs + kg * vk.x; gw = gw + kg;
                }
            }
            const float g = gs / gw;
            const float den = D.k_c * sqrtf(g) + 0x1p-20f;
            inv_den = 1.f / den;
        }
        lc = variance_lum(c.x, c.y, c.z);
    }
    float ax = 0.f, ay = 0.f, az = 0.f, av = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float k = h[dy + 2] * h[dx + 2];
            if (dy == 0 && dx == 0) {
                ax = ax + k * c.x; ay = ay + k * c.y; az = az + k * c.z;
                if constexpr (VAR) av = av + (k * k) * c.w;
                sw = sw + k;
                continue;
            }
            const int qx = x + dx * D.stride, qy = y + dy * D.stride;
            if (qx < 0 || qx >= D.width || qy < 0 || qy >= D.height) continue;
            const float4 q1 = fetch(dy, dx, qx, qy, 2);
            if (__float_as_int(q1.w) != key) continue;
            const float4 qc = fetch(dy, dx, qx, qy, 0);
            float xc = 0.f, xn = 0.f, xx = 0.f;
            if constexpr (VAR) {
                if (D.on_c) xc = fabsf(lc - variance_lum(qc.x, qc.y, qc.z)) * inv_den;
            } else {
                if (D.on_c) xc = denoise_dist2(c, qc) * D.k_c;
            }
            if (D.on_n) xn = denoise_dist2(g0, fetch(dy, dx, qx, qy, 1)) * D.inv_n;
            if (D.on_x) xx = denoise_dist2(g1, q1) * D.inv_x;
            const float X = (xc + xn) + xx;
            if (!(X < 80.f)) continue;
            const float kw = k * denoise_exp_neg(X);
            ax = ax + kw * qc.x; ay = ay + kw * qc.y; az = az + kw * qc.z;
            if constexpr (VAR) av = av + (kw * kw) * qc.w;
            sw = sw + kw;
        }
    }
    return make_float4(ax / sw, ay / sw, az / sw, VAR ? av / (sw * sw) : 0.f);
}

__device__ __forceinline__ void denoise_store(const DenoiseParams& D, size_t pix, float4 o) {
    if (D.out3) { D.out3[3 * pix] = o.x; D.out3[3 * pix + 1] = o.y; D.out3[3 * pix + 2] = o.z; }
    else D.out[pix] = o;
}

// The prefilter's tap from global memory: the fourth lanes of the colour row and of the second guide row.
__device__ __forceinline__ float2 denoise_vk_global(const DenoiseParams& D, int qx, int qy) {
    const size_t q = (size_t)qy * D.width + qx;          // inside the frame: the caller checked
    return make_float2(D.in[q].w, D.guides[2 * q + 1].w);
}

// The direct kernels: one lane per pixel, every tap from global memory.  The yardstick; any stride.
constexpr int DENOISE_BX = 64, DENOISE_DIRECT_BY = 4;
template <bool VAR>
__device__ __forceinline__ void denoise_direct_body(const DenoiseParams& D) {
    const int x = blockIdx.x * DENOISE_BX + threadIdx.x, y = blockIdx.y * DENOISE_DIRECT_BY + threadIdx.y;
    if (x >= D.width || y >= D.height) return;
    const size_t pix = (size_t)y * D.width + x;
    const float4 c = D.in[pix], g0 = D.guides[2 * pix], g1 = D.guides[2 * pix + 1];
    const float4 o = denoise_taps<VAR>(D, x, y, c, g0, g1,
        [&](int, int, int qx, int qy, int which) {
            const size_t q = (size_t)qy * D.width + qx;  // inside the frame: the tap loop checked
            return which == 0 ? D.in[q] : D.guides[2 * q + (which - 1)];
        },
        [&](int, int, int qx, int qy) { return denoise_vk_global(D, qx, qy); });
    denoise_store(D, pix, o);
}

// The tiled kernels: a workgroup of 64 x 8 lanes filters the pixels x0 .. x0 + 63 of the 8 rows y = r + s (8 g + j),
// j = 0 .. 7, of one residue class r of y modulo the stride s: in an a-trous pass only those rows interact.  It stages
// the 12 rows j = -2 .. 9 over x0 - 2 s .. x0 + 63 + 2 s in LDS, as three arrays of 16-B rows (colour, guide row 0,
// guide row 1) with coalesced 16-B loads along x, then runs the shared tap loop out of LDS.  LDS: 12 (64 + 4 s) 48 B,
// dynamic: 39,168 B at s = 1, 55,296 B at s = 8 and 73,728 B at s = 16, the largest stride it is launched with
// (DENOISE_TILED_MAX_STRIDE: measured faster than the direct kernel at s = 1 .. 16 and slower at s = 32, where a block
// fetches 12 x 192 rows for 512 pixels).  Above 64 KiB the host raises the kernel's dynamic LDS limit once.
// Entries outside the frame are never written and never read (the tap loop's frame test comes before the fetch).
// VAR: the variance rides in the staged colour rows' fourth lane.  The prefilter's eight taps lie at +-1 pixel whatever
// the stride: at s = 1 they are among the staged rows and columns (j +- 1, x +- 1) and come from LDS; at s > 1 the rows
// y +- 1 belong to other residue classes, which this block does not stage, and all eight come from global memory
// (DESIGN.md §24 has the cost).
constexpr int DENOISE_TY = 8, DENOISE_ROWS = DENOISE_TY + 4;
constexpr int DENOISE_TILED_MAX_STRIDE = 16;
template <bool VAR>
__device__ __forceinline__ void denoise_tiled_body(const DenoiseParams& D, int groups) {
    extern __shared__ float4 denoise_lds[];
    const int s = D.stride, cols = DENOISE_BX + 4 * s, n = DENOISE_ROWS * cols;
    float4* l_c = denoise_lds;
    float4* l_g0 = denoise_lds + n;
    float4* l_g1 = denoise_lds + 2 * n;
    const int r = blockIdx.y / groups, g = blockIdx.y % groups;     // blockIdx.y < s * groups
    const int x0 = blockIdx.x * DENOISE_BX, j0 = g * DENOISE_TY;
    const int tid = threadIdx.y * DENOISE_BX + threadIdx.x;
    for (int i = tid; i < n; i += DENOISE_BX * DENOISE_TY) {
        const int row = i / cols, col = i - row * cols;
        const int qx = x0 - 2 * s + col, qy = r + s * (j0 + row - 2);
        if (qx >= 0 && qx < D.width && qy >= 0 && qy < D.height) {
            const size_t q = (size_t)qy * D.width + qx;
            l_c[i] = D.in[q];
            l_g0[i] = D.guides[2 * q];
            l_g1[i] = D.guides[2 * q + 1];
        }
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = r + s * (j0 + threadIdx.y);
    if (x >= D.width || y >= D.height) return;
    const int at = (threadIdx.y + 2) * cols + threadIdx.x + 2 * s;
    const float4 o = denoise_taps<VAR>(D, x, y, l_c[at], l_g0[at], l_g1[at],
        [&](int dy, int dx, int, int, int which) {
            const int q = at + dy * cols + dx * s;       // row j + dy, column x + dx s of the staged block
            return which == 0 ? l_c[q] : which == 1 ? l_g0[q] : l_g1[q];
        },
        [&](int dy, int dx, int qx, int qy) {
            if (s == 1) { const int q = at + dy * cols + dx; return make_float2(l_c[q].w, l_g1[q].w); }
            return denoise_vk_global(D, qx, qy);
        });
    denoise_store(D, (size_t)y * D.width + x, o);
}

// The host takes these four addresses (the dynamic LDS limit is per kernel function) and the profiles name them.
__global__ __launch_bounds__(DENOISE_BX * DENOISE_DIRECT_BY) void crt_denoise_direct_kernel(DenoiseParams D) {
    denoise_direct_body<false>(D);
}
__global__ __launch_bounds__(DENOISE_BX * DENOISE_TY) void crt_denoise_tiled_kernel(DenoiseParams D, int groups) {
    denoise_tiled_body<false>(D, groups);
}
__global__ __launch_bounds__(DENOISE_BX * DENOISE_DIRECT_BY) void crt_denoise_variance_direct_kernel(DenoiseParams D) {
    denoise_direct_body<true>(D);
}
__global__ __launch_bounds__(DENOISE_BX * DENOISE_TY) void crt_denoise_variance_tiled_kernel(DenoiseParams D, int groups) {
    denoise_tiled_body<true>(D, groups);
}

namespace {

// The state is allocated on first use and initialised on `st`, the stream its first user goes on to enqueue on.
int denoise_state(crt_renderer* R, hipStream_t st, DenoiseState** out) {
    return first_use(R->denoise, "the denoiser state of this renderer could not be allocated", out, [&](DenoiseState* N) -> int {
        const size_t n_pix = (size_t)R->width * R->height;
        HIP_TRY(N->rays.alloc(n_pix * 2));
        HIP_TRY(N->hits.alloc(n_pix * 2));
        HIP_TRY(N->guides[0].alloc(n_pix * 2));
        HIP_TRY(N->col[0].alloc(n_pix));
        HIP_TRY(N->col[1].alloc(n_pix));
        HIP_TRY(N->denoised.alloc(n_pix * 3));
        HIP_TRY(N->wave_hits.alloc((n_pix + 63) / 64));
        HIP_TRY(hipMemsetAsync(N->denoised.get(), 0, n_pix * 12, st));
        for (DevEvent* e : {&N->g0, &N->g1, &N->f0, &N->f1}) HIP_TRY(e->create());
        for (DevEvent& e : N->it) HIP_TRY(e.create());
        return CRT_OK;
    });
}

// Before new guides are written: a buffer the reprojection keeps as its previous frame is left alone.
void denoise_next_guides(DenoiseState* N) {
    if (N->keep) { N->gi ^= 1; N->keep = false; }
}

// The iterations and the three sigmas of either filter's options; first: the colour term's name.
int denoise_check_sigmas(const std::string& w, int iterations, const char* first, float s0, float s1, float s2) {
    if (iterations < 0 || iterations > 8) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": iterations must be 0..8 (0 = 5)");
    const float sig[3] = {s0, s1, s2};
    const char* name[3] = {first, "sigma_normal", "sigma_position"};
    for (int k = 0; k < 3; ++k)
        if (!(sig[k] == __builtin_inff() || (sig[k] >= 0x1p-50f && sig[k] <= 0x1p50f)))
            return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": " + name[k] + " must be in [2^-50, 2^50] or +inf (that term off)");
    return CRT_OK;
}

// The checks of the options alone (no handle, no device).
int denoise_check_options(const crt_denoise_options* o, const char* who) {
    const std::string w = who;
    if (!o) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": null options");
    if (int rc = denoise_check_sigmas(w, o->iterations, "sigma_color", o->sigma_color, o->sigma_normal, o->sigma_position))
        return rc;
    if (o->flags & ~(CRT_DENOISE_TILE_SCALE | CRT_DENOISE_DIRECT_ONLY))
        return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": unknown flag bits");
    if (o->reserved != 0) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": reserved must be 0");
    return CRT_OK;
}

// What differs between the two filters on the host: the kernel pair, whose dynamic LDS limit was raised (the attribute is
// per kernel function), and the colour term.
struct DenoiseFilter {
    void (*tiled)(DenoiseParams, int);
    void (*direct)(DenoiseParams);
    bool* lds_raised;
    bool quarter;       // true: the colour term is 1 / sigma^2 and quarters per level; false: the sigma as given, every level
};

// One launch per iteration i with stride 1 << i, from c0 (or col[0]) to `denoised`.  sigma: colour (or luminance),
// normal, position; iterations, flags: the options' (checked).
// timed: an event after every launch (crt_renderer_denoise_iteration_ms); the caller waits for f1 before reading them.
int denoise_iterations(crt_renderer* R, DenoiseState* N, const DenoiseFilter& F, const float* sigma, int iterations,
                       uint32_t flags, const float4* c0, hipStream_t st, bool timed) {
    const int W = R->width, H = R->height;
    if (!iterations) iterations = 5;
    const bool direct_only = (flags & CRT_DENOISE_DIRECT_ONLY) != 0;
    N->timed_iterations = 0;
    if (timed) HIP_TRY(hipEventRecord(N->it[0].get(), st));
    DenoiseParams D{};
    D.guides = N->guides[N->gi].get();
    D.width = W; D.height = H;
    const float inf = __builtin_inff();
    D.on_c = sigma[0] != inf; D.on_n = sigma[1] != inf; D.on_x = sigma[2] != inf;
    D.k_c = !D.on_c ? 0.f : F.quarter ? 1.f / (sigma[0] * sigma[0]) : sigma[0];
    D.inv_n = D.on_n ? 1.f / (sigma[1] * sigma[1]) : 0.f;
    D.inv_x = D.on_x ? 1.f / (sigma[2] * sigma[2]) : 0.f;
    for (int i = 0; i < iterations; ++i) {
        const bool last = i == iterations - 1;
        D.in = i == 0 && c0 ? c0 : N->col[i & 1].get();
        D.out = last ? nullptr : N->col[(i + 1) & 1].get();
        D.out3 = last ? N->denoised.get() : nullptr;
        D.stride = 1 << i;
        if (!direct_only && D.stride <= DENOISE_TILED_MAX_STRIDE) {
            const int s = D.stride, rows = (H + s - 1) / s;                   // the rows of residue class 0, the longest
            const int groups = (rows + DENOISE_TY - 1) / DENOISE_TY;
            const size_t lds = (size_t)DENOISE_ROWS * (DENOISE_BX + 4 * s) * 48;
            if (lds > 65536 && !*F.lds_raised) {
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(F.tiled), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            DENOISE_ROWS * (DENOISE_BX + 4 * DENOISE_TILED_MAX_STRIDE) * 48));
                *F.lds_raised = true;
            }
            hipLaunchKernelGGL(F.tiled, dim3((W + DENOISE_BX - 1) / DENOISE_BX, s * groups), dim3(DENOISE_BX, DENOISE_TY), lds,
                               st, D, groups);
        } else {
            hipLaunchKernelGGL(F.direct, dim3((W + DENOISE_BX - 1) / DENOISE_BX, (H + DENOISE_DIRECT_BY - 1) / DENOISE_DIRECT_BY),
                               dim3(DENOISE_BX, DENOISE_DIRECT_BY), 0, st, D);
        }
        if (F.quarter && D.on_c) D.k_c = D.k_c * 4.f;    // the colour sigma halves per level
        if (timed) HIP_TRY(hipEventRecord(N->it[i + 1].get(), st));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(N->f1.get(), st));
    if (timed) N->timed_iterations = iterations;
    N->have_denoised = true;
    return CRT_OK;
}

// The filter on `st`: c0 from the sums, then the iterations.  The handle's guides and options were checked.
// c0 non-null (crt_renderer_denoise_history): iteration 0 reads those rows' (x, y, z) instead and the sums are not read.
int denoise_run(crt_renderer* R, DenoiseState* N, const crt_denoise_options* o, float scale, hipStream_t st, bool timed,
                const float4* c0 = nullptr) {
    const int W = R->width, n_pix = W * R->height;
    const bool tile_scale = (o->flags & CRT_DENOISE_TILE_SCALE) != 0;
    HIP_TRY(hipEventRecord(N->f0.get(), st));
    if (!c0)
        hipLaunchKernelGGL(crt_denoise_input_kernel, dim3((n_pix + 255) / 256), dim3(256), 0, st, R->d_sum, N->col[0].get(),
                           tile_scale ? R->adaptive->tile_spp.get() : nullptr, W, n_pix, R->tiles_x(), scale);
    const float sigma[3] = {o->sigma_color, o->sigma_normal, o->sigma_position};
    const DenoiseFilter F{crt_denoise_tiled_kernel, crt_denoise_direct_kernel, &N->lds_raised, true};
    return denoise_iterations(R, N, F, sigma, o->iterations, o->flags, c0, st, timed);
}

// The pixels whose guide is a hit: the pack kernel's per-wave counts, summed (N->counted).
int denoise_pixels_hit(crt_renderer* R, DenoiseState* N, uint32_t* out) {
    std::vector<uint32_t> w(((size_t)R->width * R->height + 63) / 64);
    HIP_TRY(hipMemcpy(w.data(), N->wave_hits.get(), w.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t c : w) *out += c;
    return CRT_OK;
}

// The stats of the filter run just enqueued on `N` (crt_renderer_denoise, crt_renderer_denoise_history): waits for its
// last launch.
int denoise_stats(crt_renderer* R, DenoiseState* N, const crt_denoise_options* o, crt_denoise_stats* out) {
    crt_denoise_stats s{};
    s.iterations = (uint32_t)(o->iterations ? o->iterations : 5);
    HIP_TRY(hipEventSynchronize(N->f1.get()));
    HIP_TRY(hipEventElapsedTime(&s.filter_ms, N->f0.get(), N->f1.get()));
    if (N->timed_guides) {
        HIP_TRY(hipEventSynchronize(N->g1.get()));
        HIP_TRY(hipEventElapsedTime(&s.guides_ms, N->g0.get(), N->g1.get()));
    }
    if (N->counted)
        if (int rc = denoise_pixels_hit(R, N, &s.pixels_hit)) return rc;
    *out = s;
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_renderer_compute_guides(crt_renderer* R, const crt_scene* S, const crt_trace_options* opts, void* stream) {
    if (!R || !S) return set_error(CRT_ERR_INVALID_ARGUMENT, "compute guides: null argument");
    if (S->device != R->device)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "compute guides: scene and renderer on different devices");
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, "compute guides: camera not set");
    if (R->tile_shards > 1) return set_error(CRT_ERR_UNSUPPORTED, "compute guides: a pixel shard other than (0, 1)");
    HIP_TRY(hipSetDevice(R->device));
    hipStream_t st = (hipStream_t)stream;
    DenoiseState* N = nullptr;
    if (int rc = denoise_state(R, st, &N)) return rc;
    const int n_pix = R->width * R->height;
    N->have_guides = N->counted = false;
    denoise_next_guides(N);
    N->guide_cam = R->cam;
    HIP_TRY(hipEventRecord(N->g0.get(), st));
    GuideRayParams G{};
    G.cam = R->cam; G.width = R->width; G.height = R->height; G.rays = N->rays.get();
    hipLaunchKernelGGL(crt_guide_rays_kernel, dim3((n_pix + 255) / 256), dim3(256), 0, st, G);
    HIP_TRY(hipGetLastError());
    if (int rc = crt_scene_trace_device(S, reinterpret_cast<const crt_ray*>(N->rays.get()), n_pix, opts,
                                        reinterpret_cast<crt_hit*>(N->hits.get()), nullptr, 0u, stream))
        return rc;
    hipLaunchKernelGGL(crt_guide_pack_kernel, dim3((n_pix + 255) / 256), dim3(256), 0, st, N->rays.get(), N->hits.get(), N->guides[N->gi].get(),
                       N->wave_hits.get(), n_pix);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(N->g1.get(), st));
    N->have_guides = N->counted = N->timed_guides = true;
    return CRT_OK;
}

int crt_renderer_denoise(crt_renderer* R, const crt_denoise_options* o, float scale, crt_denoise_stats* stats_out,
                         void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise: null renderer");
    if (int rc = denoise_check_options(o, "denoise")) return rc;
    const bool tile_scale = (o->flags & CRT_DENOISE_TILE_SCALE) != 0;
    if (!tile_scale && !(scale > 0.f)) return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise: scale must be > 0");
    if (tile_scale && (!R->adaptive || !R->adaptive->tile_spp))
        return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise: the tile scale needs an adaptive render on this renderer");
    if (R->tile_shards > 1) return set_error(CRT_ERR_UNSUPPORTED, "denoise: a pixel shard other than (0, 1)");
    if (!R->denoise || !R->denoise->have_guides)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise: no guides computed yet (crt_renderer_compute_guides)");
    HIP_TRY(hipSetDevice(R->device));
    DenoiseState* N = nullptr;
    if (int rc = denoise_state(R, (hipStream_t)stream, &N)) return rc;
    if (int rc = denoise_run(R, N, o, scale, (hipStream_t)stream, stats_out != nullptr)) return rc;
    return stats_out ? denoise_stats(R, N, o, stats_out) : CRT_OK;
}

int crt_renderer_resolve_denoised(crt_renderer* R, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    if (!R->denoise || !R->denoise->have_denoised)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "resolve denoised: no denoised frame on this renderer yet");
    HIP_TRY(hipSetDevice(R->device));
    const int n = R->width * R->height;
    hipLaunchKernelGGL(crt_resolve_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, R->denoise->denoised.get(),
                       R->d_rgba.get(), n, 1.f);
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

int crt_renderer_read_denoised(crt_renderer* R, float* out) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "read denoised: null argument");
    if (!R->denoise || !R->denoise->have_denoised)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "read denoised: no denoised frame on this renderer yet");
    return read_dev(R, out, R->denoise->denoised.get(), (size_t)R->width * R->height * 12);
}

int crt_renderer_read_guides(crt_renderer* R, float* out) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "read guides: null argument");
    if (!R->denoise || !R->denoise->have_guides)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "read guides: no guides computed yet (crt_renderer_compute_guides)");
    return read_dev(R, out, R->denoise->guides[R->denoise->gi].get(), (size_t)R->width * R->height * 32);
}

int crt_renderer_denoise_iteration_ms(crt_renderer* R, float* out9) {
    if (!R || !out9) return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise iteration ms: null argument");
    if (!R->denoise || !R->denoise->timed_iterations)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise iteration ms: no denoise with a stats pointer on this renderer yet");
    DenoiseState* N = R->denoise.get();
    HIP_TRY(hipSetDevice(R->device));
    HIP_TRY(hipEventSynchronize(N->f1.get()));
    for (int k = 0; k < 9; ++k) out9[k] = 0.f;
    HIP_TRY(hipEventElapsedTime(&out9[0], N->f0.get(), N->it[0].get()));
    for (int i = 0; i < N->timed_iterations; ++i) HIP_TRY(hipEventElapsedTime(&out9[i + 1], N->it[i].get(), N->it[i + 1].get()));
    return CRT_OK;
}

float* crt_renderer_denoised_device_ptr(crt_renderer* R) { return R && R->denoise ? R->denoise->denoised.get() : nullptr; }

// The filter on caller-supplied buffers: the renderer's own state and the host function crt_renderer_denoise calls, on
// the null stream.  The colours go into the renderer's linear buffer and are taken with scale 1 (1.f * c = c).
int crt_selftest_denoise(crt_renderer* R, const float* color, const float* guides, const crt_denoise_options* o, float* out) {
    if (!R || !color || !guides || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "selftest denoise: null argument");
    if (int rc = denoise_check_options(o, "selftest denoise")) return rc;
    if (o->flags & CRT_DENOISE_TILE_SCALE)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "selftest denoise: takes the colours as they are (no tile scale)");
    HIP_TRY(hipSetDevice(R->device));
    DenoiseState* N = nullptr;
    if (int rc = denoise_state(R, 0, &N)) return rc;
    const size_t n_pix = (size_t)R->width * R->height;
    HIP_TRY(hipMemcpy(R->d_sum, color, n_pix * 12, hipMemcpyHostToDevice));
    denoise_next_guides(N);
    HIP_TRY(hipMemcpy(N->guides[N->gi].get(), guides, n_pix * 32, hipMemcpyHostToDevice));
    N->have_guides = true;
    N->counted = N->timed_guides = false;
    N->guide_cam = crt_camera_desc{};                // no camera made these guides: a reprojection after this restarts
    if (int rc = denoise_run(R, N, o, 1.f, 0, false)) return rc;
    HIP_TRY(hipStreamSynchronize(0));
    HIP_TRY(hipMemcpy(out, N->denoised.get(), n_pix * 12, hipMemcpyDeviceToHost));
    return CRT_OK;
}

}  // extern "C"
