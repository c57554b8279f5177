// Variance-guided filtering of the history (Schied et al., HPG 2017): the first two luminance moments
// carried through the reprojection, a per-pixel variance from them, and an a-trous filter whose luminance edge-stop is
// as wide as that variance, itself filtered, says.  Included by crt_hip.hip after crt_reproject.h.  Nothing here is used
// by a render kernel, and no kernel of crt_denoise.h or crt_reproject.h is touched: the four kernels below are new and
// share only those files' __forceinline__ helpers (denoise_exp_neg, denoise_dist2, reproject_dot, reproject_finite).
//
// Every operation is f32 and uncontracted and in the order the header states, so tests/helpers/variance_model.py
// reproduces the bits.  The variance rides in the fourth lane of the filter's 16-B colour rows, in global memory and in
// the tiled kernel's LDS, so the filter moves the bytes the plain one moves, plus the prefilter's taps.
#pragma once

__device__ __forceinline__ float variance_lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

struct ReprojectMomentsParams {
    ReprojectParams P;
    const float2* __restrict__ mom_in;      // the previous moments, 1 row per pixel
    float2* __restrict__ mom_out;
};

// crt_reproject_kernel's rule, operation for operation, so the history rows are its bits; the moments take exactly the
// taps the colours took, with the colours' weights, sum and blend factor.  The moment rows of those taps are loaded
// with their history rows.
__global__ __launch_bounds__(REPROJECT_BX * REPROJECT_BY) void crt_reproject_moments_kernel(ReprojectMomentsParams M) {
    const ReprojectParams& P = M.P;
    const int x = blockIdx.x * REPROJECT_BX + threadIdx.x, y = blockIdx.y * REPROJECT_BY + threadIdx.y;
    const int W = P.width, H = P.height;
    bool took = false;
    if (x < W && y < H) {
        const size_t pix = (size_t)y * W + x;
        const float4 g1 = P.guides[2 * pix + 1];
        const float cx = P.scale * P.sum[3 * pix], cy = P.scale * P.sum[3 * pix + 1], cz = P.scale * P.sum[3 * pix + 2];
        float4 out = make_float4(cx, cy, cz, 1.f);
        const float l = variance_lum(cx, cy, cz);
        const float l2 = l * l;
        float2 om = make_float2(l, l2);
        const int key = __float_as_int(g1.w);
        if (P.valid && key != DENOISE_MISS_KEY && reproject_finite(cx) && reproject_finite(cy) && reproject_finite(cz)) {
            const float dx = g1.x - P.o[0], dy = g1.y - P.o[1], dz = g1.z - P.o[2];
            const float s = P.LN / reproject_dot(dx, dy, dz, P.N[0], P.N[1], P.N[2]);
            const float qx = s * dx - P.L[0], qy = s * dy - P.L[1], qz = s * dz - P.L[2];
            const float u = reproject_dot(qx, qy, qz, P.hor[0], P.hor[1], P.hor[2]) / P.hh;
            const float v = reproject_dot(qx, qy, qz, P.ver[0], P.ver[1], P.ver[2]) / P.vv;
            const float fx = u * (float)W - 0.5f, fy = v * (float)H - 0.5f;
            if (s > 0.f && fx > -1.f && fx < (float)W && fy > -1.f && fy < (float)H) {
                const float x0f = floorf(fx), y0f = floorf(fy);
                const float ax = fx - x0f, ay = fy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;          // -1 .. W - 1, -1 .. H - 1
                float lim = 0.f;
                if (P.on_x) lim = P.tol2 * reproject_dot(dx, dy, dz, dx, dy, dz);
                size_t q[4];
                float4 p1[4];
                bool ok[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {                    // j outer, i inner
                    const int tx = x0 + (k & 1), ty = y0 + (k >> 1);
                    ok[k] = tx >= 0 && tx < W && ty >= 0 && ty < H;
                    q[k] = (size_t)min(max(ty, 0), H - 1) * W + min(max(tx, 0), W - 1);
                    p1[k] = P.prev_guides[2 * q[k] + 1];
                }
                float w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    w[k] = ((k & 1) ? ax : 1.f - ax) * ((k >> 1) ? ay : 1.f - ay);
                    ok[k] = ok[k] && w[k] > 0.f && __float_as_int(p1[k].w) == key;
                    if (P.on_x) ok[k] = ok[k] && denoise_dist2(g1, p1[k]) <= lim;
                }
                if (P.on_n) {
                    const float4 g0 = P.guides[2 * pix];
                    float4 p0[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k)                  // issued together, tested afterwards
                        if (ok[k]) p0[k] = P.prev_guides[2 * q[k]];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (ok[k]) ok[k] = reproject_dot(g0.x, g0.y, g0.z, p0[k].x, p0[k].y, p0[k].z) >= P.normal_min;
                }
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                float2 am = make_float2(0.f, 0.f);
                float sw = 0.f;
                float4 hr[4];
                float2 mr[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)                      // the rows of the taps that passed, issued together
                    if (ok[k]) { hr[k] = P.hist_in[q[k]]; mr[k] = M.mom_in[q[k]]; }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (ok[k] && reproject_finite(hr[k].x) && reproject_finite(hr[k].y) && reproject_finite(hr[k].z)) {
                        acc.x = acc.x + w[k] * hr[k].x; acc.y = acc.y + w[k] * hr[k].y;
                        acc.z = acc.z + w[k] * hr[k].z; acc.w = acc.w + w[k] * hr[k].w;
                        am.x = am.x + w[k] * mr[k].x; am.y = am.y + w[k] * mr[k].y;
                        sw = sw + w[k];
                    }
                if (sw > 0.f) {
                    const float hx = acc.x / sw, hy = acc.y / sw, hz = acc.z / sw, hl = acc.w / sw;
                    const float m = fminf(hl + 1.f, P.max_history);
                    const float a = 1.f / m;
                    out = make_float4(hx + (cx - hx) * a, hy + (cy - hy) * a, hz + (cz - hz) * a, m);
                    const float h1 = am.x / sw, h2 = am.y / sw;
                    om = make_float2(h1 + (l - h1) * a, h2 + (l2 - h2) * a);
                    took = true;
                }
            }
        }
        P.hist_out[pix] = out;
        M.mom_out[pix] = om;
    }
    const unsigned long long taken = __ballot(took);
    if (threadIdx.x == 0 && y < H) P.wave_taken[(size_t)y * P.blocks_x + blockIdx.x] = (uint32_t)__popcll(taken);
}

// The variance estimate: c_0 rows (r, g, b, v) from the history rows (r, g, b, len), the moments and the guides' keys.
// One lane per pixel; a pixel with a long history needs only its own rows, a short one gathers the 7 x 7 window's
// (key, moments) from global memory (clamped addresses are never formed: the frame test comes first).
__global__ __launch_bounds__(256) void crt_variance_estimate_kernel(const float4* __restrict__ hist, const float2* __restrict__ mom,
                                                                    const float4* __restrict__ guides, float4* __restrict__ col,
                                                                    float* __restrict__ variance, int width, int height,
                                                                    float min_history) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= width * height) return;
    const int x = pix % width, y = pix / width;
    const float4 hrow = hist[pix];
    float v;
    if (hrow.w >= min_history) {
        const float2 m = mom[pix];
        v = fmaxf(0.f, m.y - m.x * m.x);
    } else {
        const int key = __float_as_int(guides[2 * (size_t)pix + 1].w);
        float s1 = 0.f, s2 = 0.f, n = 0.f;
        for (int dy = -3; dy <= 3; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= height) continue;
#pragma unroll
            for (int dx = -3; dx <= 3; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= width) continue;
                const size_t q = (size_t)qy * width + qx;
                if (__float_as_int(guides[2 * q + 1].w) != key) continue;
                const float2 m = mom[q];
                if (!reproject_finite(m.x) || !reproject_finite(m.y)) continue;
                s1 = s1 + m.x; s2 = s2 + m.y; n = n + 1.f;
            }
        }
        v = 0.f;
        if (n != 0.f) {
            const float M1 = s1 / n, M2 = s2 / n;
            v = fmaxf(0.f, M2 - M1 * M1) * (min_history / hrow.w);
        }
    }
    col[pix] = make_float4(hrow.x, hrow.y, hrow.z, v);
    variance[pix] = v;
}

struct VarianceFilterParams {
    const float4* __restrict__ in;      // (c_i, v_i), 1 row per pixel
    const float4* __restrict__ guides;  // 2 rows per pixel
    float4* __restrict__ out;           // (c_{i+1}, v_{i+1}) as rows, or null on the last iteration
    float* __restrict__ out3;           // the last iteration's output, 3 floats per pixel
    int width, height, stride;
    float sigma_l, inv_n, inv_x;        // sigma_luminance as given (not halved per level); 1 / sigma^2 of the other two
    int on_l, on_n, on_x;               // 0: the term is off (sigma = +inf), never computed
};

// The tap loop both variance kernels share: denoise_taps' frame, key and X < 80 rules and its order, with the
// luminance term in the colour term's place and the variance accumulated beside the colours.  fetch as in denoise_taps;
// vfetch(dy, dx, qx, qy) returns (v, key as float bits) of the prefilter's tap (x + dx, y + dy), called only inside the
// frame.
template <class Fetch, class VFetch>
__device__ __forceinline__ float4 variance_taps(const VarianceFilterParams& D, int x, int y, float4 c, float4 g0, float4 g1,
                                                Fetch fetch, VFetch vfetch) {
    constexpr float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    constexpr float hg[3] = {0.25f, 0.5f, 0.25f};
    const int key = __float_as_int(g1.w);
    float inv_den = 0.f;
    if (D.on_l) {
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
        const float den = D.sigma_l * sqrtf(g) + 0x1p-20f;
        inv_den = 1.f / den;
    }
    const float lc = variance_lum(c.x, c.y, c.z);
    float ax = 0.f, ay = 0.f, az = 0.f, av = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float k = h[dy + 2] * h[dx + 2];
            if (dy == 0 && dx == 0) {
                ax = ax + k * c.x; ay = ay + k * c.y; az = az + k * c.z;
                av = av + (k * k) * c.w;
                sw = sw + k;
                continue;
            }
            const int qx = x + dx * D.stride, qy = y + dy * D.stride;
            if (qx < 0 || qx >= D.width || qy < 0 || qy >= D.height) continue;
            const float4 q1 = fetch(dy, dx, qx, qy, 2);
            if (__float_as_int(q1.w) != key) continue;
            const float4 qc = fetch(dy, dx, qx, qy, 0);
            float xc = 0.f, xn = 0.f, xx = 0.f;
            if (D.on_l) xc = fabsf(lc - variance_lum(qc.x, qc.y, qc.z)) * inv_den;
            if (D.on_n) xn = denoise_dist2(g0, fetch(dy, dx, qx, qy, 1)) * D.inv_n;
            if (D.on_x) xx = denoise_dist2(g1, q1) * D.inv_x;
            const float X = (xc + xn) + xx;
            if (!(X < 80.f)) continue;
            const float kw = k * denoise_exp_neg(X);
            ax = ax + kw * qc.x; ay = ay + kw * qc.y; az = az + kw * qc.z;
            av = av + (kw * kw) * qc.w;
            sw = sw + kw;
        }
    }
    return make_float4(ax / sw, ay / sw, az / sw, av / (sw * sw));
}

__device__ __forceinline__ void variance_store(const VarianceFilterParams& D, size_t pix, float4 o) {
    if (D.out3) { D.out3[3 * pix] = o.x; D.out3[3 * pix + 1] = o.y; D.out3[3 * pix + 2] = o.z; }
    else D.out[pix] = o;
}

// The prefilter's tap from global memory: the fourth lanes of the colour row and of the second guide row.
__device__ __forceinline__ float2 variance_vk_global(const VarianceFilterParams& D, int qx, int qy) {
    const size_t q = (size_t)qy * D.width + qx;          // inside the frame: the caller checked
    return make_float2(D.in[q].w, D.guides[2 * q + 1].w);
}

// The direct kernel: crt_denoise_direct_kernel's shape.  The yardstick; any stride.
__global__ __launch_bounds__(DENOISE_BX * DENOISE_DIRECT_BY) void crt_denoise_variance_direct_kernel(VarianceFilterParams D) {
    const int x = blockIdx.x * DENOISE_BX + threadIdx.x, y = blockIdx.y * DENOISE_DIRECT_BY + threadIdx.y;
    if (x >= D.width || y >= D.height) return;
    const size_t pix = (size_t)y * D.width + x;
    const float4 c = D.in[pix], g0 = D.guides[2 * pix], g1 = D.guides[2 * pix + 1];
    const float4 o = variance_taps(D, x, y, c, g0, g1,
        [&](int, int, int qx, int qy, int which) {
            const size_t q = (size_t)qy * D.width + qx;  // inside the frame: the tap loop checked
            return which == 0 ? D.in[q] : D.guides[2 * q + (which - 1)];
        },
        [&](int, int, int qx, int qy) { return variance_vk_global(D, qx, qy); });
    variance_store(D, pix, o);
}

// The tiled kernel: crt_denoise_tiled_kernel's staging, shape and LDS (12 (64 + 4 s) 48 B), the variance in the staged
// colour rows' fourth lane.  The prefilter's eight taps lie at +-1 pixel whatever the stride: at s = 1 they are among
// the staged rows and columns (j +- 1, x +- 1) and come from LDS; at s > 1 the rows y +- 1 belong to other residue
// classes, which this block does not stage, and all eight come from global memory (DESIGN.md §24 has the cost).
__global__ __launch_bounds__(DENOISE_BX * DENOISE_TY) void crt_denoise_variance_tiled_kernel(VarianceFilterParams D, int groups) {
    extern __shared__ float4 variance_lds[];
    const int s = D.stride, cols = DENOISE_BX + 4 * s, n = DENOISE_ROWS * cols;
    float4* l_c = variance_lds;
    float4* l_g0 = variance_lds + n;
    float4* l_g1 = variance_lds + 2 * n;
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
    const float4 o = variance_taps(D, x, y, l_c[at], l_g0[at], l_g1[at],
        [&](int dy, int dx, int, int, int which) {
            const int q = at + dy * cols + dx * s;       // row j + dy, column x + dx s of the staged block
            return which == 0 ? l_c[q] : which == 1 ? l_g0[q] : l_g1[q];
        },
        [&](int dy, int dx, int qx, int qy) {
            if (s == 1) { const int q = at + dy * cols + dx; return make_float2(l_c[q].w, l_g1[q].w); }
            return variance_vk_global(D, qx, qy);
        });
    variance_store(D, (size_t)y * D.width + x, o);
}

namespace {

int variance_state(crt_renderer* R, VarianceState** out) {
    if (!R->variance) {
        R->variance.reset(new (std::nothrow) VarianceState);     // whatever it comes to hold is freed with the handle
        if (!R->variance) return set_error(CRT_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    *out = R->variance.get();
    return CRT_OK;
}

// The moment buffers, on the first call that needs them.
int variance_moment_buffers(crt_renderer* R, VarianceState* V) {
    const size_t n_pix = (size_t)R->width * R->height;
    for (DevBuf<float2>& b : V->mom)
        if (!b) HIP_TRY(b.alloc(n_pix));
    return CRT_OK;
}

// The checks of the options alone (no handle, no device).
int variance_check_options(const crt_denoise_variance_options* o, const char* who) {
    const std::string w = who;
    if (!o) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": null options");
    if (o->iterations < 0 || o->iterations > 8) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": iterations must be 0..8 (0 = 5)");
    const float sig[3] = {o->sigma_luminance, o->sigma_normal, o->sigma_position};
    const char* name[3] = {"sigma_luminance", "sigma_normal", "sigma_position"};
    for (int k = 0; k < 3; ++k)
        if (!(sig[k] == __builtin_inff() || (sig[k] >= 0x1p-50f && sig[k] <= 0x1p50f)))
            return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": " + name[k] + " must be in [2^-50, 2^50] or +inf (that term off)");
    if (!(o->min_history >= 1.f && o->min_history <= 0x1p24f))
        return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": min_history must be in [1, 2^24]");
    if (o->flags & ~CRT_DENOISE_DIRECT_ONLY) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": unknown flag bits");
    if (o->reserved != 0) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": reserved must be 0");
    return CRT_OK;
}

// crt_renderer_reproject_moments' launch: reproject_run with the moments beside the history.
int reproject_moments_run(crt_renderer* R, DenoiseState* N, ReprojectState* S, VarianceState* V,
                          const crt_reproject_options* o, float scale, hipStream_t st) {
    ReprojectMomentsParams M{};
    M.P = reproject_params(R, N, S, o, scale);
    M.P.valid = S->valid && V->moments_valid;            // a history without moments starts over as a whole
    M.mom_in = V->mom[V->mi].get();
    M.mom_out = V->mom[V->mi ^ 1].get();
    HIP_TRY(hipEventRecord(S->e0.get(), st));
    hipLaunchKernelGGL(crt_reproject_moments_kernel, dim3(M.P.blocks_x, (R->height + REPROJECT_BY - 1) / REPROJECT_BY),
                       dim3(REPROJECT_BX, REPROJECT_BY), 0, st, M);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S->e1.get(), st));
    reproject_advance(N, S);
    V->mi ^= 1;
    V->moments_valid = true;
    return CRT_OK;
}

// The estimate and the filter on `st`.  Options, history, moments and guides were checked; c_0 goes to col[0].
int variance_run(crt_renderer* R, DenoiseState* N, ReprojectState* S, VarianceState* V,
                 const crt_denoise_variance_options* o, hipStream_t st, bool timed) {
    const int W = R->width, H = R->height, n_pix = W * H;
    const int iterations = o->iterations ? o->iterations : 5;
    const bool direct_only = (o->flags & CRT_DENOISE_DIRECT_ONLY) != 0;
    HIP_TRY(hipEventRecord(N->f0.get(), st));
    hipLaunchKernelGGL(crt_variance_estimate_kernel, dim3((n_pix + 255) / 256), dim3(256), 0, st, S->hist[S->hi].get(),
                       V->mom[V->mi].get(), N->guides[N->gi].get(), N->col[0].get(), V->variance.get(), W, H, o->min_history);
    N->timed_iterations = 0;
    if (timed) HIP_TRY(hipEventRecord(N->it[0].get(), st));
    VarianceFilterParams D{};
    D.guides = N->guides[N->gi].get();
    D.width = W; D.height = H;
    const float inf = __builtin_inff();
    D.on_l = o->sigma_luminance != inf; D.on_n = o->sigma_normal != inf; D.on_x = o->sigma_position != inf;
    D.sigma_l = D.on_l ? o->sigma_luminance : 0.f;
    D.inv_n = D.on_n ? 1.f / (o->sigma_normal * o->sigma_normal) : 0.f;
    D.inv_x = D.on_x ? 1.f / (o->sigma_position * o->sigma_position) : 0.f;
    for (int i = 0; i < iterations; ++i) {
        const bool last = i == iterations - 1;
        D.in = N->col[i & 1].get();
        D.out = last ? nullptr : N->col[(i + 1) & 1].get();
        D.out3 = last ? N->denoised.get() : nullptr;
        D.stride = 1 << i;
        if (!direct_only && D.stride <= DENOISE_TILED_MAX_STRIDE) {
            const int s = D.stride, rows = (H + s - 1) / s;                   // the rows of residue class 0, the longest
            const int groups = (rows + DENOISE_TY - 1) / DENOISE_TY;
            const size_t lds = (size_t)DENOISE_ROWS * (DENOISE_BX + 4 * s) * 48;
            if (lds > 65536 && !V->lds_raised) {
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(crt_denoise_variance_tiled_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize,
                                            DENOISE_ROWS * (DENOISE_BX + 4 * DENOISE_TILED_MAX_STRIDE) * 48));
                V->lds_raised = true;
            }
            hipLaunchKernelGGL(crt_denoise_variance_tiled_kernel, dim3((W + DENOISE_BX - 1) / DENOISE_BX, s * groups),
                               dim3(DENOISE_BX, DENOISE_TY), lds, st, D, groups);
        } else {
            hipLaunchKernelGGL(crt_denoise_variance_direct_kernel,
                               dim3((W + DENOISE_BX - 1) / DENOISE_BX, (H + DENOISE_DIRECT_BY - 1) / DENOISE_DIRECT_BY),
                               dim3(DENOISE_BX, DENOISE_DIRECT_BY), 0, st, D);
        }
        if (timed) HIP_TRY(hipEventRecord(N->it[i + 1].get(), st));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(N->f1.get(), st));
    if (timed) N->timed_iterations = iterations;
    N->have_denoised = true;
    V->have_variance = true;
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_renderer_reproject_moments(crt_renderer* R, const crt_reproject_options* o, float scale, crt_reproject_stats* stats_out,
                                   void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "reproject moments: null renderer");
    if (int rc = reproject_check_options(o, "reproject moments")) return rc;
    if (!(scale > 0.f)) return set_error(CRT_ERR_INVALID_ARGUMENT, "reproject moments: scale must be > 0");
    if (R->tile_shards > 1) return set_error(CRT_ERR_UNSUPPORTED, "reproject moments: a pixel shard other than (0, 1)");
    if (!R->denoise || !R->denoise->have_guides)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "reproject moments: no guides computed yet (crt_renderer_compute_guides)");
    HIP_TRY(hipSetDevice(R->device));
    DenoiseState* N = R->denoise.get();
    ReprojectState* S = nullptr;
    if (int rc = reproject_state(R, &S)) return rc;
    VarianceState* V = nullptr;
    if (int rc = variance_state(R, &V)) return rc;
    if (int rc = variance_moment_buffers(R, V)) return rc;
    if (int rc = reproject_moments_run(R, N, S, V, o, scale, (hipStream_t)stream)) return rc;
    return stats_out ? reproject_stats(R, N, S, stats_out) : CRT_OK;
}

int crt_renderer_read_moments(crt_renderer* R, float* out) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "read moments: null argument");
    if (!R->variance || !R->variance->moments_valid)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "read moments: no valid moments on this renderer (crt_renderer_reproject_moments)");
    return read_dev(R, out, R->variance->mom[R->variance->mi].get(), (size_t)R->width * R->height * 8);
}

int crt_renderer_denoise_history_variance(crt_renderer* R, const crt_denoise_variance_options* o, crt_denoise_stats* stats_out,
                                          void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise history variance: null renderer");
    if (int rc = variance_check_options(o, "denoise history variance")) return rc;
    if (R->tile_shards > 1) return set_error(CRT_ERR_UNSUPPORTED, "denoise history variance: a pixel shard other than (0, 1)");
    if (!R->reproject || !R->reproject->have_history)
        return set_error(CRT_ERR_INVALID_ARGUMENT,
                         "denoise history variance: no history on this renderer yet (crt_renderer_reproject_moments)");
    if (!R->variance || !R->variance->moments_valid)
        return set_error(CRT_ERR_INVALID_ARGUMENT,
                         "denoise history variance: the history has no valid moments (crt_renderer_reproject_moments makes them)");
    HIP_TRY(hipSetDevice(R->device));
    DenoiseState* N = R->denoise.get();              // exists: the reprojection needed its guides
    ReprojectState* S = R->reproject.get();
    VarianceState* V = R->variance.get();
    if (!V->variance) HIP_TRY(V->variance.alloc((size_t)R->width * R->height));
    if (int rc = variance_run(R, N, S, V, o, (hipStream_t)stream, stats_out != nullptr)) return rc;
    if (!stats_out) return CRT_OK;
    crt_denoise_options plain{};
    plain.iterations = o->iterations;
    return denoise_stats(R, N, &plain, stats_out);
}

int crt_renderer_read_variance(crt_renderer* R, float* out) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "read variance: null argument");
    if (!R->variance || !R->variance->have_variance)
        return set_error(CRT_ERR_INVALID_ARGUMENT,
                         "read variance: no variance on this renderer yet (crt_renderer_denoise_history_variance)");
    return read_dev(R, out, R->variance->variance.get(), (size_t)R->width * R->height * 4);
}

// crt_selftest_reproject with the moments beside the history.
int crt_selftest_reproject_moments(crt_renderer* R, const float* color, const float* guides, const float* prev_guides,
                                   const float* prev_history, const float* prev_moments, const crt_camera_desc* prev_camera,
                                   const crt_reproject_options* o, float* out_history, float* out_moments) {
    if (!R || !color || !guides || !prev_guides || !prev_camera || !out_history || !out_moments)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "selftest reproject moments: null argument");
    if (prev_history && !prev_moments)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "selftest reproject moments: null prev_moments with a previous history");
    if (int rc = reproject_check_options(o, "selftest reproject moments")) return rc;
    HIP_TRY(hipSetDevice(R->device));
    DenoiseState* N = nullptr;
    if (int rc = denoise_state(R, &N)) return rc;
    ReprojectState* S = nullptr;
    if (int rc = reproject_state(R, &S)) return rc;
    VarianceState* V = nullptr;
    if (int rc = variance_state(R, &V)) return rc;
    if (int rc = variance_moment_buffers(R, V)) return rc;
    const size_t n_pix = (size_t)R->width * R->height;
    N->keep = false;
    S->prev_gi = N->gi ^ 1;
    HIP_TRY(hipMemcpy(R->d_sum, color, n_pix * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->guides[N->gi].get(), guides, n_pix * 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->guides[S->prev_gi].get(), prev_guides, n_pix * 32, hipMemcpyHostToDevice));
    if (prev_history) {
        HIP_TRY(hipMemcpy(S->hist[S->hi].get(), prev_history, n_pix * 16, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(V->mom[V->mi].get(), prev_moments, n_pix * 8, hipMemcpyHostToDevice));
    }
    N->have_guides = true;
    N->counted = N->timed_guides = false;
    N->guide_cam = *prev_camera;
    S->prev_cam = *prev_camera;
    S->valid = V->moments_valid = prev_history != nullptr;
    if (int rc = reproject_moments_run(R, N, S, V, o, 1.f, 0)) return rc;
    HIP_TRY(hipStreamSynchronize(0));
    HIP_TRY(hipMemcpy(out_history, S->hist[S->hi].get(), n_pix * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_moments, V->mom[V->mi].get(), n_pix * 8, hipMemcpyDeviceToHost));
    return CRT_OK;
}

// The estimate and the filter on caller-supplied buffers: the renderer's own state and the host function
// crt_renderer_denoise_history_variance calls, on the null stream.  The uploaded history has no previous frame: a
// reprojection after this starts over.
int crt_selftest_denoise_variance(crt_renderer* R, const float* history, const float* moments, const float* guides,
                                  const crt_denoise_variance_options* o, float* out, float* out_variance) {
    if (!R || !history || !moments || !guides || !out || !out_variance)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "selftest denoise variance: null argument");
    if (int rc = variance_check_options(o, "selftest denoise variance")) return rc;
    HIP_TRY(hipSetDevice(R->device));
    DenoiseState* N = nullptr;
    if (int rc = denoise_state(R, &N)) return rc;
    ReprojectState* S = nullptr;
    if (int rc = reproject_state(R, &S)) return rc;
    VarianceState* V = nullptr;
    if (int rc = variance_state(R, &V)) return rc;
    if (int rc = variance_moment_buffers(R, V)) return rc;
    const size_t n_pix = (size_t)R->width * R->height;
    if (!V->variance) HIP_TRY(V->variance.alloc(n_pix));
    denoise_next_guides(N);
    HIP_TRY(hipMemcpy(N->guides[N->gi].get(), guides, n_pix * 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(S->hist[S->hi].get(), history, n_pix * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(V->mom[V->mi].get(), moments, n_pix * 8, hipMemcpyHostToDevice));
    N->have_guides = true;
    N->counted = N->timed_guides = false;
    N->guide_cam = crt_camera_desc{};                // no camera made these guides: a reprojection after this restarts
    S->valid = false;
    S->have_history = true;
    V->moments_valid = false;
    if (int rc = variance_run(R, N, S, V, o, 0, false)) return rc;
    HIP_TRY(hipStreamSynchronize(0));
    HIP_TRY(hipMemcpy(out, N->denoised.get(), n_pix * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_variance, V->variance.get(), n_pix * 4, hipMemcpyDeviceToHost));
    return CRT_OK;
}

}  // extern "C"
