// Reprojection of a frame's history across camera moves, guided by the denoiser's first-hit buffers.
// Included by crt_hip.hip after crt_denoise.h.  Nothing here is used by a render kernel.
//
// History: one 16-B row (r, g, b, len) per pixel in a ping-pong pair.  One kernel per frame: every hit pixel projects
// its first-hit position into the previous guide camera, takes the (up to) four bilinear taps of the previous history
// whose previous guide vouches for them (same key, position within a relative distance, optionally the normal), and
// blends its own 1-frame estimate c = scale * sum into their mean with weight 1 / min(len + 1, max_history).  Every
// operation is f32 and uncontracted and in the order the header states, so tests/helpers/reproject_model.py reproduces
// the bits.  The previous guides are not copied: the denoiser state holds two guide buffers behind an index, and the
// one a reprojection has read as "current" is kept as the next call's "previous" (DenoiseState::keep).
#pragma once

struct ReprojectParams {
    const float* __restrict__ sum;          // W*H*3
    const float4* __restrict__ guides;      // the current frame's, 2 rows per pixel
    const float4* __restrict__ prev_guides; // the previous frame's
    const float4* __restrict__ hist_in;     // the previous history, 1 row per pixel
    float4* __restrict__ hist_out;
    uint32_t* __restrict__ wave_taken;      // per wave: pixels with sw > 0
    int width, height, blocks_x;
    float scale;
    int valid;                              // 0: no previous frame, every pixel restarts
    int on_x, on_n;                         // 0: the term is off, never computed
    float o[3], L[3], N[3], hor[3], ver[3]; // the previous guide camera: origin, lower_left - origin, cross(hor, ver)
    float LN, hh, vv, tol2, normal_min, max_history;
};

__device__ __forceinline__ float reproject_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

__device__ __forceinline__ bool reproject_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// One lane per pixel, 64 consecutive x per wave (the direct denoise kernel's block shape).  The pixel's own sum, guide
// rows and output row are coalesced; the taps are a gather whose four addresses are neighbours of the neighbouring
// lanes'.  The four previous (position, key) rows are loaded together from clamped, always valid addresses before any
// of them is tested; the previous normal rows only with the normal term on, the history rows only for taps that passed.
// MOMENTS: the first two luminance moments ride along.  They take exactly the taps the colours took, with the colours'
// weights, sum and blend factor, and their rows are loaded with the history rows.
constexpr int REPROJECT_BX = 64, REPROJECT_BY = 4;
template <bool MOMENTS>
__device__ __forceinline__ void reproject_body(const ReprojectParams& P, const float2* __restrict__ mom_in,
                                               float2* __restrict__ mom_out) {
    const int x = blockIdx.x * REPROJECT_BX + threadIdx.x, y = blockIdx.y * REPROJECT_BY + threadIdx.y;
    const int W = P.width, H = P.height;
    bool took = false;
    if (x < W && y < H) {
        const size_t pix = (size_t)y * W + x;
        const float4 g1 = P.guides[2 * pix + 1];
        const float cx = P.scale * P.sum[3 * pix], cy = P.scale * P.sum[3 * pix + 1], cz = P.scale * P.sum[3 * pix + 2];
        float4 out = make_float4(cx, cy, cz, 1.f);
        float l = 0.f, l2 = 0.f;
        if constexpr (MOMENTS) { l = variance_lum(cx, cy, cz); l2 = l * l; }
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
                    if (ok[k]) {
                        hr[k] = P.hist_in[q[k]];
                        if constexpr (MOMENTS) mr[k] = mom_in[q[k]];
                    }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (ok[k] && reproject_finite(hr[k].x) && reproject_finite(hr[k].y) && reproject_finite(hr[k].z)) {
                        acc.x = acc.x + w[k] * hr[k].x; acc.y = acc.y + w[k] * hr[k].y;
                        acc.z = acc.z + w[k] * hr[k].z; acc.w = acc.w + w[k] * hr[k].w;
                        if constexpr (MOMENTS) { am.x = am.x + w[k] * mr[k].x; am.y = am.y + w[k] * mr[k].y; }
                        sw = sw + w[k];
                    }
                if (sw > 0.f) {
                    const float hx = acc.x / sw, hy = acc.y / sw, hz = acc.z / sw, hl = acc.w / sw;
                    const float m = fminf(hl + 1.f, P.max_history);
                    const float a = 1.f / m;
                    out = make_float4(hx + (cx - hx) * a, hy + (cy - hy) * a, hz + (cz - hz) * a, m);
                    if constexpr (MOMENTS) {
                        const float h1 = am.x / sw, h2 = am.y / sw;
                        om = make_float2(h1 + (l - h1) * a, h2 + (l2 - h2) * a);
                    }
                    took = true;
                }
            }
        }
        P.hist_out[pix] = out;
        if constexpr (MOMENTS) mom_out[pix] = om;
    }
    const unsigned long long taken = __ballot(took);
    if (threadIdx.x == 0 && y < H) P.wave_taken[(size_t)y * P.blocks_x + blockIdx.x] = (uint32_t)__popcll(taken);
}

__global__ __launch_bounds__(REPROJECT_BX * REPROJECT_BY) void crt_reproject_kernel(ReprojectParams P) {
    reproject_body<false>(P, nullptr, nullptr);
}

struct ReprojectMomentsParams {
    ReprojectParams P;
    const float2* __restrict__ mom_in;      // the previous moments, 1 row per pixel
    float2* __restrict__ mom_out;
};

__global__ __launch_bounds__(REPROJECT_BX * REPROJECT_BY) void crt_reproject_moments_kernel(ReprojectMomentsParams M) {
    reproject_body<true>(M.P, M.mom_in, M.mom_out);
}

// writeColor of rows (r, g, b, *) with scale 1: crt_resolve_kernel's operations on 16-B rows.
__global__ __launch_bounds__(256) void crt_resolve_rows_kernel(const float4* __restrict__ rows, uint8_t* __restrict__ rgba,
                                                               int n_pix) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n_pix) return;
    const float4 c = rows[pix];
    uchar4 o;
    o.x = to_u8(1.f * c.x); o.y = to_u8(1.f * c.y); o.z = to_u8(1.f * c.z); o.w = 255;
    reinterpret_cast<uchar4*>(rgba)[pix] = o;
}

namespace {

int reproject_waves(const crt_renderer* R) { return ((R->width + REPROJECT_BX - 1) / REPROJECT_BX) * R->height; }

// The handle's denoiser state must exist (the guides live there).
int reproject_state(crt_renderer* R, ReprojectState** out) {
    DenoiseState* N = R->denoise.get();
    return first_use(R->reproject, "the reprojection state of this renderer could not be allocated", out, [&](ReprojectState* P) -> int {
        const size_t n_pix = (size_t)R->width * R->height;
        HIP_TRY(P->hist[0].alloc(n_pix));
        HIP_TRY(P->hist[1].alloc(n_pix));
        HIP_TRY(P->wave_taken.alloc((size_t)reproject_waves(R)));
        if (!N->guides[1]) HIP_TRY(N->guides[1].alloc(n_pix * 2));
        HIP_TRY(P->e0.create());
        HIP_TRY(P->e1.create());
        return CRT_OK;
    });
}

// The checks of the options alone (no handle, no device).
int reproject_check_options(const crt_reproject_options* o, const char* who) {
    const std::string w = who;
    const float inf = __builtin_inff();
    if (!o) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": null options");
    if (!(o->position_tolerance == inf || (o->position_tolerance >= 0x1p-50f && o->position_tolerance <= 0x1p50f)))
        return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": position_tolerance must be in [2^-50, 2^50] or +inf (that term off)");
    if (!(o->normal_min == -inf || (o->normal_min >= -1.f && o->normal_min <= 1.f)))
        return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": normal_min must be in [-1, 1] or -inf (that term off)");
    if (!(o->max_history >= 1.f && o->max_history <= 0x1p24f))
        return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": max_history must be in [1, 2^24]");
    if (o->flags != 0) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": unknown flag bits");
    if (o->reserved != 0) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": reserved must be 0");
    return CRT_OK;
}

// The variance state (crt_variance.h) with its moment buffers, for a reprojection that carries the moments.
int reproject_moments_state(crt_renderer* R, VarianceState** out) {
    if (!R->variance)
        if (int rc = new_state(R->variance)) return rc;
    for (DevBuf<float2>& b : R->variance->mom)
        if (!b) HIP_TRY(b.alloc((size_t)R->width * R->height));
    *out = R->variance.get();
    return CRT_OK;
}

// The kernels' parameters for one call.  Options, guides and state were checked.
ReprojectParams reproject_params(crt_renderer* R, DenoiseState* N, ReprojectState* S, const crt_reproject_options* o,
                                 float scale) {
    const float inf = __builtin_inff();
    ReprojectParams P{};
    P.sum = R->d_sum;
    P.guides = N->guides[N->gi].get();
    P.prev_guides = N->guides[S->prev_gi].get();
    P.hist_in = S->hist[S->hi].get();
    P.hist_out = S->hist[S->hi ^ 1].get();
    P.wave_taken = S->wave_taken.get();
    P.width = R->width; P.height = R->height; P.blocks_x = (R->width + REPROJECT_BX - 1) / REPROJECT_BX;
    P.scale = scale;
    P.valid = S->valid;
    P.on_x = o->position_tolerance != inf;
    P.on_n = o->normal_min != -inf;
    const crt_camera_desc& c = S->prev_cam;
    for (int a = 0; a < 3; ++a) {
        P.o[a] = c.origin[a]; P.hor[a] = c.horizontal[a]; P.ver[a] = c.vertical[a];
        P.L[a] = c.lower_left[a] - c.origin[a];
    }
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, d = (a + 2) % 3;
        const float p0 = P.hor[b] * P.ver[d], p1 = P.hor[d] * P.ver[b];
        P.N[a] = p0 - p1;
    }
    auto dot = [](const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    P.LN = dot(P.L, P.N); P.hh = dot(P.hor, P.hor); P.vv = dot(P.ver, P.ver);
    P.tol2 = P.on_x ? o->position_tolerance * o->position_tolerance : 0.f;
    P.normal_min = o->normal_min;
    P.max_history = o->max_history;
    return P;
}

// After a call's launch: the current frame becomes the previous one.
void reproject_advance(DenoiseState* N, ReprojectState* S) {
    S->hi ^= 1;
    S->prev_gi = N->gi;
    S->prev_cam = N->guide_cam;
    N->keep = true;
    S->valid = S->have_history = true;
}

// One reprojection on `st`: the launch, then the current frame becomes the previous one.  Options, guides and state
// were checked.  V non-null: the moments ride beside the history (its buffers exist); null: this history has none.
int reproject_run(crt_renderer* R, DenoiseState* N, ReprojectState* S, VarianceState* V, const crt_reproject_options* o,
                  float scale, hipStream_t st) {
    ReprojectMomentsParams M{};
    M.P = reproject_params(R, N, S, o, scale);
    const dim3 grid(M.P.blocks_x, (R->height + REPROJECT_BY - 1) / REPROJECT_BY), block(REPROJECT_BX, REPROJECT_BY);
    HIP_TRY(hipEventRecord(S->e0.get(), st));
    if (V) {
        M.P.valid = S->valid && V->moments_valid;            // a history without moments starts over as a whole
        M.mom_in = V->mom[V->mi].get();
        M.mom_out = V->mom[V->mi ^ 1].get();
        hipLaunchKernelGGL(crt_reproject_moments_kernel, grid, block, 0, st, M);
    } else {
        hipLaunchKernelGGL(crt_reproject_kernel, grid, block, 0, st, M.P);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S->e1.get(), st));
    reproject_advance(N, S);
    if (V) { V->mi ^= 1; V->moments_valid = true; }
    return CRT_OK;
}

// The stats of the reprojection just enqueued: waits for its launch.
int reproject_stats(crt_renderer* R, DenoiseState* N, ReprojectState* S, crt_reproject_stats* out) {
    crt_reproject_stats s{};
    HIP_TRY(hipEventSynchronize(S->e1.get()));
    HIP_TRY(hipEventElapsedTime(&s.reproject_ms, S->e0.get(), S->e1.get()));
    std::vector<uint32_t> w((size_t)reproject_waves(R));
    HIP_TRY(hipMemcpy(w.data(), S->wave_taken.get(), w.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t c : w) s.pixels_reprojected += c;
    if (N->counted)
        if (int rc = denoise_pixels_hit(R, N, &s.pixels_hit)) return rc;
    *out = s;
    return CRT_OK;
}

// crt_renderer_reproject and, with `moments`, crt_renderer_reproject_moments; `who` prefixes the refusals.
int reproject_entry(crt_renderer* R, const char* who, bool moments, const crt_reproject_options* o, float scale,
                    crt_reproject_stats* stats_out, void* stream) {
    const std::string w = who;
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": null renderer");
    if (int rc = reproject_check_options(o, who)) return rc;
    if (!(scale > 0.f)) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": scale must be > 0");
    if (R->tile_shards > 1) return set_error(CRT_ERR_UNSUPPORTED, w + ": a pixel shard other than (0, 1)");
    if (!R->denoise || !R->denoise->have_guides)
        return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": no guides computed yet (crt_renderer_compute_guides)");
    HIP_TRY(hipSetDevice(R->device));
    DenoiseState* N = R->denoise.get();
    ReprojectState* S = nullptr;
    if (int rc = reproject_state(R, &S)) return rc;
    VarianceState* V = nullptr;
    if (moments) {
        if (int rc = reproject_moments_state(R, &V)) return rc;
    } else if (R->variance) {
        R->variance->moments_valid = false;                  // this history has no moments (crt_variance.h)
    }
    if (int rc = reproject_run(R, N, S, V, o, scale, (hipStream_t)stream)) return rc;
    return stats_out ? reproject_stats(R, N, S, stats_out) : CRT_OK;
}

// crt_selftest_reproject and, with `moments`, crt_selftest_reproject_moments: the reprojection on caller-supplied
// buffers, through the renderer's own state and the host function the entries above call, on the null stream.  The
// colours go into the renderer's linear buffer and are taken with scale 1.
int reproject_selftest(crt_renderer* R, const char* who, bool moments, const float* color, const float* guides,
                       const float* prev_guides, const float* prev_history, const float* prev_moments,
                       const crt_camera_desc* prev_camera, const crt_reproject_options* o, float* out_history,
                       float* out_moments) {
    const std::string w = who;
    if (!R || !color || !guides || !prev_guides || !prev_camera || !out_history || (moments && !out_moments))
        return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": null argument");
    if (moments && prev_history && !prev_moments)
        return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": null prev_moments with a previous history");
    if (int rc = reproject_check_options(o, who)) return rc;
    HIP_TRY(hipSetDevice(R->device));
    DenoiseState* N = nullptr;
    if (int rc = denoise_state(R, 0, &N)) return rc;
    ReprojectState* S = nullptr;
    if (int rc = reproject_state(R, &S)) return rc;
    VarianceState* V = nullptr;
    if (moments)
        if (int rc = reproject_moments_state(R, &V)) return rc;
    const size_t n_pix = (size_t)R->width * R->height;
    N->keep = false;
    S->prev_gi = N->gi ^ 1;
    HIP_TRY(hipMemcpy(R->d_sum, color, n_pix * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->guides[N->gi].get(), guides, n_pix * 32, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(N->guides[S->prev_gi].get(), prev_guides, n_pix * 32, hipMemcpyHostToDevice));
    if (prev_history) HIP_TRY(hipMemcpy(S->hist[S->hi].get(), prev_history, n_pix * 16, hipMemcpyHostToDevice));
    if (V && prev_history) HIP_TRY(hipMemcpy(V->mom[V->mi].get(), prev_moments, n_pix * 8, hipMemcpyHostToDevice));
    N->have_guides = true;
    N->counted = N->timed_guides = false;
    N->guide_cam = *prev_camera;
    S->prev_cam = *prev_camera;
    S->valid = prev_history != nullptr;
    if (V) V->moments_valid = S->valid;
    if (int rc = reproject_run(R, N, S, V, o, 1.f, 0)) return rc;
    HIP_TRY(hipStreamSynchronize(0));
    HIP_TRY(hipMemcpy(out_history, S->hist[S->hi].get(), n_pix * 16, hipMemcpyDeviceToHost));
    if (V) HIP_TRY(hipMemcpy(out_moments, V->mom[V->mi].get(), n_pix * 8, hipMemcpyDeviceToHost));
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_renderer_reproject(crt_renderer* R, const crt_reproject_options* o, float scale, crt_reproject_stats* stats_out,
                           void* stream) {
    return reproject_entry(R, "reproject", false, o, scale, stats_out, stream);
}

int crt_renderer_reproject_moments(crt_renderer* R, const crt_reproject_options* o, float scale, crt_reproject_stats* stats_out,
                                   void* stream) {
    return reproject_entry(R, "reproject moments", true, o, scale, stats_out, stream);
}

int crt_renderer_reset_history(crt_renderer* R) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "reset history: null renderer");
    if (R->reproject) R->reproject->valid = false;
    if (R->variance) R->variance->moments_valid = false;
    return CRT_OK;
}

int crt_renderer_denoise_history(crt_renderer* R, const crt_denoise_options* o, crt_denoise_stats* stats_out, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise history: null renderer");
    if (int rc = denoise_check_options(o, "denoise history")) return rc;
    if (o->flags & CRT_DENOISE_TILE_SCALE)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise history: takes the history colours as they are (no tile scale)");
    if (R->tile_shards > 1) return set_error(CRT_ERR_UNSUPPORTED, "denoise history: a pixel shard other than (0, 1)");
    if (!R->reproject || !R->reproject->have_history)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "denoise history: no history on this renderer yet (crt_renderer_reproject)");
    HIP_TRY(hipSetDevice(R->device));
    DenoiseState* N = R->denoise.get();              // exists: the reprojection needed its guides
    ReprojectState* S = R->reproject.get();
    if (int rc = denoise_run(R, N, o, 1.f, (hipStream_t)stream, stats_out != nullptr, S->hist[S->hi].get())) return rc;
    return stats_out ? denoise_stats(R, N, o, stats_out) : CRT_OK;
}

int crt_renderer_resolve_history(crt_renderer* R, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    if (!R->reproject || !R->reproject->have_history)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "resolve history: no history on this renderer yet");
    HIP_TRY(hipSetDevice(R->device));
    const int n = R->width * R->height;
    hipLaunchKernelGGL(crt_resolve_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       R->reproject->hist[R->reproject->hi].get(), R->d_rgba.get(), n);
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

int crt_renderer_read_history(crt_renderer* R, float* out) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "read history: null argument");
    if (!R->reproject || !R->reproject->have_history)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "read history: no history on this renderer yet");
    return read_dev(R, out, R->reproject->hist[R->reproject->hi].get(), (size_t)R->width * R->height * 16);
}

float* crt_renderer_history_device_ptr(crt_renderer* R) {
    return R && R->reproject && R->reproject->have_history
               ? reinterpret_cast<float*>(R->reproject->hist[R->reproject->hi].get()) : nullptr;
}

int crt_selftest_reproject(crt_renderer* R, const float* color, const float* guides, const float* prev_guides,
                           const float* prev_history, const crt_camera_desc* prev_camera, const crt_reproject_options* o,
                           float* out_history) {
    return reproject_selftest(R, "selftest reproject", false, color, guides, prev_guides, prev_history, nullptr, prev_camera, o,
                              out_history, nullptr);
}

int crt_selftest_reproject_moments(crt_renderer* R, const float* color, const float* guides, const float* prev_guides,
                                   const float* prev_history, const float* prev_moments, const crt_camera_desc* prev_camera,
                                   const crt_reproject_options* o, float* out_history, float* out_moments) {
    return reproject_selftest(R, "selftest reproject moments", true, color, guides, prev_guides, prev_history, prev_moments,
                              prev_camera, o, out_history, out_moments);
}

}  // extern "C"
