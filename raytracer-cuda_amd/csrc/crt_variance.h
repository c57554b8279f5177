// Variance-guided filtering of the history (Schied et al., HPG 2017): the first two luminance moments
// carried through the reprojection, a per-pixel variance from them, and an a-trous filter whose luminance edge-stop is
// as wide as that variance, itself filtered, says.  Included by crt_hip.hip after crt_reproject.h.  Nothing here is used
// by a render kernel.  The moments ride in crt_reproject.h's one reprojection body (MOMENTS), and the filter is
// crt_denoise.h's tap loop, kernel bodies and host launch loop in their variance mode (VAR); what is only here is the
// estimate kernel and the entries.
//
// Every operation is f32 and uncontracted and in the order the header states, so tests/helpers/variance_model.py
// reproduces the bits.  The variance rides in the fourth lane of the filter's 16-B colour rows, in global memory and in
// the tiled kernel's LDS, so the filter moves the bytes the plain one moves, plus the prefilter's taps.
#pragma once

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

namespace {

// The checks of the options alone (no handle, no device).
int variance_check_options(const crt_denoise_variance_options* o, const char* who) {
    const std::string w = who;
    if (!o) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": null options");
    if (int rc = denoise_check_sigmas(w, o->iterations, "sigma_luminance", o->sigma_luminance, o->sigma_normal, o->sigma_position))
        return rc;
    if (!(o->min_history >= 1.f && o->min_history <= 0x1p24f))
        return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": min_history must be in [1, 2^24]");
    if (o->flags & ~CRT_DENOISE_DIRECT_ONLY) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": unknown flag bits");
    if (o->reserved != 0) return set_error(CRT_ERR_INVALID_ARGUMENT, w + ": reserved must be 0");
    return CRT_OK;
}

// The estimate and the filter on `st`.  Options, history, moments and guides were checked; c_0 goes to col[0].
int variance_run(crt_renderer* R, DenoiseState* N, ReprojectState* S, VarianceState* V,
                 const crt_denoise_variance_options* o, hipStream_t st, bool timed) {
    const int W = R->width, H = R->height, n_pix = W * H;
    HIP_TRY(hipEventRecord(N->f0.get(), st));
    hipLaunchKernelGGL(crt_variance_estimate_kernel, dim3((n_pix + 255) / 256), dim3(256), 0, st, S->hist[S->hi].get(),
                       V->mom[V->mi].get(), N->guides[N->gi].get(), N->col[0].get(), V->variance.get(), W, H, o->min_history);
    const float sigma[3] = {o->sigma_luminance, o->sigma_normal, o->sigma_position};
    const DenoiseFilter F{crt_denoise_variance_tiled_kernel, crt_denoise_variance_direct_kernel, &V->lds_raised, false};
    if (int rc = denoise_iterations(R, N, F, sigma, o->iterations, o->flags, nullptr, st, timed)) return rc;
    V->have_variance = true;
    return CRT_OK;
}

}  // namespace

extern "C" {

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
    if (int rc = denoise_state(R, 0, &N)) return rc;
    ReprojectState* S = nullptr;
    if (int rc = reproject_state(R, &S)) return rc;
    VarianceState* V = nullptr;
    if (int rc = reproject_moments_state(R, &V)) return rc;
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
