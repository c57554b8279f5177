// crt_selftest.h — the host side of the core's self-tests: the entries that run crt_hip.hip's self-test kernels (the
// arithmetic, the wave scans, the primitive tests, the camera ray, the material step, the XORWOW draws) on caller-supplied
// inputs, then the entries that run the schedule stages of crt_dispatch.h on caller-supplied costs.  Host code only.
// Included by crt_hip.hip after crt_dispatch.h; needs crt_renderer.h's seq_tables and uv_div_mismatches.
#pragma once

extern "C" {

int crt_selftest_uv_div(int dim, unsigned long long* mismatches) {
    if (dim <= 0 || !mismatches) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = use_device(0)) return rc;
    return uv_div_mismatches(dim, mismatches);
}

int crt_selftest_math(const float* a, const float* b, int n, float* out, double* out64) {
    if (!a || !b || !out || !out64 || n <= 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = use_device(0)) return rc;
    DevBuf<float> da, db, dout;
    DevBuf<double> d64;
    HIP_TRY(da.alloc(n));
    HIP_TRY(db.alloc(n));
    HIP_TRY(dout.alloc(n * 4));
    HIP_TRY(d64.alloc(n * 2));
    HIP_TRY(hipMemcpy(da.get(), a, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db.get(), b, n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(crt_selftest_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, da.get(), db.get(), n, dout.get(),
                       d64.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.get(), n * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out64, d64.get(), n * 16, hipMemcpyDeviceToHost));
    return CRT_OK;
}

// crt_selftest_rcp / crt_selftest_sqrt: `kernel` over the f32 bit patterns [lo_bits, hi_bits].
static int selftest_bit_range(void (*kernel)(uint32_t, uint32_t, unsigned long long*, uint32_t*), uint32_t lo_bits,
                              uint32_t hi_bits, unsigned long long* mismatches, uint32_t* first_bad) {
    if (!mismatches || !first_bad) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = use_device(0)) return rc;
    DevBuf<unsigned long long> dbad;
    DevBuf<uint32_t> dfirst;
    HIP_TRY(dbad.alloc(1));
    HIP_TRY(dfirst.alloc(1));
    HIP_TRY(hipMemset(dbad.get(), 0, 8));
    HIP_TRY(hipMemset(dfirst.get(), 0xff, 4));
    hipLaunchKernelGGL(kernel, dim3(8192), dim3(256), 0, 0, lo_bits, hi_bits, dbad.get(), dfirst.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(mismatches, dbad.get(), 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(first_bad, dfirst.get(), 4, hipMemcpyDeviceToHost));
    return CRT_OK;
}
int crt_selftest_rcp(uint32_t lo_bits, uint32_t hi_bits, unsigned long long* mismatches, uint32_t* first_bad) {
    return selftest_bit_range(crt_selftest_rcp_kernel, lo_bits, hi_bits, mismatches, first_bad);
}
int crt_selftest_sqrt(uint32_t lo_bits, uint32_t hi_bits, unsigned long long* mismatches, uint32_t* first_bad) {
    return selftest_bit_range(crt_selftest_sqrt_kernel, lo_bits, hi_bits, mismatches, first_bad);
}

int crt_selftest_unit(const float* in, int n, float* out) {
    if (!in || !out || n <= 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = use_device(0)) return rc;
    DevBuf<float> din, dout;
    HIP_TRY(din.alloc((size_t)n * 3));
    HIP_TRY(dout.alloc((size_t)n * 3));
    HIP_TRY(hipMemcpy(din.get(), in, (size_t)n * 12, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(crt_selftest_unit_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, din.get(), n, dout.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.get(), (size_t)n * 12, hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_selftest_scan(const int* in, int n_waves, int* out) {
    if (!in || !out || n_waves <= 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = use_device(0)) return rc;
    DevBuf<int> din, dout;
    HIP_TRY(din.alloc((size_t)n_waves * 64));
    HIP_TRY(dout.alloc((size_t)n_waves * 64 * 3));
    HIP_TRY(hipMemcpy(din.get(), in, (size_t)n_waves * 64 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(crt_selftest_scan_kernel, dim3(n_waves), dim3(64), 0, 0, din.get(), dout.get(), n_waves);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.get(), (size_t)n_waves * 64 * 12, hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_selftest_geometry(int kind, const float* in, int n, const crt_camera_desc* cam, int width, int height,
                          uint32_t* rng, float* out) {
    static const int in_words[5] = {17, 14, 12, 2, 12}, out_words[5] = {1, 1, 1, 6, 1};
    if (kind < 0 || kind > 4 || !in || !out || n <= 0 || (kind == 3 && (!cam || !rng || width <= 0 || height <= 0)))
        return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = use_device(0)) return rc;
    DevBuf<float> din, dout;
    DevBuf<uint32_t> drng;
    HIP_TRY(din.alloc((size_t)n * in_words[kind]));
    HIP_TRY(dout.alloc((size_t)n * out_words[kind]));
    if (kind == 3) HIP_TRY(drng.alloc((size_t)n * 6));
    HIP_TRY(hipMemcpy(din.get(), in, (size_t)n * in_words[kind] * 4, hipMemcpyHostToDevice));
    unsigned long long bad_w = 0, bad_h = 0;   // the renderer's choice for this size (crt_renderer_create)
    if (kind == 3) {
        HIP_TRY(hipMemcpy(drng.get(), rng, (size_t)n * 24, hipMemcpyHostToDevice));
        if (int rc = uv_div_mismatches(width, &bad_w)) return rc;
        if (int rc = uv_div_mismatches(height, &bad_h)) return rc;
    }
    hipLaunchKernelGGL(crt_selftest_geometry_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, kind, din.get(), n, dout.get(),
                       drng.get(), cam ? *cam : crt_camera_desc{}, width, height, kind == 3 ? 1.0f / (float)width : 1.f,
                       kind == 3 ? 1.0f / (float)height : 1.f, (int)(kind == 3 && bad_w == 0 && bad_h == 0));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.get(), (size_t)n * out_words[kind] * 4, hipMemcpyDeviceToHost));
    if (kind == 3) HIP_TRY(hipMemcpy(rng, drng.get(), (size_t)n * 24, hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_selftest_shade(const float* in, int n, float* out) {
    if (!in || !out || n <= 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = use_device(0)) return rc;
    DevBuf<float> din, dout;
    HIP_TRY(din.alloc((size_t)n * 32));
    HIP_TRY(dout.alloc((size_t)n * 20));
    HIP_TRY(hipMemcpy(din.get(), in, (size_t)n * 32 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(crt_selftest_shade_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, din.get(), n, dout.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.get(), (size_t)n * 20 * 4, hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt_selftest_rng(unsigned long long seed, const unsigned long long* subseq, int n, int n_draw,
                     uint32_t* state_out, float* uniforms_out) {
    if (!subseq || !state_out || !uniforms_out || n <= 0 || n_draw < 0)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = use_device(0)) return rc;
    const auto& tab = seq_tables();
    DevBuf<uint32_t> dseq, dst;
    DevBuf<float> du;
    HIP_TRY(dseq.alloc(tab.size()));
    HIP_TRY(dst.alloc((size_t)n * 6));
    HIP_TRY(du.alloc((size_t)n * std::max(n_draw, 1)));
    HIP_TRY(hipMemcpy(dseq.get(), tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    for (int i = 0; i < n; ++i) {   // one launch per subsequence keeps the kernel identical to the renderer's
        hipLaunchKernelGGL(crt_init_rand_kernel, dim3(1), dim3(64), 0, 0, dst.get() + 6 * i, dseq.get(), 1, seed, subseq[i]);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(crt_selftest_rng_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, dst.get(), n, n_draw, du.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(state_out, dst.get(), (size_t)n * 24, hipMemcpyDeviceToHost));
    if (n_draw) HIP_TRY(hipMemcpy(uniforms_out, du.get(), (size_t)n * n_draw * 4, hipMemcpyDeviceToHost));
    return CRT_OK;
}

// The schedule stages on caller-supplied costs: the renderer's own buffers and the host functions the renders call
// (order_tiles_by_probe, sort_descending, order_tile_slots, shard_tiles_in_row_order), on the null stream.
int crt_selftest_tile_schedule(crt_renderer* R, const uint32_t* pix_cost, int stride, int key_mode, int shard, int shards,
                               int xcd_regions, unsigned long long* stats_out) {
    if (!R || !pix_cost) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    if ((stride != 1 && stride != 2 && stride != 4) || key_mode < 0 || key_mode > 2 || shards < 1 || shard < 0 ||
        shard >= shards)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "bad stride, key mode or shard");
    HIP_TRY(hipSetDevice(R->device));
    const size_t n_pix = (size_t)R->width * R->height;
    const int n_tiles = R->n_tiles();
    if (int rc = ensure_order_buffers(R, 0, n_pix, n_tiles, true)) return rc;
    HIP_TRY(hipMemset(R->d_order.get(), 0xff, std::max(n_pix, (size_t)n_tiles * 64) * 4));
    HIP_TRY(hipMemcpy(R->d_tile_cost.get(), pix_cost, n_pix * 4, hipMemcpyHostToDevice));
    const int mode0 = R->tile_key_mode, xcd0 = R->xcd_regions;
    R->tile_key_mode = key_mode;
    R->xcd_regions = xcd_regions ? 1 : 0;
    const int rc = order_tiles_by_probe(R, 0, stride, stats_out != nullptr, shard, shards);
    R->tile_key_mode = mode0;
    R->xcd_regions = xcd0;
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    if (stats_out) { stats_out[0] = R->h_probe_stats.get()[0]; stats_out[1] = R->h_probe_stats.get()[1]; }
    return CRT_OK;
}

int crt_selftest_pixel_order(crt_renderer* R, int kind, const uint32_t* in, int shard, int shards) {
    if (!R || kind < 0 || kind > 3 || (kind <= 1 && !in)) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (kind == 3 && (shards < 1 || shard < 0 || shard >= shards))
        return set_error(CRT_ERR_INVALID_ARGUMENT, "bad shard");
    HIP_TRY(hipSetDevice(R->device));
    const size_t n_pix = (size_t)R->width * R->height;
    const int n_tiles = R->n_tiles();
    if (int rc = ensure_order_buffers(R, 0, n_pix, n_tiles, kind == 3)) return rc;
    HIP_TRY(hipMemset(R->d_order.get(), 0xff, std::max(n_pix, (size_t)n_tiles * 64) * 4));
    int rc = CRT_OK;
    if (kind == 0) {
        HIP_TRY(hipMemcpy(R->d_tile_cost.get(), in, n_pix * 4, hipMemcpyHostToDevice));
        rc = sort_descending(R, 0, R->d_tile_cost.get(), (int)n_pix, R->d_order.get());
    } else if (kind == 3) {
        shard_tiles_in_row_order(R, 0, n_tiles, shard, shards);
    } else {
        const int temporal0 = R->temporal;
        const bool valid0 = R->pix_rays_valid;
        R->temporal = kind == 1;
        if (kind == 1) {
            if (!R->d_pix_rays) rc = order_tile_slots(R, 0);   // allocates the temporal buffers (row order this once)
            if (!rc) {
                hipError_t e = hipMemcpy(R->d_pix_rays.get(), in, n_pix * 4, hipMemcpyHostToDevice);
                if (e == hipSuccess) e = hipMemset(R->d_order.get(), 0xff, (size_t)n_tiles * 64 * 4);
                if (e != hipSuccess) rc = set_error(CRT_ERR_HIP, hipGetErrorString(e));
            }
            R->pix_rays_valid = true;
        }
        if (!rc) rc = order_tile_slots(R, 0);
        R->temporal = temporal0;
        R->pix_rays_valid = kind == 1 ? false : valid0;   // kind 1 replaced the last frame's map
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return CRT_OK;
}

int crt_selftest_schedule_buffer(crt_renderer* R, int which, uint32_t* out, int64_t capacity, int64_t* n_out) {
    if (!R || !n_out || capacity < 0 || (capacity > 0 && !out))
        return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    const size_t n_pix = (size_t)R->width * R->height;
    const size_t n_tiles = (size_t)R->n_tiles();
    const uint32_t* src;
    size_t n;
    switch (which) {
        case 0: src = R->d_order.get(); n = std::max(n_pix, n_tiles * 64); break;
        case 1: src = R->d_tile_key.get(); n = n_tiles; break;
        case 2: src = R->d_tile_cost.get(); n = n_pix; break;
        case 3: src = R->d_pix_rays.get(); n = n_pix; break;
        case 4: src = R->d_tile_order.get(); n = n_tiles; break;
        default: return set_error(CRT_ERR_INVALID_ARGUMENT, "unknown schedule buffer");
    }
    if (!src) n = 0;
    *n_out = (int64_t)n;
    n = std::min(n, (size_t)capacity);
    if (n) {
        HIP_TRY(hipSetDevice(R->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, src, n * 4, hipMemcpyDeviceToHost));
    }
    return CRT_OK;
}

}  // extern "C"
