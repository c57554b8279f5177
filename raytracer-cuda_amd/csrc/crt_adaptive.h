// Adaptive sampling: refine only the 8x8 tiles of a frame that are still noisy.  Included by crt_hip.hip
// after the renderer; the refinement passes are the tile kernels (variants 8 and 10) over a shorter order list, so this
// file adds the error estimate, the list, the loop round them and a resolve that knows the tiles' sample counts.
//
// A pixel's samples come from its own RNG stream and its sum receives them in order, so a pixel that has received n
// samples holds the sum and the RNG state of a uniform n-spp frame whatever schedule gave it those samples.
#pragma once

// One wave per tile, four tiles per workgroup.  Tiles with tile_spp != n are left alone (their key is 0).  Per pixel the
// term of Dammertz et al.'s stopping condition from the two half buffers P = prev and Q = sum - prev, every operation f32,
// uncontracted, the divisions and the square root correctly rounded (the build's flags); the tile's error is the xor
// butterfly sum over the wave divided by the tile's in-frame pixels.  The order of the additions is fixed: the tests
// model it bit for bit.
__global__ __launch_bounds__(256) void crt_adaptive_plan_kernel(const float* __restrict__ sum, float* __restrict__ prev,
                                                                int32_t* __restrict__ tile_spp,
                                                                float* __restrict__ tile_error, uint32_t* __restrict__ key,
                                                                int width, int height, int tiles_x, int n_tiles, int n,
                                                                int next, float tolerance) {
    const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (t >= n_tiles) return;
    const int lane = threadIdx.x & 63;
    if (tile_spp[t] != n) {
        if (lane == 0) key[t] = 0u;
        return;
    }
    const int x0 = (t % tiles_x) * 8, y0 = (t / tiles_x) * 8;
    const int x = x0 + (lane & 7), y = y0 + (lane >> 3);
    const bool valid = x < width && y < height;
    const size_t p = valid ? 3 * ((size_t)y * width + x) : 0;
    float sx = 0.f, sy = 0.f, sz = 0.f, e = 0.f;
    if (valid) {
        sx = sum[p]; sy = sum[p + 1]; sz = sum[p + 2];
        const float px = prev[p], py = prev[p + 1], pz = prev[p + 2];
        const float qx = sx - px, qy = sy - py, qz = sz - pz;
        const float d = (fabsf(px - qx) + fabsf(py - qy)) + fabsf(pz - qz);
        const float I = ((sx + sy) + sz) / (float)n;
        if (I > 0.f) e = (d / (float)(n / 2)) / sqrtf(I);
    }
    float v = e;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) v += __shfl_xor(v, k, 64);
    const int in_frame = min(8, width - x0) * min(8, height - y0);
    const float E = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))) / (float)in_frame;
    const bool unconverged = !(E <= tolerance);      // a NaN is unconverged
    if (lane == 0) {
        tile_error[t] = E;
        // ordered integer of the error: NaN first, then the numbers by value (E >= 0: its bits order it); never 0
        const uint32_t bits = __float_as_uint(E);
        key[t] = !unconverged ? 0u : E != E ? 0xffffffffu : (bits & 0x80000000u) ? 1u : bits + 1u;
        if (unconverged) tile_spp[t] = next;
    }
    if (unconverged && valid) { prev[p] = sx; prev[p + 1] = sy; prev[p + 2] = sz; }
}

// The tiles with a key, in tile order, with their keys and their number: one workgroup, every thread a run of
// consecutive tiles, one scan over the threads' counts in LDS.  No atomics; the count is an ordinary store.
constexpr int ADAPT_COMPACT_THREADS = 1024;
__global__ __launch_bounds__(ADAPT_COMPACT_THREADS) void crt_adaptive_compact_kernel(const uint32_t* __restrict__ key,
                                                                                     int n_tiles,
                                                                                     uint32_t* __restrict__ tiles_out,
                                                                                     uint32_t* __restrict__ keys_out,
                                                                                     uint32_t* __restrict__ count) {
    __shared__ uint32_t part[ADAPT_COMPACT_THREADS];
    const int t = threadIdx.x;
    const int per = (n_tiles + ADAPT_COMPACT_THREADS - 1) / ADAPT_COMPACT_THREADS;
    const int lo = min(t * per, n_tiles), hi = min(lo + per, n_tiles);
    uint32_t c = 0;
    for (int i = lo; i < hi; ++i) c += key[i] != 0u;
    part[t] = c;
    __syncthreads();
    for (int o = 1; o < ADAPT_COMPACT_THREADS; o <<= 1) {
        const uint32_t add = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    uint32_t at = part[t] - c;      // the listed tiles before this thread's run: at + c <= the total <= n_tiles
    for (int i = lo; i < hi; ++i) {
        const uint32_t k = key[i];
        if (k != 0u) { tiles_out[at] = (uint32_t)i; keys_out[at] = k; ++at; }
    }
    if (t == ADAPT_COMPACT_THREADS - 1) *count = part[t];
}

// list = the compacted tiles, largest key first (ties in tile order).  Every listed tile counts the listed tiles ahead
// of it: count^2 integer compares over keys staged through LDS in blocks of 1024 (every lane reads the same words, a
// broadcast), no atomics, an exact and deterministic order.  The grid covers n_tiles; workgroups beyond the count, which
// the kernel reads from device memory, leave at once.  A tile's rank counts other listed tiles only, so it is below the count.
constexpr int ADAPT_RANK_BLOCK = 1024;
__global__ __launch_bounds__(256) void crt_adaptive_rank_kernel(const uint32_t* __restrict__ tiles_in,
                                                                const uint32_t* __restrict__ keys_in,
                                                                const uint32_t* __restrict__ count, int n_tiles,
                                                                uint32_t* __restrict__ list) {
    __shared__ __attribute__((aligned(16))) uint32_t k_lds[ADAPT_RANK_BLOCK];
    const int m = (int)min(*count, (uint32_t)n_tiles);
    if ((int)(blockIdx.x * 256) >= m) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t mine = i < m ? keys_in[i] : 0u;
    uint32_t rank = 0;
    for (int base = 0; base < m; base += ADAPT_RANK_BLOCK) {
        __syncthreads();
        for (int j = threadIdx.x; j < ADAPT_RANK_BLOCK; j += 256) k_lds[j] = base + j < m ? keys_in[base + j] : 0u;
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < ADAPT_RANK_BLOCK; j += 4) {
            const uint4 k = *reinterpret_cast<const uint4*>(k_lds + j);
            const int u = base + j;
            rank += (k.x > mine || (k.x == mine && u < i)) + (k.y > mine || (k.y == mine && u + 1 < i)) +
                    (k.z > mine || (k.z == mine && u + 2 < i)) + (k.w > mine || (k.w == mine && u + 3 < i));
        }
    }
    if (i < m) list[rank] = tiles_in[i];      // the padding's key 0 never counts for a listed tile (its key is >= 1)
}

// crt_resolve_kernel with the pixel's own scale, 1 / the samples its tile holds.
__global__ __launch_bounds__(256) void crt_resolve_adaptive_kernel(const float* __restrict__ sum, uint8_t* __restrict__ rgba,
                                                                   const int32_t* __restrict__ tile_spp, int width,
                                                                   int n_pix, int tiles_x) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n_pix) return;
    const int x = pix % width, y = pix / width;
    const float scale = 1.f / (float)tile_spp[(y >> 3) * tiles_x + (x >> 3)];
    uchar4 o;
    o.x = to_u8(scale * sum[3 * (size_t)pix]);
    o.y = to_u8(scale * sum[3 * (size_t)pix + 1]);
    o.z = to_u8(scale * sum[3 * (size_t)pix + 2]);
    o.w = 255;
    reinterpret_cast<uchar4*>(rgba)[pix] = o;
}

namespace {

// The state is allocated on first use and initialised on `st`, the stream its first user goes on to enqueue on.
int adaptive_state(crt_renderer* R, hipStream_t st, AdaptiveState** out) {
    return first_use(R->adaptive, "the adaptive state of this renderer could not be allocated", out, [&](AdaptiveState* A) -> int {
        const size_t n_pix = (size_t)R->width * R->height, n_tiles = (size_t)R->n_tiles();
        HIP_TRY(A->prev.alloc(n_pix * 3));
        HIP_TRY(A->tile_spp.alloc(n_tiles));
        HIP_TRY(A->tile_error.alloc(n_tiles));
        HIP_TRY(A->key.alloc(n_tiles));
        HIP_TRY(A->ctile.alloc(n_tiles));
        HIP_TRY(A->ckey.alloc(n_tiles));
        HIP_TRY(A->list.alloc(n_tiles));
        HIP_TRY(A->d_count.alloc(1));
        HIP_TRY(A->h_count.alloc(1));
        HIP_TRY(hipMemsetAsync(A->prev.get(), 0, n_pix * 3 * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(A->tile_spp.get(), 0, n_tiles * 4, st));
        HIP_TRY(hipMemsetAsync(A->tile_error.get(), 0, n_tiles * 4, st));
        HIP_TRY(hipMemsetAsync(A->list.get(), 0xff, n_tiles * 4, st));
        HIP_TRY(hipMemsetAsync(A->d_count.get(), 0, 4, st));
        HIP_TRY(A->ev0.create());
        HIP_TRY(A->ev1.create());
        return CRT_OK;
    });
}

// One plan step on `st`: errors, keys, tile_spp and prev of the tiles at n samples, then the listed tiles and their
// count.  Returns the list through *list: by error, or (by_error false) the compacted tiles in tile order.
int adaptive_plan(crt_renderer* R, AdaptiveState* A, hipStream_t st, int n, int next, float tolerance, bool by_error,
                  const uint32_t** list) {
    const int tiles_x = R->tiles_x(), n_tiles = R->n_tiles();
    hipLaunchKernelGGL(crt_adaptive_plan_kernel, dim3((n_tiles + 3) / 4), dim3(256), 0, st, R->d_sum, A->prev.get(), A->tile_spp.get(),
                       A->tile_error.get(), A->key.get(), R->width, R->height, tiles_x, n_tiles, n, next, tolerance);
    hipLaunchKernelGGL(crt_adaptive_compact_kernel, dim3(1), dim3(ADAPT_COMPACT_THREADS), 0, st, A->key.get(), n_tiles, A->ctile.get(),
                       A->ckey.get(), A->d_count.get());
    if (by_error)
        hipLaunchKernelGGL(crt_adaptive_rank_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, st, A->ctile.get(), A->ckey.get(),
                           A->d_count.get(), n_tiles, A->list.get());
    HIP_TRY(hipGetLastError());
    *list = by_error ? A->list.get() : A->ctile.get();
    return CRT_OK;
}

// A refinement pass: the tile kernel of the scene's width (variant 8 or 10) over `count` tiles of `list`, spp more
// samples added to their sums.  No probe: the list is the order (the loop passes the tiles in tile order, which was
// measured faster than by error: neighbouring tiles run together).  Occupancy as crt_renderer_render chooses it without the
// probe, from the tiles of this pass.  The critical-tile threshold is the probe order's and stays off.
int adaptive_pass(crt_renderer* R, const crt_scene* S, hipStream_t st, const uint32_t* list, int count, int spp,
                  int max_bounces, bool critical) {
    const int variant = S->width == 4 ? 8 : 10;
    RenderParams P = render_params(R, S, spp, max_bounces, CRT_RENDER_ACCUMULATE);
    const int occ = R->min_waves ? R->min_waves
                  : variant == 8 ? ((size_t)count >= (size_t)4 * R->n_cus * 4 * 7 ? 7 : 6) : 6;
    P.stack_lds = stack_lds_for(R, S, occ);
    if (int rc = ensure_overflow_stack(R, S, st, P)) return rc;
    P.tiles_x = R->tiles_x();
    P.order = list;
    if (critical && variant == 8) {   // measurement only: the list's first tiles at the critical threshold
        P.crit_tiles = R->crit_tiles < 0 ? 4 * R->n_cus : R->crit_tiles;
        P.crit_threshold = R->crit_threshold;
    }
    take_timing_slot(R);
    HIP_TRY(hipEventRecord(R->ev0, st));
    R->last_schedule[0] = R->last_schedule[2] = R->last_schedule[3] = 0.f;
    R->last_schedule[1] = variant == 8 ? (float)occ : 0.f;
    if (int rc = launch_render(R, RENDER_ROWS[render_row(variant, false, occ)], false, dim3((unsigned)count), dim3(64),
                               st, P, S))
        return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(R->ev1, st));
    ++R->n_timed;
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_renderer_render_adaptive(crt_renderer* R, const crt_scene* S, const crt_adaptive_options* o, int max_bounces,
                                 unsigned flags, crt_adaptive_stats* stats_out, void* stream) {
    if (!R || !S || !o) return set_error(CRT_ERR_INVALID_ARGUMENT, "render adaptive: null argument");
    if (o->spp_min < 2 || (o->spp_min & 1))
        return set_error(CRT_ERR_INVALID_ARGUMENT, "render adaptive: spp_min must be even and >= 2");
    if (o->spp_max < o->spp_min) return set_error(CRT_ERR_INVALID_ARGUMENT, "render adaptive: spp_max below spp_min");
    if (o->tolerance != o->tolerance) return set_error(CRT_ERR_INVALID_ARGUMENT, "render adaptive: tolerance is NaN");
    if (o->reserved & ~3) return set_error(CRT_ERR_INVALID_ARGUMENT, "render adaptive: reserved bits set");
    if (max_bounces < 1) return set_error(CRT_ERR_INVALID_ARGUMENT, "render adaptive: max_bounces must be >= 1");
    if (flags) return set_error(CRT_ERR_UNSUPPORTED, "render adaptive: takes no render flag (it owns the sums; work counters are crt_renderer_render's)");
    if (S->device != R->device)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "render adaptive: scene and renderer on different devices");
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, "render adaptive: camera not set");
    if (R->tile_shards > 1) return set_error(CRT_ERR_UNSUPPORTED, "render adaptive: pixel sharding is crt_renderer_render's");
    HIP_TRY(hipSetDevice(R->device));
    hipStream_t st = (hipStream_t)stream;
    AdaptiveState* A = nullptr;
    if (int rc = adaptive_state(R, st, &A)) return rc;
    const size_t n_pix = (size_t)R->width * R->height;
    const int tiles_x = R->tiles_x(), n_tiles = R->n_tiles();
    if (!R->n_cus) HIP_TRY(hipDeviceGetAttribute(&R->n_cus, hipDeviceAttributeMultiprocessorCount, R->device));
    crt_adaptive_stats stats{};
    HIP_TRY(hipEventRecord(A->ev0.get(), st));
    // the first spp_min samples in two halves, so that prev holds the first half's sums
    if (int rc = crt_renderer_render(R, S, o->spp_min / 2, max_bounces, 0u, stream)) return rc;
    HIP_TRY(hipMemcpyAsync(A->prev.get(), R->d_sum, n_pix * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (int rc = crt_renderer_render(R, S, o->spp_min / 2, max_bounces, CRT_RENDER_ACCUMULATE, stream)) return rc;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)A->tile_spp.get(), o->spp_min, (size_t)n_tiles, st));
    HIP_TRY(hipMemsetAsync(A->tile_error.get(), 0, (size_t)n_tiles * 4, st));
    for (int64_t n = o->spp_min; n < o->spp_max; n *= 2) {
        const int next = (int)std::min<int64_t>(2 * n, o->spp_max);
        const uint32_t* list = nullptr;
        if (int rc = adaptive_plan(R, A, st, (int)n, next, o->tolerance, (o->reserved & 1) != 0, &list)) return rc;
        HIP_TRY(hipMemcpyAsync(A->h_count.get(), A->d_count.get(), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));      // the pass's one host wait
        const int m = (int)std::min<uint32_t>(A->h_count.get()[0], (uint32_t)n_tiles);
        if (m == 0) break;
        if (int rc = adaptive_pass(R, S, st, list, m, next - (int)n, max_bounces, (o->reserved & 2) != 0)) return rc;
        ++stats.passes;
    }
    HIP_TRY(hipEventRecord(A->ev1.get(), st));
    std::vector<int32_t> spp((size_t)n_tiles);
    HIP_TRY(hipMemcpyAsync(spp.data(), A->tile_spp.get(), (size_t)n_tiles * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventSynchronize(A->ev1.get()));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&stats.ms, A->ev0.get(), A->ev1.get()));
    for (int t = 0; t < n_tiles; ++t) {
        const int w = std::min(8, R->width - (t % tiles_x) * 8), h = std::min(8, R->height - (t / tiles_x) * 8);
        stats.samples += (uint64_t)(w * h) * (uint64_t)spp[(size_t)t];
        stats.tiles_refined += spp[(size_t)t] > o->spp_min;
        stats.tiles_at_max += spp[(size_t)t] == o->spp_max;
    }
    if (stats_out) *stats_out = stats;
    return crt_renderer_synchronize(R, stream);
}

int crt_renderer_resolve_adaptive(crt_renderer* R, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    if (!R->adaptive || !R->adaptive->tile_spp)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "resolve adaptive: no adaptive render on this renderer yet");
    HIP_TRY(hipSetDevice(R->device));
    const int n = R->width * R->height;
    hipLaunchKernelGGL(crt_resolve_adaptive_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, R->d_sum,
                       R->d_rgba.get(), R->adaptive->tile_spp.get(), R->width, n, R->tiles_x());
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

int crt_renderer_read_tile_spp(crt_renderer* R, int32_t* out) {
    if (!R || !R->adaptive || !R->adaptive->tile_spp)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "read tile spp: no adaptive render on this renderer yet");
    return read_dev(R, out, R->adaptive->tile_spp.get(), (size_t)R->n_tiles() * 4);
}
int crt_renderer_read_tile_error(crt_renderer* R, float* out) {
    if (!R || !R->adaptive || !R->adaptive->tile_error)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "read tile error: no adaptive render on this renderer yet");
    return read_dev(R, out, R->adaptive->tile_error.get(), (size_t)R->n_tiles() * 4);
}
int crt_renderer_read_adaptive_prev(crt_renderer* R, float* out) {
    if (!R || !R->adaptive || !R->adaptive->prev)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "read adaptive prev: no adaptive render on this renderer yet");
    return read_dev(R, out, R->adaptive->prev.get(), (size_t)R->width * R->height * 12);
}

// The plan on caller-supplied buffers: the renderer's own state and the host function the loop calls, on the null stream.
int crt_selftest_adaptive_plan(crt_renderer* R, const float* sum, const float* prev, const int32_t* tile_spp, int n,
                               int next, float tolerance, uint32_t* list_out, uint32_t* n_listed_out) {
    if (!R || !sum || !prev || !tile_spp || !list_out || !n_listed_out)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "selftest adaptive plan: null argument");
    if (n < 2 || (n & 1) || next < n) return set_error(CRT_ERR_INVALID_ARGUMENT, "selftest adaptive plan: n must be even and >= 2, next >= n");
    if (tolerance != tolerance) return set_error(CRT_ERR_INVALID_ARGUMENT, "selftest adaptive plan: tolerance is NaN");
    HIP_TRY(hipSetDevice(R->device));
    AdaptiveState* A = nullptr;
    if (int rc = adaptive_state(R, 0, &A)) return rc;
    const size_t n_pix = (size_t)R->width * R->height, n_tiles = (size_t)R->n_tiles();
    HIP_TRY(hipMemcpy(R->d_sum, sum, n_pix * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(A->prev.get(), prev, n_pix * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(A->tile_spp.get(), tile_spp, n_tiles * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(A->list.get(), 0xff, n_tiles * 4));
    const uint32_t* list = nullptr;
    if (int rc = adaptive_plan(R, A, 0, n, next, tolerance, true, &list)) return rc;
    HIP_TRY(hipStreamSynchronize(0));
    HIP_TRY(hipMemcpy(n_listed_out, A->d_count.get(), 4, hipMemcpyDeviceToHost));
    const size_t m = std::min<size_t>(*n_listed_out, n_tiles);
    if (m) HIP_TRY(hipMemcpy(list_out, list, m * 4, hipMemcpyDeviceToHost));
    return CRT_OK;
}

}  // extern "C"
