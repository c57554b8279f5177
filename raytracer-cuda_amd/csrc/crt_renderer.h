// crt_renderer.h — the renderer handle's own entries: creation (the XORWOW jump tables, the uv_div check of the frame's
// size), attach, destroy, init_rand, every setter, synchronise and the device error word, the reads, the
// counters, the profile and timing getters, compare, resolve and render_frame.  The render itself is crt_dispatch.h.
// Host code only.  Included by crt_hip.hip after crt_scene.h; needs crt_handles.h and the compare, init-rand, resolve
// and uv_div check kernels.
#pragma once

namespace {

// XORWOW single-step linear map and its 2^67*4^k powers (160 columns x 5 words).
void xw_step(uint32_t v[5]) {
    uint32_t t = v[0] ^ (v[0] >> 2);
    v[0] = v[1]; v[1] = v[2]; v[2] = v[3]; v[3] = v[4];
    v[4] = (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1));
}
void mv(const uint32_t* m, uint32_t v[5]) {
    uint32_t r[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 160; ++i)
        if (v[i / 32] & (1u << (i % 32)))
            for (int k = 0; k < 5; ++k) r[k] ^= m[i * 5 + k];
    std::memcpy(v, r, sizeof r);
}
void mm(const uint32_t* b, const uint32_t* a, uint32_t* c) {   // c = b o a
    for (int col = 0; col < 160; ++col) {
        uint32_t v[5];
        std::memcpy(v, a + 5 * col, sizeof v);
        mv(b, v);
        std::memcpy(c + 5 * col, v, sizeof v);
    }
}
const std::vector<uint32_t>& seq_tables() {
    static std::vector<uint32_t> tab;
    static std::once_flag once;
    std::call_once(once, [] {
        tab.assign(32 * 800, 0);
        std::vector<uint32_t> m(800), t(800);
        for (int col = 0; col < 160; ++col) {
            uint32_t v[5] = {0, 0, 0, 0, 0};
            v[col / 32] = 1u << (col % 32);
            xw_step(v);
            std::memcpy(&m[5 * col], v, sizeof v);
        }
        for (int s = 0; s < 67; ++s) { mm(m.data(), m.data(), t.data()); m.swap(t); }
        std::memcpy(&tab[0], m.data(), 800 * 4);
        for (int k = 1; k < 32; ++k) {
            mm(&tab[800 * (k - 1)], &tab[800 * (k - 1)], t.data());
            mm(t.data(), t.data(), &tab[800 * k]);
        }
    });
    return tab;
}

}  // namespace

namespace {
// Mismatches of uv_div(a, b, RN(1 / b)) against a / b over every a next_ray can form for an image dimension b:
// a = fl(x + U) with x in [0, b - 1] and U = fl(X * 2^-32 + 2^-33) in [2^-33, 1], so a in [2^-33, b].
constexpr uint32_t UV_A_MIN_BITS = 0x2f000000u;   // 2^-33
int uv_div_mismatches(int dim, unsigned long long* out) {
    const float b = (float)dim, r = 1.0f / b;
    uint32_t hi;
    std::memcpy(&hi, &b, 4);
    DevBuf<unsigned long long> d;
    HIP_TRY(d.alloc(1));
    HIP_TRY(hipMemset(d.get(), 0, 8));
    hipLaunchKernelGGL(crt_uv_div_check_kernel, dim3(4096), dim3(256), 0, 0, b, r, UV_A_MIN_BITS, hi, d.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d.get(), 8, hipMemcpyDeviceToHost));
    return CRT_OK;
}
}  // namespace

extern "C" {

static hipError_t create_timing_ring(crt_renderer* R) {
    for (auto& slot : R->ring)
        for (DevEvent& ev : slot)
            if (hipError_t e = ev.create(); e != hipSuccess) return e;
    return hipSuccess;
}

int crt_renderer_create(int width, int height, int device, crt_renderer** out) {
    if (!out || width <= 0 || height <= 0 || (long long)width * height > (1LL << 31) / 6)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "bad renderer size");
    *out = nullptr;
    if (int rc = use_device(device)) return rc;
    crt_renderer* R = new (std::nothrow) crt_renderer;
    if (!R) return set_error(CRT_ERR_OUT_OF_MEMORY, "host allocation failed");
    R->device = device; R->width = width; R->height = height;
    const size_t n = (size_t)width * height;
    const auto& tab = seq_tables();
    hipError_t e;
    if ((e = R->d_rng.alloc(n * 6)) != hipSuccess ||
        (e = R->d_sum_own.alloc(n * 3)) != hipSuccess ||
        (e = R->d_rgba.alloc(n * 4)) != hipSuccess ||
        (e = R->d_seq.alloc(tab.size())) != hipSuccess ||
        (e = R->d_counters.alloc(16)) != hipSuccess ||
        (e = hipMemcpy(R->d_seq.get(), tab.data(), tab.size() * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemset(R->d_sum_own.get(), 0, n * 3 * 4)) != hipSuccess ||
        (e = hipMemset(R->d_rgba.get(), 0, n * 4)) != hipSuccess ||
        (e = hipMemset(R->d_counters.get(), 0, 16 * sizeof(unsigned long long))) != hipSuccess ||
        (e = create_timing_ring(R)) != hipSuccess) {
        crt_renderer_destroy(R);
        return set_error(e == hipErrorOutOfMemory ? CRT_ERR_OUT_OF_MEMORY : CRT_ERR_HIP,
                         std::string("renderer allocation: ") + hipGetErrorString(e));
    }
    R->d_sum = R->d_sum_own.get();
    // next_ray's image-coordinate divisions: uv_div when it equals the IEEE division for every input of this size
    unsigned long long bad_w = 0, bad_h = 0;
    int rc = uv_div_mismatches(width, &bad_w);
    if (rc == CRT_OK) rc = height == width ? CRT_OK : uv_div_mismatches(height, &bad_h);
    if (rc != CRT_OK) {
        crt_renderer_destroy(R);
        return rc;
    }
    R->rcp_w = 1.0f / (float)width;
    R->rcp_h = 1.0f / (float)height;
    R->fast_uv = bad_w == 0 && bad_h == 0;
    // the table's copy, the three clears and the division checks ran on the null stream: wait for them here, once per
    // handle, so that the first call may come on any stream (a non-blocking one too)
    if ((e = hipStreamSynchronize(0)) != hipSuccess) {
        crt_renderer_destroy(R);
        return set_error(CRT_ERR_HIP, std::string("renderer initialisation: ") + hipGetErrorString(e));
    }
    *out = R;
    return CRT_OK;
}

int crt_renderer_attach_linear(crt_renderer* R, float* ptr) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    if (ptr) {
        hipPointerAttribute_t attr;
        HIP_TRY(hipPointerGetAttributes(&attr, ptr));
        if (attr.type != hipMemoryTypeDevice || attr.device != R->device)
            return set_error(CRT_ERR_INVALID_ARGUMENT, "attach_linear: not device memory of the renderer's device");
    }
    R->d_sum = ptr ? ptr : R->d_sum_own.get();
    return CRT_OK;
}

void crt_renderer_destroy(crt_renderer* R) {
    if (!R) return;
    (void)hipSetDevice(R->device);
    delete R;
}

int crt_renderer_init_rand(crt_renderer* R, unsigned long long seed, unsigned long long subseq_base, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    HIP_TRY(hipSetDevice(R->device));
    const int n = R->width * R->height;
    hipStream_t st = (hipStream_t)stream;
    // curand_init is a pure function of (seed, subsequence): keep the initialised array and copy it back for a
    // repeated (seed, base) — 2.8 ms of GF(2) jumps at 2560x1440 become a 35 us device copy, same bits
    if (R->rng_cache_valid && R->rng_cache_seed == seed && R->rng_cache_base == subseq_base) {
        HIP_TRY(hipMemcpyAsync(R->d_rng.get(), R->d_rng_cache.get(), (size_t)n * 24, hipMemcpyDeviceToDevice, st));
        return CRT_OK;
    }
    hipLaunchKernelGGL(crt_init_rand_kernel, dim3((n + 255) / 256), dim3(256), 0, st, R->d_rng.get(),
                       R->d_seq.get(), n, seed, subseq_base);
    HIP_TRY(hipGetLastError());
    R->rng_cache_valid = false;
    if (!R->d_rng_cache) {
        HIP_TRY(hipStreamSynchronize(st));
        if (R->d_rng_cache.alloc((size_t)n * 6) != hipSuccess) {   // optional: no cache then
            (void)hipGetLastError();
            return CRT_OK;
        }
    }
    HIP_TRY(hipMemcpyAsync(R->d_rng_cache.get(), R->d_rng.get(), (size_t)n * 24, hipMemcpyDeviceToDevice, st));
    R->rng_cache_seed = seed;
    R->rng_cache_base = subseq_base;
    R->rng_cache_valid = true;
    return CRT_OK;
}

int crt_renderer_set_kernel_variant(crt_renderer* R, int variant) {
    if (!R || variant < -1 || variant > 10 || variant == 5 || variant == 6 || variant == 9)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "bad kernel variant (-1 = automatic, 0-4, 7, 8, 10)");
    R->variant = variant;
    return CRT_OK;
}

int crt_renderer_set_schedule(crt_renderer* R, int probe_spp, int min_spp, int flags) {
    if (!R || probe_spp < -1 || probe_spp > 64 || min_spp < 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad schedule");
    const int stride = (flags >> 20) & 0xf;   // variant 8's probe subsampling: 0 = automatic, 1 (every pixel), 2, 4
    if (stride != 0 && stride != 1 && stride != 2 && stride != 4)   // checked before any field changes
        return set_error(CRT_ERR_INVALID_ARGUMENT, "probe stride (flags >> 20): 0, 1, 2 or 4");
    R->probe_spp = probe_spp < 0 ? -1 : probe_spp;
    R->probe_min_spp = min_spp;
    R->tile_key_mode = (flags >> 16) & 0xf;   // 0 = slowest pixel (callers that pass 0 get the plain key)
    R->probe_stride = stride;
    return CRT_OK;
}

int crt_renderer_set_pixel_shard(crt_renderer* R, int shard, int shards) {
    if (!R || shards < 1 || shard < 0 || shard >= shards) return set_error(CRT_ERR_INVALID_ARGUMENT, "shard in [0, shards)");
    if (shards > R->n_tiles()) return set_error(CRT_ERR_INVALID_ARGUMENT, "more shards than 8x8 tiles");
    R->tile_shard = shard;
    R->tile_shards = shards;
    return CRT_OK;
}

int crt_renderer_set_top_levels(crt_renderer* R, int levels) {
    if (!R || levels < -1 || levels > CRT_TOP_LEVELS)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "top levels -1 (default) .. " + std::to_string(CRT_TOP_LEVELS));
    R->top_levels = levels;
    return CRT_OK;
}

int crt_renderer_set_critical_tiles(crt_renderer* R, int tiles, int lanes) {
    if (!R || tiles < -1 || lanes < 1 || lanes > 64) return set_error(CRT_ERR_INVALID_ARGUMENT, "critical tiles >= -1, lanes 1..64");
    R->crit_tiles = tiles;
    R->crit_threshold = lanes;
    return CRT_OK;
}

int crt_renderer_set_occupancy_target(crt_renderer* R, int waves_per_simd) {
    if (!R || waves_per_simd < 0 || waves_per_simd > 8) return set_error(CRT_ERR_INVALID_ARGUMENT, "waves per SIMD 0..8");
    R->min_waves = waves_per_simd;
    return CRT_OK;
}

int crt_renderer_set_stack_lds(crt_renderer* R, int entries) {
    if (!R || entries < 1 || entries > STACK_LDS) return set_error(CRT_ERR_INVALID_ARGUMENT, "stack LDS entries 1..16");
    R->stack_lds = entries;
    return CRT_OK;
}

int crt_renderer_set_regen_threshold(crt_renderer* R, int lanes) {
    if (!R || lanes < 1 || lanes > 64) return set_error(CRT_ERR_INVALID_ARGUMENT, "threshold must be 1..64");
    R->regen_threshold = lanes;
    R->regen_threshold_wide = lanes;
    return CRT_OK;
}

int crt_renderer_set_camera(crt_renderer* R, const crt_camera_desc* cam) {
    if (!R || !cam) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    // primary rays start within lens_radius of the origin (right/up are unit vectors); the 4-wide slab test needs
    // |o| * 2^64 finite (box_inv), the same 2^60 bound the rebuilt tree's boxes are held to
    bool ok = std::isfinite(cam->lens_radius) && std::fabs(cam->lens_radius) < 0x1p58f;
    for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(cam->origin[a]) && std::fabs(cam->origin[a]) < 0x1p59f;
    if (!ok) return set_error(CRT_ERR_INVALID_ARGUMENT, "camera origin or lens radius non-finite or beyond 2^59");
    R->cam = *cam;
    R->has_camera = true;
    return CRT_OK;
}

int crt_scene_compare_dump(crt_renderer* R, const crt_scene* A, const crt_scene* B, int spp, int max_bounces,
                           uint64_t out[5], float* dump, int max_dump);
int crt_scene_compare(crt_renderer* R, const crt_scene* A, const crt_scene* B, int spp, int max_bounces,
                      uint64_t out[5]) {
    return crt_scene_compare_dump(R, A, B, spp, max_bounces, out, nullptr, 0);
}

int crt_scene_compare_dump(crt_renderer* R, const crt_scene* A, const crt_scene* B, int spp, int max_bounces,
                           uint64_t out[5], float* dump, int max_dump) {
    if (!R || !A || !B || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, "camera not set");
    if (A->device != R->device || B->device != R->device)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "scenes and renderer on different devices");
    if (A->n_ranks != B->n_ranks) return set_error(CRT_ERR_INVALID_ARGUMENT, "scenes hold different primitive sets");
    if (spp < 0 || max_bounces < 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "negative spp / bounces");
    HIP_TRY(hipSetDevice(R->device));
    HIP_TRY(hipMemset(R->d_counters.get(), 0, ERR_WORD * sizeof(unsigned long long)));
    CompareParams Q{};
    RenderParams& P = Q.A;
    P.nodes = A->d_nodes.get(); P.prims = A->d_prims.get(); P.mats = A->d_mats.get(); P.shade = A->d_shade.get();
    P.n_nodes = A->n_nodes; P.n_mats = A->n_mats; P.n_prims = A->n_prims; P.n_layouts = A->layouts;
    P.err = reinterpret_cast<unsigned*>(R->d_counters.get() + ERR_WORD);
    P.width = R->width; P.height = R->height; P.spp = spp; P.max_bounces = max_bounces;
    P.accumulate = 0; P.regen_threshold = 64; P.drain_threshold = 64; P.wave_drain = 64;
    P.rng = R->d_rng.get(); P.sum = R->d_sum; P.counters = R->d_counters.get(); P.cam = R->cam;
    P.rcp_w = R->rcp_w; P.rcp_h = R->rcp_h; P.fast_uv = R->fast_uv;
    P.probe_stride = 1;
    P.pix_rays = nullptr;
    Q.nodes_b = B->d_nodes.get(); Q.prims_b = B->d_prims.get(); Q.n_nodes_b = B->n_nodes; Q.n_layouts_b = B->layouts;
    Q.width_a = A->width; Q.width_b = B->width;
    Q.dump = nullptr;
    Q.max_dump = 0;
    DevBuf<float> d_dump;
    if (dump && max_dump > 0) {
        HIP_TRY(d_dump.alloc((size_t)max_dump * 10));
        Q.dump = d_dump.get();
        Q.max_dump = max_dump;
    }
    P.sphere_first = A->sphere_first; P.n_ray_spheres = A->n_ray_spheres; P.sphere_chain = A->d_chain.get();
    P.n_chain = A->n_chain;
    std::memcpy(P.sph2, A->sph2, sizeof P.sph2);
    Q.sphere_first_b = B->sphere_first; Q.n_spheres_b = B->n_ray_spheres; Q.chain_b = B->d_chain.get();
    Q.n_chain_b = B->n_chain;
    dim3 grid((R->width + 15) / 16, (R->height + 15) / 16), block(256);
    hipLaunchKernelGGL(crt_compare_kernel, grid, block, 0, 0, Q);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long h[8];
    HIP_TRY(hipMemcpy(h, R->d_counters.get(), sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 5; ++i) out[i] = h[i];
    if (d_dump) {
        const size_t n = std::min<size_t>((size_t)max_dump, (size_t)(h[6] & 0xffffffffu));
        if (n) HIP_TRY(hipMemcpy(dump, d_dump.get(), n * 10 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return CRT_OK;
}

int crt_renderer_resolve(crt_renderer* R, float scale, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    HIP_TRY(hipSetDevice(R->device));
    const int n = R->width * R->height;
    hipLaunchKernelGGL(crt_resolve_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, R->d_sum,
                       R->d_rgba.get(), n, scale);
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

int crt_renderer_render_frame(crt_renderer* R, const crt_scene* S, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, "camera not set");
    if (int rc = crt_renderer_render(R, S, R->cam.samples_per_pixel, 20, 0u, stream)) return rc;
    if (int rc = crt_renderer_resolve(R, R->cam.pixel_sample_scale, stream)) return rc;
    return crt_renderer_synchronize(R, stream);
}

// The device error word (sticky across renders until read here): a render that dropped a traversal-stack entry
// or met an out-of-range primitive index produced a wrong frame.  Reported where the reference reports a kernel
// fault, at the synchronisation after the launch (CUDARenderer.cuh:59, CUDA_CHECK(cudaDeviceSynchronize())).
static int take_device_error(crt_renderer* R, unsigned long long word) {
    if (!word) return CRT_OK;
    // the callers waited for the stream before they read the word; the clear is a null-stream operation and is waited
    // for, so that a render the caller enqueues next on any stream cannot have its report cleared
    HIP_TRY(hipMemset(R->d_counters.get() + ERR_WORD, 0, sizeof(unsigned long long)));
    HIP_TRY(hipStreamSynchronize(0));
    std::string m = "render kernel reported an internal error:";
    if (word & 1u) m += " primitive index out of range;";
    if (word & 2u) m += " traversal stack deeper than the scene's stack bound (entries dropped);";
    if (word & 4u) m += " leaf-round pair outside its owner's span (checked build);";
    return set_error(CRT_ERR_HIP, m + " the frame is invalid");
}

int crt_renderer_synchronize(crt_renderer* R, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    HIP_TRY(hipSetDevice(R->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    unsigned long long word = 0;
    HIP_TRY(hipMemcpy(&word, R->d_counters.get() + ERR_WORD, sizeof word, hipMemcpyDeviceToHost));
    return take_device_error(R, word);
}

static int read_dev(crt_renderer* R, void* dst, const void* src, size_t bytes) {
    if (!R || !dst) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(R->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return CRT_OK;
}
int crt_renderer_read_linear(crt_renderer* R, float* out) {
    return R ? read_dev(R, out, R->d_sum, (size_t)R->width * R->height * 12) : set_error(CRT_ERR_INVALID_ARGUMENT, "null");
}
int crt_renderer_read_rgba8(crt_renderer* R, uint8_t* out) {
    return R ? read_dev(R, out, R->d_rgba.get(), (size_t)R->width * R->height * 4) : set_error(CRT_ERR_INVALID_ARGUMENT, "null");
}
int crt_renderer_read_rng(crt_renderer* R, uint32_t* out) {
    return R ? read_dev(R, out, R->d_rng.get(), (size_t)R->width * R->height * 24) : set_error(CRT_ERR_INVALID_ARGUMENT, "null");
}
int crt_renderer_write_linear(crt_renderer* R, const float* in) {
    if (!R || !in) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(R->device));
    HIP_TRY(hipMemcpy(R->d_sum, in, (size_t)R->width * R->height * 12, hipMemcpyHostToDevice));
    return CRT_OK;
}
int crt_renderer_get_counters(crt_renderer* R, crt_work_counters* out) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    unsigned long long c[16];
    if (int rc = read_dev(R, c, R->d_counters.get(), sizeof c)) return rc;
    R->diag[0] = c[5]; R->diag[1] = c[6] & ((1ull << 40) - 1); R->diag[2] = c[6] >> 40;
    for (int i = 0; i < 7; ++i) R->prof[i] = c[8 + i];
    R->prof[7] = c[7];
    out->rays = c[0]; out->box_tests = c[1]; out->tri_tests = c[2]; out->sphere_tests = c[3]; out->paths = c[4];
    return take_device_error(R, c[ERR_WORD]);
}
int crt_renderer_get_section_profile(crt_renderer* R, unsigned long long* out7) {
    if (!R || !out7) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    for (int i = 0; i < 7; ++i) out7[i] = R->prof[i];
    return CRT_OK;
}
int crt_renderer_get_section_profile_ex(crt_renderer* R, unsigned long long* out, int n) {
    if (!R || !out || n < 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    for (int i = 0; i < n && i < 8; ++i) out[i] = R->prof[i];
    return CRT_OK;
}
int crt_renderer_get_schedule_stats(crt_renderer* R, unsigned long long* out3) {
    if (!R || !out3) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    out3[0] = R->diag[0]; out3[1] = R->diag[1]; out3[2] = R->diag[2];
    return CRT_OK;
}

float* crt_renderer_linear_device_ptr(crt_renderer* R) { return R ? R->d_sum : nullptr; }
uint8_t* crt_renderer_rgba_device_ptr(crt_renderer* R) { return R ? R->d_rgba.get() : nullptr; }
uint32_t* crt_renderer_rng_device_ptr(crt_renderer* R) { return R ? R->d_rng.get() : nullptr; }

const char* crt_renderer_last_kernel_name(const crt_renderer* R) { return R ? R->kernel_name : ""; }
int crt_renderer_last_launch_frozen(const crt_renderer* R) { return R ? R->last_frozen : 0; }

int crt_renderer_set_tail_fill(crt_renderer* R, int tiles, int spp) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    R->fill_tiles = tiles < 0 ? -1 : tiles;
    R->fill_spp = tiles > 0 ? spp : 0;
    return CRT_OK;
}

int crt_renderer_last_tail_fill(crt_renderer* R, int out[4]) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = R->last_fill[0]; out[1] = R->last_fill[1]; out[2] = out[3] = 0;
    if (out[0] == 0) return CRT_OK;
    HIP_TRY(hipSetDevice(R->device));
    HIP_TRY(hipEventSynchronize(R->last_fill_ev));   // the render's ev1: its copy of the two counts is done
    out[2] = (int)R->h_fill.get()[0];
    out[3] = (int)R->h_fill.get()[1];
    return CRT_OK;
}

#ifdef CRT_PROFILE_PAIRS
extern "C" int crt_profile_pair_hist(unsigned long long* out32, int reset) {
    if (!out32) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_pair_hist), 32 * 8, 0, hipMemcpyDeviceToHost));
    if (reset) {
        static const unsigned long long zero[32] = {};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_pair_hist), zero, sizeof zero, 0, hipMemcpyHostToDevice));
    }
    return CRT_OK;
}
#endif
#ifdef CRT_PROFILE_LIVE
extern "C" int crt_profile_live_hist(unsigned long long* out16, int reset) {
    if (!out16) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_live_hist), 16 * 8, 0, hipMemcpyDeviceToHost));
    if (reset) {
        static const unsigned long long zero[16] = {};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_live_hist), zero, sizeof zero, 0, hipMemcpyHostToDevice));
    }
    return CRT_OK;
}
#endif
#ifdef CRT_PROFILE_PASS
extern "C" int crt_profile_pass_sections(unsigned long long* out20, int reset) {
    if (!out20) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out20, HIP_SYMBOL(g_pass_prof), 20 * 8, 0, hipMemcpyDeviceToHost));
    if (reset) {
        static const unsigned long long zero[20] = {};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_pass_prof), zero, sizeof zero, 0, hipMemcpyHostToDevice));
    }
    return CRT_OK;
}
#endif
#ifdef CRT_PROFILE_LOOPS
extern "C" int crt_profile_loop_counts(unsigned long long* out8, int reset) {
    if (!out8) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_loop_prof), 8 * 8, 0, hipMemcpyDeviceToHost));
    if (reset) {
        static const unsigned long long zero[8] = {};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_loop_prof), zero, sizeof zero, 0, hipMemcpyHostToDevice));
    }
    return CRT_OK;
}
#endif
#ifdef CRT_PROFILE_SITES
extern "C" int crt_profile_site_counts(unsigned long long* out12, int reset) {
    if (!out12) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out12, HIP_SYMBOL(g_site_prof), 12 * 8, 0, hipMemcpyDeviceToHost));
    if (reset) {
        static const unsigned long long zero[12] = {};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_site_prof), zero, sizeof zero, 0, hipMemcpyHostToDevice));
    }
    return CRT_OK;
}
#endif
#ifdef CRT_PROFILE_CRIT_TRACE
// out: 2 x 16384 trace words, then 2 x n_waves HW words
extern "C" int crt_profile_crit_trace(unsigned long long* trace, unsigned* hw, int n_waves) {
    if (!trace || !hw || n_waves <= 0 || n_waves > 4 * 65536) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(trace, HIP_SYMBOL(g_crit_trace), sizeof(unsigned long long) * 2 * 16384, 0,
                                hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpyFromSymbol(hw, HIP_SYMBOL(g_wave_hw), (size_t)n_waves * 8, 0, hipMemcpyDeviceToHost));
    static const unsigned long long zero[2 * 16384] = {};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_crit_trace), zero, sizeof zero, 0, hipMemcpyHostToDevice));
    return CRT_OK;
}
#endif
#ifdef CRT_PROFILE_WAVE_TIMES
extern "C" int crt_profile_wave_times(unsigned long long* out, int n_waves) {
    if (!out || n_waves <= 0 || n_waves > 4 * 65536) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_prof), (size_t)n_waves * 16, 0, hipMemcpyDeviceToHost));
    return CRT_OK;
}
#endif

int crt_renderer_timing_history(crt_renderer* R, int back, float out[3]) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    if (back < 0 || back >= CRT_TIMING_RING) return set_error(CRT_ERR_INVALID_ARGUMENT, "back outside [0, CRT_TIMING_RING)");
    if ((unsigned long long)back >= R->n_timed) return set_error(CRT_ERR_INVALID_ARGUMENT, "fewer renders than back + 1");
    const DevEvent* slot = R->ring[(R->n_timed - 1 - (unsigned long long)back) % (CRT_TIMING_RING + 1)];
    HIP_TRY(hipSetDevice(R->device));
    HIP_TRY(hipEventSynchronize(slot[2].get()));
    HIP_TRY(hipEventElapsedTime(&out[0], slot[0].get(), slot[2].get()));
    HIP_TRY(hipEventElapsedTime(&out[1], slot[0].get(), slot[1].get()));
    HIP_TRY(hipEventElapsedTime(&out[2], slot[1].get(), slot[2].get()));
    return CRT_OK;
}

int crt_renderer_set_temporal_order(crt_renderer* R, int on) {
    if (!R || on < 0 || on > 1) return set_error(CRT_ERR_INVALID_ARGUMENT, "temporal order: 0 or 1");
    R->temporal = on;
    R->pix_rays_valid = false;
    return CRT_OK;
}

int crt_renderer_set_drain_threshold(crt_renderer* R, int lanes) {
    if (!R || lanes < 0 || lanes > 64) return set_error(CRT_ERR_INVALID_ARGUMENT, "drain threshold 0..64");
    R->drain_threshold = lanes;
    return CRT_OK;
}

int crt_renderer_set_wave_drain(crt_renderer* R, int sixty_fourths) {
    if (!R || sixty_fourths < 1 || sixty_fourths > 64) return set_error(CRT_ERR_INVALID_ARGUMENT, "wave drain 1..64");
    R->wave_drain = sixty_fourths;
    return CRT_OK;
}

int crt_renderer_set_xcd_regions(crt_renderer* R, int on) {
    if (!R || on < 0 || on > 1) return set_error(CRT_ERR_INVALID_ARGUMENT, "xcd regions: 0 or 1");
    R->xcd_regions = on;
    return CRT_OK;
}

// The round-4 leaf-pair carry was measured and not kept (+1.8 % / +15 %); its kernels live on as
// profiles/r04c/leaf_carry.patch.  The entry point stays in the ABI and reports that this build has no carry.
int crt_renderer_set_leaf_carry(crt_renderer* R, int lanes, int max_pairs) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "null renderer");
    (void)lanes;
    (void)max_pairs;
    return set_error(CRT_ERR_UNSUPPORTED, "leaf-pair carry: not in this build (measured and removed, DESIGN.md §8; "
                                          "profiles/r04c/leaf_carry.patch)");
}

int crt_renderer_last_schedule(crt_renderer* R, float out[4]) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = R->last_schedule[k];
    return CRT_OK;
}

int crt_renderer_last_timings(crt_renderer* R, float out[3]) {
    if (!R || !out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    if (!R->n_timed) return set_error(CRT_ERR_INVALID_ARGUMENT, "no render yet");
    return crt_renderer_timing_history(R, 0, out);
}

float crt_renderer_last_kernel_ms(crt_renderer* R) {
    float t[3];
    if (!R || !R->n_timed || crt_renderer_timing_history(R, 0, t) != CRT_OK) return -1.f;
    return t[0];
}

}  // extern "C"
