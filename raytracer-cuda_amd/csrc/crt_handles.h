// crt_handles.h — the two handles of the C ABI (crt_scene, crt_renderer), the per-handle states that hang off them, the
// helpers every later header shares (use_device, set_camera_frame, first_use, take_timing_slot) and the entries that
// take no handle.  Host code only.  Included by crt_hip.hip first of the host headers, after the device half: it needs
// set_error / HIP_TRY, crt_devmem.h's buffer types and crt_device.h's constants.
#pragma once

// The per-handle states of the later entries, each allocated by the first call that needs it (first_use) and freed with
// its handle.  `ready` is set once everything in the state is allocated: a state that is not ready could not be allocated.

// Ray queries (crt_trace.h).
struct TraceScratch {
    DevBuf<uint32_t> d_next;
    DevBuf<unsigned long long> d_stats;
    DevBuf<uint32_t> d_ovf;                  // stack entries beyond the LDS part, per grid lane
    DevBuf<crt_ray> d_rays;                  // staging of the host-pointer entries
    DevBuf<crt_hit> d_hits;
    DevBuf<uint8_t> d_occ;
    DevEvent ev0, ev1;
    bool ready = false;
    bool traced = false;
    int n_cus = 0, wg_per_cu = 0;
};

// The wavefront loop's scratch (crt_paths.h).
struct WavefrontScratch {
    DevBuf<crt_ray> rays[2];
    DevBuf<crt_path> paths[2];
    DevBuf<crt_hit> hits;
    DevBuf<int32_t> remaining;
    DevBuf<uint32_t> d_count;
    PinnedBuf<uint32_t> h_count;            // [0] the count, [2..3] the trace error word
    // the queued loop (crt_renderer_render_wavefront_queued): 8 device words and their pinned copy
    DevBuf<uint32_t> d_queue;               // [0], [1] the ping-pong counts, [2] the sticky error word, [4..7] the totals
    PinnedBuf<uint32_t> h_queue;
    DevEvent ev0, ev1;
    bool ready = false;
};

// The renderer's adaptive state (crt_adaptive.h).
struct AdaptiveState {
    DevBuf<float> prev;             // W*H*3: the sums after the first half of the samples a candidate tile holds
    DevBuf<int32_t> tile_spp;       // per tile: samples every pixel of the tile has received
    DevBuf<float> tile_error;       // per tile: the last error estimate
    DevBuf<uint32_t> key;           // per tile: 0 = not listed, else the error as an ordered integer
    DevBuf<uint32_t> ctile;         // the unconverged tiles of the last plan in tile order, n_tiles entries
    DevBuf<uint32_t> ckey;          // their keys
    DevBuf<uint32_t> list;          // the same tiles, largest error first
    DevBuf<uint32_t> d_count;       // their number
    PinnedBuf<uint32_t> h_count;
    DevEvent ev0, ev1;
    bool ready = false;
};

// The renderer's denoiser state (crt_denoise.h).
// Bytes per pixel: rays 32 + hits 32 (compute_guides only) + guides 32 + two colour buffers 2 x 16 + denoised 12 = 140,
// plus one word per 64 pixels (the hit counts).
struct DenoiseState {
    DevBuf<float4> rays;            // 2 rows per pixel: the pixel-centre rays (crt_ray)
    DevBuf<float4> hits;            // 2 rows per pixel: their closest hits (crt_hit)
    DevBuf<float4> guides[2];       // 2 rows per pixel: (normal.xyz, t) (position.xyz, key); [gi] is the current one,
                                    // [1] exists only once the reprojection keeps previous guides (crt_reproject.h)
    int gi = 0;
    bool keep = false;              // guides[gi] is also the reprojection's previous frame: the next guides go to [gi ^ 1]
    crt_camera_desc guide_cam{};    // the camera guides[gi]'s rays were made from (compute_guides)
    DevBuf<float4> col[2];          // 1 row per pixel: (c.xyz, 0)
    DevBuf<float> denoised;         // W*H*3
    DevBuf<uint32_t> wave_hits;     // per 64 pixels: how many of them hit something
    bool ready = false;
    bool have_guides = false;       // guides hold a compute_guides or self-test result
    bool counted = false;           // wave_hits belongs to the guides (compute_guides; not the self-test's upload)
    bool have_denoised = false;
    bool timed_guides = false;
    DevEvent g0, g1, f0, f1;
    DevEvent it[9];                 // a timed run: after the input kernel, then after every iteration
    bool lds_raised = false;        // the tiled kernel's dynamic LDS limit was raised for this device
    int timed_iterations = 0;       // iterations of the last timed run (crt_renderer_denoise_iteration_ms), 0: none
};

// The renderer's reprojection state (crt_reproject.h).  Bytes per pixel: two history buffers of 16-byte rows 32 + the
// second guide buffer 32 = 64, plus one word per wave of the reprojection kernel's grid.
struct ReprojectState {
    DevBuf<float4> hist[2];         // 1 row per pixel: (r, g, b, len); [hi] holds the latest history
    DevBuf<uint32_t> wave_taken;    // per wave of the kernel's grid: how many of its pixels took history
    int hi = 0;
    int prev_gi = 0;                // DenoiseState::guides[prev_gi]: the guides of the frame hist[hi] belongs to
    crt_camera_desc prev_cam{};     // and their guide camera
    bool ready = false;
    bool valid = false;             // hist[hi], guides[prev_gi] and prev_cam describe one earlier frame
    bool have_history = false;      // hist[hi] holds a reprojection's result
    DevEvent e0, e1;
};

// The renderer's variance state (crt_variance.h).  Bytes per pixel: two moment buffers of 8-byte rows 16, allocated by
// the first crt_renderer_reproject_moments, + the variance 4, allocated by the first crt_renderer_denoise_history_variance.
struct VarianceState {
    DevBuf<float2> mom[2];          // 1 row per pixel: (m1, m2) of the luminance; [mi] belongs to ReprojectState::hist[hi]
    DevBuf<float> variance;         // W*H: the estimate kernel's v (crt_renderer_read_variance)
    int mi = 0;
    bool moments_valid = false;     // mom[mi] and hist[hi] describe the same frames (a plain reprojection or a reset ends it)
    bool have_variance = false;
    bool lds_raised = false;        // the variance tiled kernel's dynamic LDS limit was raised for this device
};

struct crt_scene {
    int device = 0;
    DevBuf<float4> d_nodes, d_prims, d_mats;
    DevBuf<float4> d_chain;        // width 4: reference scene-level boxes on the per-ray spheres' paths
    int n_chain = 0;
    DevBuf<float4> d_shade;        // shading record per rank (crt_device.h)
    int n_nodes = 0, n_prims = 0, n_mats = 0, n_ranks = 0;   // n_nodes per layout
    int max_depth = 0;
    int bvh = CRT_BVH_REFERENCE, layouts = 1;
    int width = 2;                 // 2: threaded layouts (variants 0-3); 4: 4-wide nodes (variant 4)
    int stack_cap = 0;             // width 4: traversal-stack entries a ray can need
    int stack_bound = 0;           // width 4: the tree's own bound (stack_cap without the testing override)
    long spatial_splits = 0, references = 0;   // rebuilt tree: SBVH cuts, leaf references
    int sphere_first = 0, n_ray_spheres = 0;   // width 4: spheres tested per ray, prims [first, first + n)
    float sph2[2][12] = {};                    // width 4 with exactly two per-ray spheres: their kernel-argument copy
    int tree_spheres = 1;                      // width 4: some leaf holds a sphere
    long excluded = 0;
    DevBuf<int4> d_ident;          // ray queries: per rank (object, primitive, material, 0), see identity_table
    std::unique_ptr<TraceScratch> trace;    // ray queries: scratch of the handle, allocated on first use (crt_trace.h)
    DevBuf<float4> d_mat_rows;     // path steps: per material (code, 0, 0, 0) (payload), see material_shade_rows
};

constexpr int ERR_WORD = 15;      // d_counters word of the device error flags (RenderParams::err)

struct crt_renderer {
    int device = 0, width = 0, height = 0;
    // the frame's 8x8 tiles (one per wave of the tile schedules, the adaptive state's unit): per row, and in all
    int tiles_x() const { return (width + 7) / 8; }
    int n_tiles() const { return tiles_x() * ((height + 7) / 8); }
    DevBuf<uint32_t> d_rng;
    float* d_sum = nullptr;       // active linear framebuffer (own or attached)
    DevBuf<float> d_sum_own;
    DevBuf<uint8_t> d_rgba;
    DevBuf<uint32_t> d_seq;
    DevBuf<unsigned long long> d_counters;
    crt_camera_desc cam{};
    bool has_camera = false;
    // HIP events of the current render: ev0 before the cost probe, ev_main just before the main render kernel (after
    // the probe and the tile sort), ev1 after it.  They point into a ring of CRT_TIMING_RING frames, so a caller that
    // renders K frames back to back without synchronising can read every frame's phases afterwards
    // (crt_renderer_timing_history).  The ring has one slot more than the history reaches: a render records into slot
    // n_timed % (CRT_TIMING_RING + 1), which none of the last CRT_TIMING_RING complete frames occupies, so a render that
    // fails after its first event (an allocation, the overflow-region check) leaves every readable slot intact.
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_main = nullptr;
    DevEvent ring[CRT_TIMING_RING + 1][3];
    unsigned long long n_timed = 0;   // renders whose three events were all recorded
    char kernel_name[64] = "";     // instantiation of the last render launch, rocprof's spelling
    int last_frozen = 0;           // that launch ran a frozen twin (crt_renderer_last_launch_frozen)
    // variant 7: pixel order, slot queue, probe costs, sort scratch (allocated on first use)
    DevBuf<uint32_t> d_order, d_queue;
    DevBuf<uint32_t> d_tile_cost;      // per-pixel probe costs
    DevBuf<uint32_t> d_order_hist;
    DevBuf<uint32_t> d_tile_key;       // variant 8: per-tile keys
    DevBuf<unsigned long long> d_probe_stats;      // crt_tile_cost_kernel's stats: largest tile work, total work
    PinnedBuf<unsigned long long> h_probe_stats;   // their pinned host copy
    float last_schedule[4] = {0.f, 0.f, 0.f, 0.f};  // crt_renderer_last_schedule
    DevBuf<uint32_t> d_rng_cache;      // curand_init result of (rng_cache_seed, rng_cache_base)
    unsigned long long rng_cache_seed = 0, rng_cache_base = 0;
    bool rng_cache_valid = false;
    int probe_spp = -1;            // samples per pixel of the cost probe; 0 = no probe (8x8-tile order),
                                   // -1 = automatic: 4 for renders of >= 1000 spp, else 2 (profiles/r01ad)
    int probe_min_spp = 64;        // renders with fewer samples per pixel skip the probe
    int tile_key_mode = 2;         // variant 8: see crt_tile_cost_kernel (2: measured best, profiles/r01ac)
    int n_cus = 0;
    int variant = -1;              // see crt_renderer_set_kernel_variant; -1 = automatic
    unsigned long long diag[3] = {0, 0, 0};
    unsigned long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // COUNT-mode section profile (variant 4)
    int regen_threshold = 24;      // variants 2/3
    int regen_threshold_wide = REGEN_THRESHOLD_WIDE;   // variants 4/7/8
    int crit_tiles = -1;           // variant 8: leading tiles of the cost order regenerating at crit_threshold; -1 = 4 per CU
    int tile_shard = 0, tile_shards = 1;   // pixel sharding (crt_renderer_set_pixel_shard)
    int crit_threshold = 16;       // (measured: profiles/r02h, r02i)
    int top_levels = -1;           // 4-wide variants: new rays' first node steps from LDS; -1 = CRT_TOP_LEVELS
    int xcd_regions = 0;           // variant 8: XCD groups render screen strips (crt_xcd_order_kernel)
    int probe_stride = 0;          // variant 8's cost probe: every probe_stride-th pixel in x and y (0 = automatic)
    int temporal = 0;              // variant 7: tiles ordered by the previous variant-7 frame's rays per pixel
    int drain_threshold = 0;       // variant 7: regeneration threshold once the pixel queue is empty (0 = unchanged)
    int wave_drain = WAVE_DRAIN;   // variants 4/8: sixty-fourths of its live lanes a draining wave passes at
    // variant 8, tail fill (crt_renderer_set_tail_fill): fill_tiles < 0 = automatic, 0 = off, else K with fill_spp = delta
    int fill_tiles = -1, fill_spp = 0;
    DevBuf<uint32_t> d_fill;           // the tail parts rendered by the main launch and by the sweep, then one flag per tile rank
    PinnedBuf<uint32_t> h_fill;        // those two counts of the last render with tail fill (copied on its stream before ev1)
    int last_fill[2] = {0, 0};         // K and delta of the last render (0, 0: rendered without tail fill)
    hipEvent_t last_fill_ev = nullptr; // that render's ev1
    DevBuf<uint32_t> d_pix_rays;     // variant 7 with the temporal order: rays per pixel of the last frame
    DevBuf<uint32_t> d_tile_order;    // its tiles, most expensive first
    bool pix_rays_valid = false;
    int min_waves = 0;             // occupancy target (waves/SIMD); 0 = auto: 7 for variant 8 over >= 4 tiles per wave
                                   // slot, 6 for the other 4-wide launches and variants 3 and 10, 5 for variants 0-2
    DevBuf<uint32_t> d_ovf;        // variant 4: stack entries beyond the LDS part, per pixel
    int stack_lds = STACK_LDS;     // variant 4: per-lane stack entries kept in LDS
    float rcp_w = 1.f, rcp_h = 1.f; // RN(1 / width), RN(1 / height)
    int fast_uv = 0;               // next_ray divides by uv_div (verified for this size at creation, uv_div_mismatches)
    std::unique_ptr<WavefrontScratch> wavefront;    // crt_renderer_render_wavefront: batches of the handle, allocated on first use (crt_paths.h)
    std::unique_ptr<AdaptiveState> adaptive;        // crt_renderer_render_adaptive: per-tile state of the handle, allocated on first use (crt_adaptive.h)
    std::unique_ptr<DenoiseState> denoise;          // crt_renderer_compute_guides / crt_renderer_denoise: guides and colour buffers of the handle, allocated on first use (crt_denoise.h)
    std::unique_ptr<ReprojectState> reproject;      // crt_renderer_reproject: history buffers of the handle, allocated on first use (crt_reproject.h)
    std::unique_ptr<VarianceState> variance;        // crt_renderer_reproject_moments / crt_renderer_denoise_history_variance: moments and variance of the handle, allocated on first use (crt_variance.h)
};

namespace {
int use_device(int dev) {
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (n <= 0) return set_error(CRT_ERR_NO_DEVICE, "no HIP device visible");
    if (dev < 0 || dev >= n) return set_error(CRT_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    HIP_TRY(hipSetDevice(dev));
    return CRT_OK;
}

// The renderer's camera and frame, the inputs of cam_regs(), into any kernel's parameter struct that carries them
// (RenderParams, crt_paths.h's CameraRaysParams and PathAdvanceParams).
template <class Params>
void set_camera_frame(Params& P, const crt_renderer* R) {
    P.cam = R->cam;
    P.width = R->width; P.height = R->height;
    P.rcp_w = R->rcp_w; P.rcp_h = R->rcp_h; P.fast_uv = R->fast_uv;
}

// The host object of a per-handle state.  Whatever it comes to hold is freed with the handle.
template <class T>
int new_state(std::unique_ptr<T>& slot) {
    slot.reset(new (std::nothrow) T);
    return slot ? CRT_OK : set_error(CRT_ERR_OUT_OF_MEMORY, "host allocation failed");
}

// A per-handle state on its first use: `slot` is made, init(T*) -> int allocates and initialises what it holds (HIP_TRY
// works inside it), then the state is ready.  One whose init failed stays, not ready: later calls get `refused`.
template <class T, class Init>
int first_use(std::unique_ptr<T>& slot, const char* refused, T** out, Init init) {
    if (!slot) {
        if (int rc = new_state(slot)) return rc;
        if (int rc = init(slot.get())) return rc;
        slot->ready = true;
    }
    if (!slot->ready) return set_error(CRT_ERR_OUT_OF_MEMORY, refused);
    *out = slot.get();
    return CRT_OK;
}

// A render's slot of the timing ring into ev0, ev_main, ev1: the spare slot, which no readable frame occupies (crt_renderer).
void take_timing_slot(crt_renderer* R) {
    const DevEvent* slot = R->ring[R->n_timed % (CRT_TIMING_RING + 1)];
    R->ev0 = slot[0].get(); R->ev_main = slot[1].get(); R->ev1 = slot[2].get();
}
}  // namespace

extern "C" {   // the entries that take no handle

int crt_abi_version(void) { return CRT_ABI_VERSION; }
int crt_build_flags(void) {
#ifdef CRT_CHECKED
    return CRT_BUILD_CHECKED;
#else
    return 0;
#endif
}
const char* crt_last_error(void) { return g_last_error.c_str(); }

int crt_device_count(int* out) {
    if (!out) return set_error(CRT_ERR_INVALID_ARGUMENT, "null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *out = (e == hipSuccess) ? n : 0;
    return CRT_OK;
}

int crt_debug_live_allocations(int64_t* buffers, int64_t* bytes) {
    if (!buffers || !bytes) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    *buffers = g_live_buffers.load();
    *bytes = g_live_bytes.load();
    return CRT_OK;
}

}  // extern "C"
