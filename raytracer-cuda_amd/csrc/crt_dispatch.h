// crt_dispatch.h — the render dispatch: the host code that launches the render kernels and the schedule kernels (the
// counting sort, the tile keys, the XCD regions, the tile and pixel-slot orders; all in crt_hip.hip): the launch table
// (RENDER_ROWS), launch_render, the order buffers and sorts, render_params, the choice of variant and occupancy, the three
// schedules (render_grid, render_tiles, render_pixel_queue) and crt_renderer_render.  Included by crt_hip.hip after
// crt_renderer.h; needs crt_handles.h and every instantiation of crt_render_kernel and its open twin.  Host code only.
#pragma once

// Cost-probe samples for a render of `spp` samples per pixel (0 = no probe).
static int probe_spp_for(const crt_renderer* R, int spp) {
    if (spp < R->probe_min_spp || R->probe_spp == 0) return 0;
    return R->probe_spp > 0 ? R->probe_spp : (spp >= 1000 ? 4 : 2);
}

// ---- render dispatch: every instantiation of crt_render_kernel the library launches, one row per (VARIANT, MINW) ----
using RenderKernel = void (*)(RenderParams);
struct RenderRow {
    int variant, w;
    RenderKernel plain, counting;   // COUNT = false / true; counting is null where that kernel is not built
    RenderKernel open;              // variant 8: the plain kernel's open twin (crt_render_open_kernel); else null
};
#define CRT_ROW(V, W) {V, W, crt_render_kernel<false, V, W>, crt_render_kernel<true, V, W>, nullptr}
#define CRT_ROW_PLAIN8(W) {8, W, crt_render_kernel<false, 8, W>, nullptr, crt_render_open_kernel<8, W>}
#define CRT_ROW8(W) {8, W, crt_render_kernel<false, 8, W>, crt_render_kernel<true, 8, W>, crt_render_open_kernel<8, W>}
static constexpr RenderRow RENDER_ROWS[] = {
    CRT_ROW(0, 1), CRT_ROW(1, 1),
    CRT_ROW(2, 1), CRT_ROW(2, 5), CRT_ROW(2, 6), CRT_ROW(2, 8),
    CRT_ROW(3, 1), CRT_ROW(3, 4), CRT_ROW(3, 5), CRT_ROW(3, 6),
    CRT_ROW(4, 1), CRT_ROW(4, 4), CRT_ROW(4, 5), CRT_ROW(4, 6), CRT_ROW(4, 7),
    CRT_ROW(7, 5), CRT_ROW(7, 6), CRT_ROW(7, 7),
    CRT_ROW_PLAIN8(4),   // the row prefetch (profiles/r06r, r06s); the counting kernel runs at 5
    CRT_ROW8(5), CRT_ROW8(6), CRT_ROW8(7),
    CRT_ROW(10, 5), CRT_ROW(10, 6), CRT_ROW(10, 7),
};
#undef CRT_ROW
#undef CRT_ROW_PLAIN8
#undef CRT_ROW8

// The row of `variant` for an occupancy target of `occ` waves per SIMD: the largest built MINW <= occ, else the
// smallest built.  Returns an index into RENDER_ROWS.
static constexpr int render_row(int variant, bool cnt, int occ) {
    int best = -1, smallest = -1;
    for (int i = 0; i < (int)(sizeof RENDER_ROWS / sizeof RENDER_ROWS[0]); ++i) {
        const RenderRow& r = RENDER_ROWS[i];
        if (r.variant != variant || (cnt && !r.counting)) continue;
        if (r.w <= occ && (best < 0 || r.w > RENDER_ROWS[best].w)) best = i;
        if (smallest < 0 || r.w < RENDER_ROWS[smallest].w) smallest = i;
    }
    return best >= 0 ? best : smallest;
}
// MINW chosen at occ = 1..8, one decimal digit each
static constexpr int render_row_digits(int variant, bool cnt) {
    int d = 0;
    for (int occ = 1; occ <= 8; ++occ) d = d * 10 + RENDER_ROWS[render_row(variant, cnt, occ)].w;
    return d;
}
static_assert(render_row_digits(4, false) == 11145677 && render_row_digits(4, true) == 11145677, "variant 4");
static_assert(render_row_digits(7, false) == 55555677 && render_row_digits(7, true) == 55555677, "variant 7");
static_assert(render_row_digits(8, false) == 44445677, "variant 8, plain");
static_assert(render_row_digits(8, true) == 55555677, "variant 8, counting");
static_assert(render_row_digits(10, false) == 55555677 && render_row_digits(10, true) == 55555677, "variant 10");
static_assert(render_row_digits(3, false) == 11145666 && render_row_digits(3, true) == 11145666, "variant 3");
static_assert(render_row_digits(2, false) == 11115668 && render_row_digits(2, true) == 11115668, "variant 2");
static_assert(render_row_digits(0, false) == 11111111 && render_row_digits(0, true) == 11111111, "variant 0");
static_assert(render_row_digits(1, false) == 11111111 && render_row_digits(1, true) == 11111111, "variant 1");

// Whether a launch of `row` with P over scene S may run the frozen twin: the plain variant-8 kernel, and every fact
// that crt_render_body.inc holds as a constant when FROZEN is true of this launch.  A knob moved by a setter, another
// per-ray sphere count, spheres in the tree, fewer LDS stack entries than the kernel's or a probe launch runs the open
// twin, and so does a scene with a stack_cap override (a testing option that must report what it drops).  The stack
// fact is "an entry below the kernel's LDS entries is kept in LDS": P.stack_lds is all of them, or it is the tree's
// own bound and that bound lies within them, so no traversal reaches an entry where the twins could differ.
static bool render_launch_frozen(const RenderRow& row, bool cnt, const RenderParams& P, const crt_scene* S) {
    if (!row.open || cnt) return false;
    const int sd = wide_stack_entries(row.w);
    const bool own_bound = S->stack_cap == S->stack_bound;   // no stack_cap override
    const bool stack = own_bound && (P.stack_lds == sd || (S->stack_cap < sd && P.stack_lds == S->stack_cap));
    return stack && P.top_levels == CRT_TOP_LEVELS && P.tree_spheres == 0 && P.n_ray_spheres == 2 && P.n_layouts == 1 &&
           !P.probe_cost && !P.pix_rays && P.wave_drain == WAVE_DRAIN && P.regen_threshold == REGEN_THRESHOLD_WIDE;
}

// The main launch of a render: names it (rocprofv3's spelling; both twins of a plain variant-8 kernel carry the frozen
// one's name, crt_renderer_last_launch_frozen tells them apart), records ev_main immediately before it.  S: the scene,
// required for the rows that have twins (variant 8), where the choice of the twin reads it.
static int launch_render(crt_renderer* R, const RenderRow& row, bool cnt, dim3 grid, dim3 block, hipStream_t st,
                         const RenderParams& P, const crt_scene* S = nullptr) {
    std::snprintf(R->kernel_name, sizeof R->kernel_name, "crt_render_kernel<%s, %d, %d>", cnt ? "true" : "false",
                  row.variant, row.w);
    if (row.open && !S) return set_error(CRT_ERR_INVALID_ARGUMENT, "launch_render: a variant-8 launch needs its scene");
    R->last_frozen = render_launch_frozen(row, cnt, P, S) ? 1 : 0;
    HIP_TRY(hipEventRecord(R->ev_main, st));
    RenderParams Q = P;
    // frozen: the stack fact as the kernel states it (a smaller own bound: see above)
    if (R->last_frozen) Q.stack_lds = wide_stack_entries(row.w);
    const RenderKernel kernel = R->last_frozen ? row.plain : cnt ? row.counting : row.open ? row.open : row.plain;
    R->last_fill[0] = R->last_fill[1] = 0;
    if (row.variant != 8 || !P.queue) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, Q);
        return CRT_OK;
    }
    // Tail fill (render_tiles set it up; fill_prologue): the grid's blocks are the heads, K tail parts follow them, and
    // a sweep of tail parts only renders the ranks whose tail part found its head unfinished.  Both launches lie
    // between ev_main and ev1.
    const int k = P.drain_threshold, delta = P.probe_stride;
    HIP_TRY(hipMemsetAsync(R->d_fill.get(), 0, ((size_t)k + 2) * sizeof(uint32_t), st));
    Q.n_slots = (int)grid.x;
    hipLaunchKernelGGL(kernel, dim3(grid.x + (unsigned)k), block, 0, st, Q);
    Q.n_slots = 0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)k), block, 0, st, Q);
    HIP_TRY(hipMemcpyAsync(R->h_fill.get(), R->d_fill.get(), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    R->last_fill[0] = k;
    R->last_fill[1] = delta;
    R->last_fill_ev = R->ev1;
    return CRT_OK;
}

// Order, queue, probe-cost and sort buffers of the tile and pixel-queue schedules, allocated on first use (one stream
// synchronisation before the first allocation), and the device's CU count.
static int ensure_order_buffers(crt_renderer* R, hipStream_t st, size_t n_pix, int n_tiles, bool want_tile_key) {
    if (R->d_order && (R->d_tile_key || !want_tile_key)) return CRT_OK;
    HIP_TRY(hipStreamSynchronize(st));
    if (!R->d_order) {
        HIP_TRY(R->d_order.alloc(std::max(n_pix, (size_t)n_tiles * 64)));
        HIP_TRY(R->d_queue.alloc(1));
        HIP_TRY(R->d_tile_cost.alloc(n_pix));
        HIP_TRY(R->d_order_hist.alloc(ORDER_KEYS));
        HIP_TRY(R->d_fill.alloc((size_t)n_tiles + 2));
        HIP_TRY(R->h_fill.alloc(2));
        HIP_TRY(hipDeviceGetAttribute(&R->n_cus, hipDeviceAttributeMultiprocessorCount, R->device));
    }
    if (want_tile_key && !R->d_tile_key) HIP_TRY(R->d_tile_key.alloc((size_t)n_tiles));
    return CRT_OK;
}

// out = the indices 0..n-1, largest key first (counting sort over ORDER_KEYS buckets).
static int sort_descending(crt_renderer* R, hipStream_t st, const uint32_t* keys, int n, uint32_t* out) {
    const unsigned ob = (unsigned)((n + ORDER_ITEMS - 1) / ORDER_ITEMS);
    HIP_TRY(hipMemsetAsync(R->d_order_hist.get(), 0, ORDER_KEYS * 4, st));
    hipLaunchKernelGGL(crt_order_hist_kernel, dim3(ob), dim3(256), 0, st, keys, n, R->d_order_hist.get());
    hipLaunchKernelGGL(crt_order_scan_kernel, dim3(1), dim3(ORDER_KEYS), 0, st, R->d_order_hist.get());
    hipLaunchKernelGGL(crt_order_scatter_kernel, dim3(ob), dim3(256), 0, st, keys, n, R->d_order_hist.get(), out, 0u);
    return CRT_OK;
}

// After a cost probe wrote per-pixel costs (every stride-th pixel in x and y) to d_tile_cost: per-tile keys, this
// shard's tiles most expensive first in d_order.  With `stats` the largest tile work and the total work are copied to
// h_probe_stats on the stream (the caller synchronises).
static int order_tiles_by_probe(crt_renderer* R, hipStream_t st, int stride, bool stats, int shard, int shards) {
    const size_t n_pix = (size_t)R->width * R->height;
    const int tiles_x = R->tiles_x(), n_tiles = R->n_tiles();
    const dim3 tgrid((n_tiles + 255) / 256), tblock(256);
    if (stats) {
        if (!R->d_probe_stats) {
            HIP_TRY(R->d_probe_stats.alloc(2));
            HIP_TRY(R->h_probe_stats.alloc(2));
        }
        HIP_TRY(hipMemsetAsync(R->d_probe_stats.get(), 0, 2 * sizeof(unsigned long long), st));
    }
    hipLaunchKernelGGL(crt_tile_cost_kernel, tgrid, tblock, 0, st, R->d_tile_cost.get(), R->width, R->height, tiles_x, n_tiles,
                       R->d_tile_key.get(), R->tile_key_mode, stride, stats ? R->d_probe_stats.get() : nullptr);
    if (stats) HIP_TRY(hipMemcpyAsync(R->h_probe_stats.get(), R->d_probe_stats.get(), 2 * sizeof(unsigned long long),
                                      hipMemcpyDeviceToHost, st));
    if (R->tile_key_mode == 2) {   // per-pixel costs are no longer needed: reuse them for the smoothed keys
        hipLaunchKernelGGL(crt_tile_neighbour_kernel, tgrid, tblock, 0, st, R->d_tile_key.get(), tiles_x, n_tiles, R->d_tile_cost.get());
        HIP_TRY(hipMemcpyAsync(R->d_tile_key.get(), R->d_tile_cost.get(), (size_t)n_tiles * 4, hipMemcpyDeviceToDevice, st));
    }
    if (shards > 1)
        hipLaunchKernelGGL(crt_tile_shard_mask_kernel, tgrid, tblock, 0, st, R->d_tile_key.get(), n_tiles, shard, shards);
    if (int rc = sort_descending(R, st, R->d_tile_key.get(), n_tiles, R->d_order.get())) return rc;
    // XCD regions: the per-pixel costs are dead by now, so they hold the strips' lists and the pool (9 n_tiles)
    if (R->xcd_regions && shards == 1 && tiles_x <= 2048 && n_pix >= (size_t)9 * n_tiles)
        hipLaunchKernelGGL(crt_xcd_order_kernel, dim3(1), dim3(1024), 0, st, R->d_order.get(), R->d_tile_key.get(), n_tiles, tiles_x,
                           R->d_tile_cost.get(), R->d_tile_cost.get() + (size_t)8 * n_tiles);
    return CRT_OK;
}

// Pixel sharding without the probe: d_order[k] = this shard's k-th tile in row order.
static void shard_tiles_in_row_order(crt_renderer* R, hipStream_t st, int n_tiles, int shard, int shards) {
    hipLaunchKernelGGL(crt_shard_tiles_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, st, R->d_order.get(), n_tiles,
                       shard, shards);
}

static RenderParams render_params(const crt_renderer* R, const crt_scene* S, int spp, int max_bounces, unsigned flags) {
    RenderParams P{};   // no order, queue, probe costs, overflow stack or ray counts: the schedules set what they use
    P.nodes = S->d_nodes.get(); P.prims = S->d_prims.get(); P.mats = S->d_mats.get(); P.shade = S->d_shade.get();
    P.n_nodes = S->n_nodes; P.n_mats = S->n_mats; P.n_prims = S->n_prims; P.n_layouts = S->layouts;
    P.err = reinterpret_cast<unsigned*>(R->d_counters.get() + ERR_WORD);
    set_camera_frame(P, R);
    P.spp = spp; P.max_bounces = max_bounces;
    P.accumulate = (flags & CRT_RENDER_ACCUMULATE) ? 1 : 0;
    P.rng = R->d_rng.get(); P.sum = R->d_sum; P.counters = R->d_counters.get();
    P.probe_stride = 1;
    P.crit_threshold = 64;
    P.top_levels = R->top_levels < 0 ? CRT_TOP_LEVELS : R->top_levels;
    P.stack_cap = S->stack_cap;
    P.sphere_first = S->sphere_first;
    P.n_ray_spheres = S->n_ray_spheres;
    P.sphere_chain = S->d_chain.get();
    P.n_chain = S->n_chain;
    P.tree_spheres = S->tree_spheres;
    std::memcpy(P.sph2, S->sph2, sizeof P.sph2);
    P.regen_threshold = S->width == 4 ? R->regen_threshold_wide : R->regen_threshold;
    P.drain_threshold = R->drain_threshold > 0 ? R->drain_threshold : P.regen_threshold;
    P.wave_drain = R->wave_drain;
    return P;
}

// 4-wide scenes: variant 4 / 7 / 8 when selected explicitly; otherwise the measured best (profiles/r01w): 8
// (probe-ordered tiles, one wave per workgroup) when the render runs the cost probe, 7 (lanes refill from a pixel
// queue) for short renders such as the 1-spp interactive frames.  Pixel sharding is variant 8.
// Threaded scenes (the bit-exact reference BVH, rebuilt width 2): variants 0-3 and 10 when selected explicitly;
// otherwise 10 (variant 3 over probe-ordered 8x8 tiles, one wave per workgroup; -17 %, profiles/r03s) when the render
// runs the cost probe, else 3.
static int choose_variant(const crt_renderer* R, const crt_scene* S, int spp) {
    const int v = R->variant;
    const bool probe = probe_spp_for(R, spp) > 0;
    if (R->tile_shards > 1) return 8;
    if (S->width == 4) return v == 4 || v == 7 || v == 8 ? v : probe ? 8 : 7;
    return (v >= 0 && v <= 3) || v == 10 ? v : probe ? 10 : 3;
}

// Per-lane stack entries in LDS at an occupancy target.  A stack_cap override below the LDS entries must still report
// the entries it drops (crt_scene_options.stack_cap).
static int stack_lds_for(const crt_renderer* R, const crt_scene* S, int occ) {
    const int lds = std::min(R->stack_lds, occ >= 7 ? CRT_STACK7 : occ >= 6 ? CRT_STACK6 : STACK_LDS);
    return S->width == 4 && S->stack_cap > 0 ? std::min(lds, S->stack_cap) : lds;
}

// Occupancy target (waves per SIMD): variant 8 runs at 7 (72 VGPRs, 8 LDS stack entries so that 28 one-wave
// workgroups fit a CU's LDS; -2.4 % on config C, profiles/r03aj) when its frame has at least 4 tiles per wave slot,
// else at 6, or at 4 with the row prefetch when the cost probe shows a chain-bound frame: a frame with few tiles per
// slot can end with its most expensive tiles' sequential sample chains (config B, 2 tiles per slot: +3.3 % at 7,
// profiles/r03ak), and the prefetch takes the node rows' wait off every iteration of a chain (B -8 % against
// occupancy 6, profiles/r06r-r06u; where the frame is not chain-bound the lost waves cost more: the plain Cornell box
// at 1280x720 +15 %, 1600x900 +17 %, C +24 %; profiles/r06y).  The other 4-wide variants run at 6, threaded scenes
// at 5.
// Variants 10 and 3 (threaded, bit-exact) run at 6 (80 VGPRs; -8.0 % and -4.8 % against 5, profiles/r03am, r03as).
// *auto_small: variant 8, automatic occupancy, few tiles per slot: render_tiles picks 4 or 6 from the probe's statistics.
static int choose_occupancy(const crt_renderer* R, const crt_scene* S, int variant, bool cnt, int spp, bool* auto_small) {
    *auto_small = false;
    if (R->min_waves) return R->min_waves;
    if (variant != 8) return S->width == 4 || variant == 10 || variant == 3 ? 6 : 5;
    const size_t n_tiles = (size_t)R->n_tiles() / (size_t)R->tile_shards;
    // at least 4 tiles per wave slot: occupancy 7 (throughput).  Fewer: 6, or 4 when the cost probe's tile works
    // show a chain-bound frame (decided after the sort, in render_tiles; without the probe there is nothing to
    // decide on, and the tile count alone cannot tell: at 1280x720 the bunny gains 8 % at 4 and the plain Cornell
    // box loses 16 %, profiles/r06x).  (The counting kernel keeps 6: its counts do not depend on the schedule.)
    const int occ = n_tiles >= (size_t)4 * R->n_cus * 4 * 7 ? 7 : 6;   // n_cus: ensure_order_buffers
    *auto_small = occ < 7 && !cnt && probe_spp_for(R, spp) > 0;
    return occ;
}

// 4-wide scenes whose stack_cap exceeds the LDS entries: the region of the deeper entries, grown when needed.
static int ensure_overflow_stack(crt_renderer* R, const crt_scene* S, hipStream_t st, RenderParams& P) {
    if (S->width != 4 || S->stack_cap <= P.stack_lds) return CRT_OK;
    const size_t need = (size_t)(S->stack_cap - P.stack_lds);
    if (need * R->width * R->height * 4 >= ((size_t)1 << 32))
        return set_error(CRT_ERR_INVALID_ARGUMENT, "traversal-stack overflow region would exceed 4 GiB");
    if (need * R->width * R->height > R->d_ovf.size()) {   // grow the overflow stack region (rarely needed)
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(R->d_ovf.grow(need * R->width * R->height));
    }
    P.ovf = R->d_ovf.get();
    return CRT_OK;
}

// Variants 0-4: one 16x16 block of four waves per workgroup over the whole frame.
static int render_grid(crt_renderer* R, hipStream_t st, const RenderParams& P, bool cnt, int variant, int occ) {
    const dim3 grid((R->width + 15) / 16, (R->height + 15) / 16);
    return launch_render(R, RENDER_ROWS[render_row(variant, cnt, occ)], cnt, grid, dim3(256), st, P);
}

// Variants 8 and 10: one 8x8 tile per one-wave workgroup, most expensive first by a cost probe (variant 4's counting
// kernel for 8, variant 3's for 10, read-only); without the probe, tiles in row order.
static int render_tiles(crt_renderer* R, const crt_scene* S, hipStream_t st, RenderParams& P, bool cnt, int spp,
                        int variant, int occ, bool auto_small) {
    const int tiles_x = R->tiles_x(), n_tiles = R->n_tiles();
    const int shard = R->tile_shard, shards = R->tile_shards;   // one shard for threaded scenes (rejected otherwise)
    P.tiles_x = tiles_x;
    if (probe_spp_for(R, spp) > 0) {
        RenderParams Q = P;
        Q.spp = probe_spp_for(R, spp);
        Q.accumulate = 0;
        Q.probe_cost = R->d_tile_cost.get();
        if (variant == 8) {
            // every stride-th pixel in x and y; automatic: 2 below 1000 spp, where the probe is a larger share of the
            // frame (a 250-spp rank share: probe 3.2 -> 1.2 ms, render -0.9 %; at 2000 spp the render is unchanged,
            // profiles/r04f)
            Q.probe_stride = R->probe_stride ? R->probe_stride : (spp >= 1000 ? 1 : 2);
            const int ps = 16 * Q.probe_stride;
            const dim3 pgrid((R->width + ps - 1) / ps, (R->height + ps - 1) / ps);
            if (occ >= 6) hipLaunchKernelGGL((crt_render_kernel<true, 4, 6>), pgrid, dim3(256), 0, st, Q);
            else hipLaunchKernelGGL((crt_render_kernel<true, 4, 5>), pgrid, dim3(256), 0, st, Q);
        } else {
            const dim3 grid((R->width + 15) / 16, (R->height + 15) / 16);
            hipLaunchKernelGGL((crt_render_kernel<true, 3, 5>), grid, dim3(256), 0, st, Q);
        }
        if (int rc = order_tiles_by_probe(R, st, Q.probe_stride, auto_small, shard, shards)) return rc;
        P.order = R->d_order.get();
        if (variant == 8) {
            P.crit_tiles = R->crit_tiles < 0 ? 4 * R->n_cus : R->crit_tiles;
            P.crit_threshold = R->crit_threshold;
        }
        if (auto_small) {
            // Chain-bound or not, from the probe's tile works: rho = the largest tile's work over the mean work per
            // wave slot at occupancy 6 (this rank's share of the tiles when pixel-sharded).  rho > 1 means the most
            // expensive tile alone outlasts an even spread of the frame over the slots; above CRT_CHAIN_RHO the frame
            // runs at occupancy 4 with the row prefetch, which shortens every chain iteration (-9 %) and gives up a
            // third of the wave slots (profiles/r06x, r06y: config B rho 2.0, -7.6 %; the plain Cornell box at the
            // same size rho 0.8, +15 % at 4).  One host synchronisation after the sort.
            HIP_TRY(hipStreamSynchronize(st));
            const double mx = (double)R->h_probe_stats.get()[0];
            const double mine = (double)R->h_probe_stats.get()[1] / shards;
            const double rho = mine > 0 ? mx * (4.0 * R->n_cus * 6) / mine : 0.0;
            if (rho > CRT_CHAIN_RHO) {
                occ = 4;
                P.stack_lds = stack_lds_for(R, S, occ);
            }
            R->last_schedule[0] = (float)rho;
            R->last_schedule[2] = (float)mx;
            R->last_schedule[3] = (float)(mine / std::max(1, n_tiles / shards));
        }
    } else if (shards > 1) {   // pixel shard without the probe: this shard's tiles in row order
        shard_tiles_in_row_order(R, st, n_tiles, shard, shards);
        P.order = R->d_order.get();
    }
    if (P.crit_tiles > 0) P.crit_tiles = (P.crit_tiles + shards - 1) / shards;
    if (variant == 8) R->last_schedule[1] = (float)occ;
    if (variant == 8 && !cnt && shards == 1 && R->fill_tiles != 0) {
        // Tail fill (fill_prologue).  Automatic: where the launch is long against its items, i.e. the
        // probe-ordered launch at the automatic occupancy 7 (at least 4 tiles per wave slot), the first
        // CRT_FILL_TILES_NUM / CRT_FILL_TILES_DEN of the cost order hold back spp / CRT_FILL_SPP_DEN samples, unless that
        // is fewer than CRT_FILL_MIN_SPP.  A delta outside 1..spp-1 renders without it.
        int k = R->fill_tiles, delta = R->fill_spp;
        if (k < 0) {
            const bool on = CRT_FILL_AUTO && P.order && probe_spp_for(R, spp) > 0 && !R->min_waves && occ == 7;
            k = on ? (int)((long long)n_tiles * CRT_FILL_TILES_NUM / CRT_FILL_TILES_DEN) : 0;
            delta = spp / CRT_FILL_SPP_DEN;
            if (delta < CRT_FILL_MIN_SPP) k = 0;
        }
        k = std::min(k, n_tiles);
        if (k > 0 && delta >= 1 && delta <= spp - 1) {
            P.queue = R->d_fill.get();     // the tail fill's arguments (see RenderParams)
            P.drain_threshold = k;
            P.probe_stride = delta;
        }
    }
    const dim3 tgrid((unsigned)((n_tiles - shard + shards - 1) / shards));
    return launch_render(R, RENDER_ROWS[render_row(variant, cnt, occ)], cnt, tgrid, dim3(64), st, P, S);
}

// Variant 7 without the probe: d_order = the n_tiles * 64 pixel slots of the 8x8 tiles, the tiles most expensive first
// by d_pix_rays (temporal order, once a frame has written it) or in row order.  Allocates the temporal buffers on
// first use (one stream synchronisation).
static int order_tile_slots(crt_renderer* R, hipStream_t st) {
    const size_t n_pix = (size_t)R->width * R->height;
    const int tiles_x = R->tiles_x(), n_tiles = R->n_tiles();
    const size_t n_tile_slots = (size_t)n_tiles * 64;
    if (R->temporal && !R->d_pix_rays) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(R->d_pix_rays.alloc(n_pix));
        HIP_TRY(R->d_tile_order.alloc((size_t)n_tiles));
        if (!R->d_tile_key) HIP_TRY(R->d_tile_key.alloc((size_t)n_tiles));
        R->pix_rays_valid = false;
    }
    const dim3 sgrid((unsigned)((n_tile_slots + 255) / 256));
    if (R->temporal && R->pix_rays_valid) {
        // the interactive loop's frames repeat the last frame's cost map: its rays per pixel -> tile keys (the
        // slowest pixel, raised to 3/4 of the neighbours', as variant 8's probe keys) -> tiles most expensive
        // first, so the long paths start early and the launch does not end with them (profiles/r04i: a 1-spp
        // frame in row order spends its last 31 % draining)
        hipLaunchKernelGGL(crt_tile_cost_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, st, R->d_pix_rays.get(),
                           R->width, R->height, tiles_x, n_tiles, R->d_tile_order.get(), 0, 1, nullptr);
        hipLaunchKernelGGL(crt_tile_neighbour_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, st,
                           R->d_tile_order.get(), tiles_x, n_tiles, R->d_tile_key.get());
        if (int rc = sort_descending(R, st, R->d_tile_key.get(), n_tiles, R->d_tile_order.get())) return rc;
        hipLaunchKernelGGL(crt_expand_tile_order_kernel, sgrid, dim3(256), 0, st, R->d_tile_order.get(), R->d_order.get(),
                           R->width, R->height, (int)n_tile_slots);
    } else {
        hipLaunchKernelGGL(crt_order_tiles_kernel, sgrid, dim3(256), 0, st, R->d_order.get(), R->width, R->height,
                           (int)n_tile_slots);
    }
    return CRT_OK;
}

// Variant 7: persistent workgroups whose lanes refill from a queue of pixel slots, ordered by a per-pixel cost probe,
// by the previous frame's rays per pixel (temporal), or in 8x8-tile order.
static int render_pixel_queue(crt_renderer* R, hipStream_t st, RenderParams& P, bool cnt, int spp, int occ) {
    const size_t n_pix = (size_t)R->width * R->height;
    const size_t n_tile_slots = (size_t)R->n_tiles() * 64;
    if (probe_spp_for(R, spp) > 0) {
        // cost probe: variant 4 at probe_spp samples over the same RNG state, read-only: rays per pixel
        RenderParams Q = P;
        Q.spp = probe_spp_for(R, spp);
        Q.accumulate = 0;
        Q.probe_cost = R->d_tile_cost.get();
        const dim3 grid((R->width + 15) / 16, (R->height + 15) / 16);
        if (occ >= 6) hipLaunchKernelGGL((crt_render_kernel<false, 4, 6>), grid, dim3(256), 0, st, Q);
        else hipLaunchKernelGGL((crt_render_kernel<false, 4, 5>), grid, dim3(256), 0, st, Q);
        if (int rc = sort_descending(R, st, R->d_tile_cost.get(), (int)n_pix, R->d_order.get())) return rc;
        P.n_slots = (int)n_pix;
    } else {
        if (int rc = order_tile_slots(R, st)) return rc;
        P.n_slots = (int)n_tile_slots;
        if (R->temporal) {
            P.pix_rays = R->d_pix_rays.get();
            R->pix_rays_valid = true;
        }
    }
    HIP_TRY(hipMemsetAsync(R->d_queue.get(), 0, 4, st));
    P.order = R->d_order.get();
    P.queue = R->d_queue.get();
    P.probe_cost = nullptr;
    const RenderRow& row = RENDER_ROWS[render_row(7, cnt, occ)];
    const int per_cu = row.w;        // workgroups of 4 waves resident per CU
    const int n_wg = std::max(1, std::min(R->n_cus * per_cu, (int)((n_pix + 255) / 256)));
    return launch_render(R, row, cnt, dim3(n_wg), dim3(256), st, P);
}

extern "C" {

int crt_renderer_render(crt_renderer* R, const crt_scene* S, int spp, int max_bounces, unsigned flags, void* stream) {
    if (!R || !S) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, "camera not set");
    if (spp < 0 || max_bounces < 0) return set_error(CRT_ERR_INVALID_ARGUMENT, "negative spp / bounces");
    if (S->device != R->device) return set_error(CRT_ERR_INVALID_ARGUMENT, "scene and renderer on different devices");
    HIP_TRY(hipSetDevice(R->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(R->d_counters.get(), 0, ERR_WORD * sizeof(unsigned long long), st));   // the error word stays
    RenderParams P = render_params(R, S, spp, max_bounces, flags);
    const bool cnt = (flags & CRT_RENDER_COUNT_WORK) != 0;
    if (R->tile_shards > 1) {
        // pixel sharding: variant 8 renders this shard's tiles; every other pixel of the framebuffer is 0, so the sum
        // of the shards' framebuffers (one collective) is the unsharded frame exactly (x + 0 = x).  Checked and
        // cleared before ev0, so a rejected call leaves the previous frame's timings intact and the clear is not
        // counted as probe/sort time.
        if (S->width != 4) return set_error(CRT_ERR_UNSUPPORTED, "pixel sharding needs a 4-wide rebuilt scene (variant 8)");
        if (P.accumulate) return set_error(CRT_ERR_INVALID_ARGUMENT, "pixel sharding does not accumulate");
        HIP_TRY(hipMemsetAsync(R->d_sum, 0, (size_t)R->width * R->height * 3 * sizeof(float), st));
    }
    take_timing_slot(R);
    HIP_TRY(hipEventRecord(R->ev0, st));
    const int variant = choose_variant(R, S, spp);
    const bool tiles = variant == 8 || variant == 10, queue = variant == 7;
    if (tiles || queue) {
        const size_t n_pix = (size_t)R->width * R->height;
        if (int rc = ensure_order_buffers(R, st, n_pix, R->n_tiles(), tiles)) return rc;
    }
    bool auto_small = false;
    const int occ = choose_occupancy(R, S, variant, cnt, spp, &auto_small);
    R->last_schedule[0] = R->last_schedule[1] = R->last_schedule[2] = R->last_schedule[3] = 0.f;
    P.stack_lds = stack_lds_for(R, S, occ);
    if (int rc = ensure_overflow_stack(R, S, st, P)) return rc;
    int rc;
    if (tiles) rc = render_tiles(R, S, st, P, cnt, spp, variant, occ, auto_small);
    else if (queue) rc = render_pixel_queue(R, st, P, cnt, spp, occ);
    else rc = render_grid(R, st, P, cnt, variant, occ);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(R->ev1, st));
    ++R->n_timed;
    return CRT_OK;
}

}  // extern "C"
