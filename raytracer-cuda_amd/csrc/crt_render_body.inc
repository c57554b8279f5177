// The body of the render kernels (crt_hip.hip), included once per kernel: `P` is the launch's RenderParams; COUNT,
// VARIANT, MINW and FROZEN are compile-time constants of the including kernel.
// FROZEN (the plain variant-8 kernels): every LDS stack entry of this MINW in use, the LDS root step on, no spheres in
// the tree, the two per-ray spheres staged, one layout, no probe and no per-pixel ray counts, and the library's default
// wave_drain and regeneration threshold.  The facts are stated, not assigned: writing them into P makes the whole
// struct a stack object (536 B of scratch per lane).
    static_assert(!FROZEN || (VARIANT == 8 && !COUNT), "only the plain variant-8 kernels have a frozen twin");
    // Variant 8: the block's rank in the cost order, its samples and whether it continues stored sums: the launch's,
    // except with tail fill, where the block is the head or the tail part of a tile (fill_prologue).  First of all:
    // the tail part's acquire is a barrier to the compiler, and a value of P read before it is read again after it, so
    // stated ahead of it the frozen facts below would not reach the loop.  (The other kernels read P.spp, P.accumulate
    // and blockIdx.x where they did.)
    uint32_t rank = 0;
    int blk_spp = 0, blk_accumulate = 0;
    __shared__ FillNote fill_note;             // fill_prologue's note for fill_epilogue
    if constexpr (VARIANT == 8) {
        if (!fill_prologue(P, blockIdx.x, rank, blk_spp, blk_accumulate, &fill_note)) return;
    }
    if constexpr (FROZEN) {
        constexpr int FROZEN_STACK = wide_stack_entries(MINW);   // (a call inside the assumption makes the compiler drop it)
        __builtin_assume(P.stack_lds == FROZEN_STACK);
        __builtin_assume(P.top_levels == CRT_TOP_LEVELS);
        __builtin_assume(P.tree_spheres == 0);
        __builtin_assume(P.n_ray_spheres == 2);
        __builtin_assume(P.n_layouts == 1);
        __builtin_assume(P.probe_cost == nullptr);
        __builtin_assume(P.pix_rays == nullptr);
        __builtin_assume(P.wave_drain == WAVE_DRAIN);
        __builtin_assume(P.regen_threshold == REGEN_THRESHOLD_WIDE);
    }
#ifdef CRT_PROFILE_WAVE_TIMES
    const unsigned long long prof_t0 = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef CRT_PROFILE_PASS
    const uint64_t prof_life0 = shader_clock();
#endif
    constexpr int WGW = KernelShape<VARIANT>::waves;
    // variant 4: 16 LDS stack entries per lane at 5 waves/SIMD; 12 at 6+ so 6 workgroups fit the 160 KiB
    constexpr bool PERSIST = VARIANT == 7;
    constexpr bool TILED = VARIANT == 8;    // variant 4 with one wave per workgroup and a tile order
    constexpr bool TILES = TILED || VARIANT == 10;   // one 8x8 tile per one-wave workgroup (variant 10: variant 3's program)
    constexpr bool WIDE = VARIANT == 4 || PERSIST || TILED;
    using Lds = std::conditional_t<WIDE, WaveLdsWide, WaveLds>;
    __shared__ Lds lds[VARIANT >= 1 ? WGW : 1];
    constexpr int SD = WIDE ? wide_stack_entries(MINW) : 1;
    __shared__ uint32_t stack_lds[WIDE ? WGW * SD * 64 : 1];
    // the two per-ray spheres in 16-B rows, so every read is one ds_read_b128 at a fixed offset: per sphere
    // (center.xyz, radius^2) (box lo.xyz, box hi.x) (box hi.yz, rank, 0) (unused)
    __shared__ __attribute__((aligned(16))) float sph_lds[32];
    constexpr int TOPN = WIDE ? TOP_NODES : 0;
    // the two per-ray spheres' shading records (3 rows each), so a pass whose sphere test overrides the trace's hit
    // reads the record from LDS (the trace's own hit record is loaded at the pass start)
    __shared__ float4 shd_lds[WIDE ? 6 : 1];
    __shared__ float4 top_lds[TOPN > 0 ? 8 * TOPN : 1];   // CRT_TOP_LEVELS: root, then its internal children
    __shared__ uint32_t rays0_lds[PERSIST ? 64 * WGW : 1];   // variant 7: the lane's ray count when its pixel started
    if (WIDE) {
        if (threadIdx.x < 32) {
            const int k = threadIdx.x & 15;
            const int src = k < 4 ? k : k < 9 ? k + 1 : k == 9 ? 10 : k == 10 ? 4 : -1;
            sph_lds[threadIdx.x] = src < 0 ? 0.f : P.sph2[threadIdx.x >> 4][src];
        }
        if (threadIdx.x >= 32 && threadIdx.x < 38 && P.n_ray_spheres == 2) {
            const uint32_t q = threadIdx.x - 32, sp = q / 3;
            shd_lds[q] = P.shade[3u * (uint32_t)__float_as_int(P.sph2[sp][4]) + q % 3];
        }
        if (TOPN > 0 && threadIdx.x < 8u * TOPN) {
            const uint32_t m = threadIdx.x >> 3, k = threadIdx.x & 7;
            int n = 0;
            if (m > 0) {   // internal child m - 1 of the root (BFS emission: consecutive from first_child)
                const float4 rm = node_row(P.nodes, node_base(0), 6);
                n = (int)(m - 1) < (__float_as_int(rm.y) & 0xff) ? __float_as_int(rm.x) + (int)(m - 1) : -1;
            }
            if (n >= 0 && n < P.n_nodes) top_lds[threadIdx.x] = node_row(P.nodes, node_base(n), k);
        }
        __syncthreads();
    }
    // 16x16 pixel tile per workgroup, 8x8 per wave64.
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: LDS bases stay scalar
    int x, y;
    if (TILES) {                              // workgroup b renders 8x8 tile order[b]
        const uint32_t b = TILED ? rank : blockIdx.x;
        const uint32_t t = P.order ? P.order[b] : b;
        x = (int)(t % (uint32_t)P.tiles_x) * 8 + (lane & 7);
        y = (int)(t / (uint32_t)P.tiles_x) * 8 + (lane >> 3);
    } else {
        x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
        y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
        if (VARIANT == 4 && P.probe_cost) {   // a subsampled cost probe (crt_renderer_set_schedule's stride)
            x *= P.probe_stride;
            y *= P.probe_stride;
        }
    }
    const bool valid = x < P.width && y < P.height;
    const int pix = valid ? y * P.width + x : 0;

    PathState S;
    S.s = Rng{0, 0, 0, 0, 0, 0};
    S.pixel = v3(0.f, 0.f, 0.f);
    S.o = v3(0, 0, 0); S.d = v3(0, 0, 1); S.thr = v3(1, 1, 1);
    S.remaining = 0; S.bounce = 0; S.need_new = true; S.rays = 0; S.paths = 0;
#ifdef CRT_PROFILE_LOOPS
    S.k1 = S.k2 = S.kr = 0;
    unsigned long long lp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
#ifdef CRT_PROFILE_SITES
    S.site = 0;
    unsigned long long sites[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    if (valid && !PERSIST) {
        const uint32_t* r = P.rng + 6 * (size_t)pix;
        S.s = rng_load(r);
        if (TILED ? blk_accumulate : P.accumulate)
            S.pixel = v3(P.sum[3 * (size_t)pix], P.sum[3 * (size_t)pix + 1], P.sum[3 * (size_t)pix + 2]);
        S.remaining = TILED ? blk_spp : P.spp;
    }
    const CamRegs C = cam_regs(P.cam, P.width, P.height, P.rcp_w, P.rcp_h, P.fast_uv);
    TraceCounts cnt{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t wave_rays = 0;    // variant 8: rays of the wave (uniform); the other variants count per lane

    if constexpr (VARIANT == 0) {
        for (;;) {
            if (!next_ray(S, C, x, y, P.max_bounces)) break;
            ++S.rays;
            float t;
            const int hit = trace<COUNT>(P.nodes, P.prims, P.n_nodes, layout_base(S.d, P.n_layouts, P.n_nodes), S.o,
                                         S.d, t, cnt);
            shade(S, P, hit, t);
        }
    } else if constexpr (PERSIST) {
        // Variant 4's scheduling, but a lane whose pixel has no samples left stores it and takes the next
        // pixel slot from the global queue (8x8 tiles in `order`, most expensive first), so lanes never wait
        // for their wave's slowest pixel and waves never wait for their workgroup or the launch's last tiles.
        // Each pixel is still traced by ONE lane, samples in order, from its own RNG stream: same results.
        auto& L = lds[wave];
        uint32_t* stk = stack_lds + wave * SD * 64;
        const float INF = __builtin_inff();
        const size_t n_pix = (size_t)P.width * P.height;
        const uint32_t total_slots = (uint32_t)P.n_slots;
        const uint64_t below = (1ull << lane) - 1ull;
        bool live = false, has_result = false, have = false;
        int node = -1, sp = 0, hit = -1, px = 0, py = 0, ppix = 0;
        float closest = INF;
        V3 inv = v3(0.f, 0.f, 0.f);
        uint32_t rows = 0;         // ray_rows(inv)
        uint32_t pool = 0, used = 64;    // wave-uniform: first slot of the reserved block, slots handed out
        bool exhausted = false;
        L.owner_at[lane] = 0;
        for (;;) {
            const bool parked = live && node < 0;
            const int n_parked = __popcll(wave_ballot(parked));
            const int n_live = __popcll(wave_ballot(live));
            const uint64_t c0 = COUNT ? shader_clock() : 0;
            // once the queue is empty the wave only drains: its last paths no longer wait for many parked lanes
            // (crt_renderer_set_drain_threshold)
            const int regen_t = exhausted ? P.drain_threshold : P.regen_threshold;
            if (n_parked >= regen_t || n_parked == n_live) {
                if (COUNT) cnt.passes++;
                if (parked) {
                    if (has_result) finish_ray<COUNT>(S, P, inv, closest, hit, sph_lds, shd_lds, cnt, c0);
                    live = next_ray(S, C, px, py, P.max_bounces);
                    has_result = false;
                }
                if (have && !live) {     // the pixel's samples are done: store it (CUDAKernels.h:162-165)
                    uint32_t* r = P.rng + 6 * (size_t)ppix;
                    rng_store(r, S.s);
                    P.sum[3 * (size_t)ppix] = S.pixel.x;
                    P.sum[3 * (size_t)ppix + 1] = S.pixel.y;
                    P.sum[3 * (size_t)ppix + 2] = S.pixel.z;
                    if (P.pix_rays) P.pix_rays[ppix] = S.rays - rays0_lds[threadIdx.x];
                    have = false;
                }
                while (!exhausted) {                // lanes without a pixel take the next slots
                    const uint64_t need = wave_ballot(!have);
                    if (need == 0) break;
                    if (used >= 64u) {
                        uint32_t b = 0;
                        if (lane == 0) b = atomicAdd(P.queue, 64u);
                        pool = __builtin_amdgcn_readfirstlane(b);
                        used = 0;
                        if (pool >= total_slots) { exhausted = true; break; }
                    }
                    const uint32_t take = min((uint32_t)__popcll(need), 64u - used);
                    const uint32_t rank = (uint32_t)__popcll(need & below);
                    if (!have && rank < take && pool + used + rank < total_slots) {
                        const uint32_t pixel = P.order[pool + used + rank];
                        if (pixel != 0xffffffffu) {
                            ppix = (int)pixel;
                            px = ppix % P.width;
                            py = ppix / P.width;
                            const uint32_t* r = P.rng + 6 * (size_t)ppix;
                            S.s = rng_load(r);
                            S.pixel = P.accumulate ? v3(P.sum[3 * (size_t)ppix], P.sum[3 * (size_t)ppix + 1],
                                                        P.sum[3 * (size_t)ppix + 2])
                                                   : v3(0.f, 0.f, 0.f);
                            S.remaining = P.spp;
                            S.need_new = true;
                            have = true;
                            rays0_lds[threadIdx.x] = S.rays;
                            live = next_ray(S, C, px, py, P.max_bounces);
                            if (!live) {         // spp == 0: nothing to trace, store as is
                                uint32_t* w = P.rng + 6 * (size_t)ppix;
                                rng_store(w, S.s);
                                P.sum[3 * (size_t)ppix] = S.pixel.x;
                                P.sum[3 * (size_t)ppix + 1] = S.pixel.y;
                                P.sum[3 * (size_t)ppix + 2] = S.pixel.z;
                                if (P.pix_rays) P.pix_rays[ppix] = 0;
                                have = false;
                            }
                        }
                    }
                    used += take;
                }
                if (live && node < 0) {          // a new ray: the parked lanes' next ray or a new pixel's first
                    ++S.rays;
                    has_result = true;
                    node = 0;
                    sp = 0;
                    closest = INF;
                    hit = -1;
                    inv = recip3_exact(S.d);
                    inv = box_inv(inv);   // the traversal's 1/d (wide_boxes)
                    rows = ray_rows(inv);
                    if (COUNT) cnt.spheres += P.n_ray_spheres;
                    L.ray0[lane] = make_float4(S.o.x, S.o.y, S.o.z, S.d.x);
                    if (COUNT) cnt.trace_calls++;
                    if (TOPN > 0) top_steps<COUNT, TOPN>(P, top_lds, S.o, inv, rows, node, sp, cnt, stk, (size_t)ppix, n_pix);
                }
                if (!wave_ballot(live)) break;      // the queue is empty and every lane is done
            }
            if (COUNT) cnt.cyc_regen += shader_clock() - c0;
            traverse_step4<COUNT>(P, S.o, S.d, inv, rows, node, sp, closest, hit, cnt, L, stk, lane, (size_t)ppix, n_pix);
        }
    } else if constexpr (WIDE) {
        // Same scheduling as variant 3 over a 4-wide BVH: node < 0 = no node left (lane parked).
        auto& L = lds[wave];
        uint32_t* stk = stack_lds + wave * SD * 64;
        const float INF = __builtin_inff();
        const size_t n_pix = (size_t)P.width * P.height;
        // Lane masks instead of per-lane bools for the per-step tests: a ballot of a bool the compiler keeps as a lane
        // mask costs two VALU (widen, compare), a ballot of a compare none.  Every lane starts live (a pixel without
        // samples ends at the first pass); after a pass the live lanes are exactly those with a ray (has_result).
        uint64_t live_mask = wave_ballot(true);
        bool has_result = false;
        int node = -1, sp = 0, hit = -1;
        float closest = INF;
        V3 inv = v3(0.f, 0.f, 0.f);
        uint32_t rows = 0;         // ray_rows(inv)
        L.owner_at[lane] = 0;      // traverse_step4: owner + 1, 0 = none
        if (TILED && lane == 0) L.rays = 0;
        // variant 8: the most expensive tiles of the cost order bound the frame when it has few tiles per wave slot
        // (their pixels' sample chains are sequential); they regenerate sooner (DESIGN.md §5b, profiles/r02h)
        const int regen_t = (TILED && (int)rank < P.crit_tiles) ? P.crit_threshold : P.regen_threshold;
        bool first_pass = true;    // uniform
        // variant 8 at occupancy 4 (frames of few tiles per wave slot, bound by their most expensive tiles' sample
        // chains): the next node's rows load during the leaf round (traverse_step4<.., true>, profiles/r06r, r06s)
        constexpr bool PFV = TILED && MINW <= 4;
        float4 pf[PFV ? 7 : 1];
        int pf_node = -1;   // the node whose rows pf holds
#ifdef CRT_PROFILE_CRIT_TRACE
        uint32_t crit_iter = 0;
#endif
#ifdef CRT_PROFILE_LIVE
        uint64_t lh0 = 0, lh1 = 0, lh2 = 0, lh3 = 0, lh4 = 0, lh5 = 0, lh6 = 0, lh7 = 0, lh8 = 0;
        uint64_t lt_prev = shader_clock();
        int lb_prev = 8;
#endif
        constexpr bool TIME = COUNT || kProfilePass;
        // Phase priority (frozen twins; profiles/phase_priority): traversal is short bursts of arithmetic between
        // dependent loads, a pass is hundreds of VALU in a row behind one load, so a wave traverses at one s_setprio
        // level and runs its passes at another.  s_setprio ignores EXEC: every call sits in wave-uniform code.
        constexpr bool PRIO = FROZEN && MINW >= CRT_PRIO_MIN_W && CRT_PRIO_TRAVERSAL != CRT_PRIO_PASS;
        // Below CRT_PRIO_KEEP_BELOW waves per SIMD the waves that end the launch (critical tiles, and any wave once it
        // drains) keep the traversal level through their passes.  Both tests read regen_t, which the loop head holds:
        // a critical tile is one whose regen_t is not the frozen twin's constant threshold (a crit_threshold set equal
        // to it makes the tile ordinary).  Below CRT_PRIO_MIN_W the kernel has no s_setprio (crt_hip.hip).
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(CRT_PRIO_TRAVERSAL);
        for (;;) {
            const uint64_t h0 = kProfilePass ? shader_clock() : 0;
            const uint64_t parked_mask = live_mask & wave_ballot(node < 0);
            const int n_parked = __popcll(parked_mask);
            const int n_live = __popcll(live_mask);
#ifdef CRT_PROFILE_LIVE
            if (TILED) {
                const uint64_t lt = shader_clock(), dt = lt - lt_prev;
                lt_prev = lt;
                lh0 += lb_prev == 0 ? dt : 0; lh1 += lb_prev == 1 ? dt : 0; lh2 += lb_prev == 2 ? dt : 0;
                lh3 += lb_prev == 3 ? dt : 0; lh4 += lb_prev == 4 ? dt : 0; lh5 += lb_prev == 5 ? dt : 0;
                lh6 += lb_prev == 6 ? dt : 0; lh7 += lb_prev == 7 ? dt : 0; lh8 += lb_prev == 8 ? dt : 0;
                lb_prev = n_live >> 3;
                if (n_live == 0 && lane == 0) {
                    atomicAdd(&g_live_hist[0], lh0); atomicAdd(&g_live_hist[1], lh1); atomicAdd(&g_live_hist[2], lh2);
                    atomicAdd(&g_live_hist[3], lh3); atomicAdd(&g_live_hist[4], lh4); atomicAdd(&g_live_hist[5], lh5);
                    atomicAdd(&g_live_hist[6], lh6); atomicAdd(&g_live_hist[7], lh7); atomicAdd(&g_live_hist[8], lh8);
                }
            }
#endif
#ifdef CRT_PROFILE_CRIT_TRACE
            if (TILED && blockIdx.x == 0) {
                if ((crit_iter & 15u) == 0 && (crit_iter >> 4) < 16384u && lane == 0) {
                    g_crit_trace[2 * (crit_iter >> 4)] = __builtin_amdgcn_s_memrealtime();
                    g_crit_trace[2 * (crit_iter >> 4) + 1] = (unsigned long long)n_live | ((unsigned long long)n_parked << 8) |
                                                             ((unsigned long long)crit_iter << 16);
                }
                ++crit_iter;
            }
#endif
            if (n_live == 0) break;
            const uint64_t c0 = TIME ? shader_clock() : 0;
            if (kProfilePass) cnt.cyc_head += c0 - h0;
            // once fewer than regen_t lanes still have samples, waiting for every live lane to park before a pass makes
            // each of them wait for the slowest path of the others at every bounce; a pass at wave_drain/64 of them
            // (crt_renderer_set_wave_drain; 64 = all) shortens the wave's own drain (profiles/r04n)
            const bool drain_pass = n_live < regen_t && n_parked * 64 >= n_live * P.wave_drain;
            if (n_parked >= regen_t || n_parked == n_live || drain_pass) {
                if constexpr (PRIO) {
                    bool keep = false;
                    if constexpr (MINW < CRT_PRIO_KEEP_BELOW) {
                        // (an opaque copy: with regen_t itself the compiler hoists the tests out of the loop as lane
                        // masks, four scalar registers that <false, 8, 7> does not have: 2 SGPR spills, 1 VGPR spill)
                        int rt = regen_t;
                        asm volatile("" : "+s"(rt));
                        keep = rt != REGEN_THRESHOLD_WIDE || n_live < rt;
                    }
                    if (!keep) __builtin_amdgcn_s_setprio(CRT_PRIO_PASS);
                }
                if (COUNT || kProfilePass) cnt.passes++;
#ifdef CRT_PROFILE_LOOPS
                uint32_t pk1 = 0, pk2 = 0, pkr = 0;
#endif
                if (__builtin_amdgcn_inverse_ballot_w64(parked_mask)) {
                    const uint64_t s0 = TIME ? shader_clock() : 0;
                    // (loading the shading record before this sphere test, to overlap its latency, measured +0.7 %:
                    // profiles/r01ar)
                    // after the first pass every parked lane holds a result (parked_mask is within live_mask, which is
                    // the lanes with a ray): a uniform test instead of a divergent branch on has_result (-0.38 %,
                    // profiles/r02av)
                    if (!first_pass) {
                        finish_ray<COUNT>(S, P, inv, closest, hit, sph_lds, shd_lds, cnt, s0);
                    }
                    const uint64_t s1 = TIME ? shader_clock() : 0;
                    const bool live = next_ray(S, C, x, y, P.max_bounces);
                    if (TIME) {
                        const uint64_t s2 = shader_clock();
                        cnt.cyc_shade += s1 - s0;
                        cnt.cyc_next += s2 - s1;
                    }
#ifdef CRT_PROFILE_LOOPS
                    pk1 = S.k1; pk2 = S.k2; pkr = S.kr;
                    S.k1 = S.k2 = S.kr = 0;
#endif
                    has_result = false;
                    if (live) {
                        if (!TILED) ++S.rays;
                        has_result = true;
                        node = 0;
                        sp = 0;
                        closest = INF;
                        hit = -1;
                        // exact 1/d: the per-ray spheres' reference box tests need it (the padded traversal
                        // would do with rcp)
                        inv = recip3_exact(S.d);
                        inv = box_inv(inv);   // the traversal's 1/d (wide_boxes)
                        rows = ray_rows(inv);
                        if (COUNT) cnt.spheres += P.n_ray_spheres;
                        L.ray0[lane] = make_float4(S.o.x, S.o.y, S.o.z, S.d.x);
                        if (COUNT) cnt.trace_calls++;
                        const uint64_t s3 = kProfilePass ? shader_clock() : 0;
                        if (TOPN > 0) top_steps<COUNT, TOPN, FROZEN>(P, top_lds, S.o, inv, rows, node, sp, cnt, stk, (size_t)pix, n_pix);
                        if (kProfilePass) {
                            const uint64_t s4 = shader_clock();
                            cnt.cyc_top += s4 - s3;
                            cnt.cyc_setup += s3 - s1;   // next_ray and the set-up; next_ray's share is subtracted below
                        }
                    }
                }
#ifdef CRT_PROFILE_LOOPS
                {
                    uint32_t m1 = pk1, m2 = pk2, m12 = pk1 + pk2, m1r2 = pk1 + pkr + pk2, s1 = pk1, s2 = pk2;
                    for (int off = 32; off > 0; off >>= 1) {
                        m1 = max(m1, (uint32_t)__shfl_xor((int)m1, off));
                        m2 = max(m2, (uint32_t)__shfl_xor((int)m2, off));
                        m12 = max(m12, (uint32_t)__shfl_xor((int)m12, off));
                        m1r2 = max(m1r2, (uint32_t)__shfl_xor((int)m1r2, off));
                        s1 += (uint32_t)__shfl_xor((int)s1, off);
                        s2 += (uint32_t)__shfl_xor((int)s2, off);
                    }
                    lp[0] += 1; lp[1] += m1; lp[2] += m2; lp[3] += m12; lp[4] += m1r2; lp[5] += s1; lp[6] += s2;
                    lp[7] += (unsigned long long)n_parked;
                }
#endif
#ifdef CRT_PROFILE_SITES
                {
                    const uint32_t st = S.site;   // only this pass's parked lanes have marks
                    S.site = 0;
                    const bool entry = wave_ballot(st & SITE_CAM_ENTRY) != 0, killed = wave_ballot(st & SITE_CAM_KILLED) != 0;
                    const bool ruv = wave_ballot(st & SITE_UNIT_RUV) != 0, glass = wave_ballot(st & SITE_UNIT_GLASS) != 0;
                    const bool sky = wave_ballot(st & SITE_UNIT_SKY) != 0, refl = wave_ballot(st & SITE_UNIT_REFL) != 0;
                    sites[0] += 1; sites[1] += entry; sites[2] += killed; sites[3] += entry && killed;
                    sites[4] += ruv; sites[5] += glass; sites[6] += sky; sites[7] += refl;
                    sites[8] += ruv || glass || sky; sites[9] += (int)ruv + (int)glass + (int)sky;
                    sites[10] += (unsigned long long)n_parked;
                    sites[11] += (unsigned long long)__popcll(wave_ballot(st & (SITE_CAM_ENTRY | SITE_CAM_KILLED)));
                }
#endif
                live_mask = wave_ballot(has_result);
                if constexpr (kProfilePass) {
                    // the pass's section timers ran in divergent code, so each lane's accumulators hold only the passes
                    // it took part in (lane 0 alone was reported before): every lane adopts the accumulators of a lane
                    // that ran this pass's innermost timed section, which keeps them wave-uniform
                    const uint64_t ran = parked_mask & live_mask;
                    const int src = __builtin_ctzll(ran ? ran : parked_mask);
                    cnt.cyc_shade = bcast64(cnt.cyc_shade, src);
                    cnt.cyc_sph = bcast64(cnt.cyc_sph, src);
                    cnt.cyc_next = bcast64(cnt.cyc_next, src);
                    cnt.cyc_setup = bcast64(cnt.cyc_setup, src);
                    cnt.cyc_top = bcast64(cnt.cyc_top, src);
                }
                first_pass = false;
                // variant 8 counts the wave's rays in LDS (one VGPR less in the hot loop); (an LDS add without return
                // instead of the read-modify-write measured +0.4 % on config C, profiles/r05e)
                if (TILED && lane == 0) L.rays += (uint32_t)__popcll(parked_mask & live_mask);
                if constexpr (PRIO) __builtin_amdgcn_s_setprio(CRT_PRIO_TRAVERSAL);
            }
            if (TIME) cnt.cyc_regen += shader_clock() - c0;
            if constexpr (PFV) {
                traverse_step4<COUNT, true, FROZEN>(P, S.o, S.d, inv, rows, node, sp, closest, hit, cnt, L, stk, lane, (size_t)pix,
                                            n_pix, pf, &pf_node);
            } else
            traverse_step4<COUNT, false, FROZEN>(P, S.o, S.d, inv, rows, node, sp, closest, hit, cnt, L, stk, lane, (size_t)pix, n_pix);
        }
    } else if constexpr (VARIANT == 2 || VARIANT == 3 || VARIANT == 10) {
        constexpr bool PF = VARIANT == 3 || VARIANT == 10;
        float4 pA = make_float4(0.f, 0.f, 0.f, 0.f), pB = pA;
        // One wave iteration = one traversal step.  A lane whose trace ends parks until at least
        // `regen_threshold` lanes (or every live lane) are parked; the parked lanes then shade, start
        // their next ray and rejoin traversal while the others keep stepping.
        auto& L = lds[wave];
        const float INF = __builtin_inff();
        bool live = true, has_result = false;
        int node = P.n_nodes, hit = -1, nbase = 0;
        float closest = INF;
        V3 inv = v3(0.f, 0.f, 0.f);
        L.owner_at[lane] = 0;      // owner + 1, 0 = none
        for (;;) {
            const bool parked = live && node >= P.n_nodes;
            const int n_parked = __popcll(wave_ballot(parked));
            const int n_live = __popcll(wave_ballot(live));
            if (n_live == 0) break;
            if (n_parked >= P.regen_threshold || n_parked == n_live) {
                if (parked) {
                    if (has_result) shade(S, P, hit, closest);
                    live = next_ray(S, C, x, y, P.max_bounces);
                    has_result = false;
                    if (live) {
                        ++S.rays;
                        has_result = true;
                        node = 0;
                        closest = INF;
                        hit = -1;
                        inv = v3(1.0f / S.d.x, 1.0f / S.d.y, 1.0f / S.d.z);
                        nbase = layout_base(S.d, P.n_layouts, P.n_nodes);
                        L.ray0[lane] = make_float4(S.o.x, S.o.y, S.o.z, S.d.x);
                        if (PF) {
                            pA = P.nodes[nbase];
                            pB = P.nodes[nbase + 1];
                        }
                        if (COUNT) cnt.trace_calls++;
                    }
                }
            }
            traverse_step<COUNT, PF>(P.nodes, P.prims, P.n_nodes, nbase, P.n_prims, P.err, S.o, S.d, inv, node,
                                     closest, hit, cnt, L, lane, pA, pB);
        }
    } else {
        bool live = true;
        for (;;) {
            if (live) live = next_ray(S, C, x, y, P.max_bounces);
            if (!wave_ballot(live)) break;
            float t;
            const int hit = trace_coop<COUNT>(P.nodes, P.prims, P.n_nodes, layout_base(S.d, P.n_layouts, P.n_nodes),
                                              P.n_prims, P.err, S.o, S.d, live, t, cnt, lds[wave], lane);
            if (live) {
                ++S.rays;
                shade(S, P, hit, t);
            }
        }
    }

    if (((WIDE && !PERSIST) || VARIANT == 3) && P.probe_cost) {   // probe launch: work of this pixel; no state is written
        // counting probe: a ray's shading + generation costs about as much as 16 child-box tests, a triangle
        // test about 4 (section profile, profiles/r01h); plain probe: rays
        if (valid) P.probe_cost[pix] = COUNT ? (16u * S.rays + cnt.boxes + 4u * cnt.tris) >> 3 : S.rays;
        return;
    }
    if (valid && !PERSIST) {
        uint32_t* r = P.rng + 6 * (size_t)pix;
        rng_store(r, S.s);
        P.sum[3 * (size_t)pix] = S.pixel.x;
        P.sum[3 * (size_t)pix + 1] = S.pixel.y;
        P.sum[3 * (size_t)pix + 2] = S.pixel.z;
    }
    if constexpr (TILED) fill_epilogue(&fill_note, lane);
    if constexpr (TILED) wave_rays = lds[0].rays;
    const uint64_t wr = TILED ? (uint64_t)wave_rays : wave_sum_u64(S.rays);
    if (COUNT) {
        const uint64_t wb = wave_sum_u64(cnt.boxes), wt = wave_sum_u64(cnt.tris);
        const uint64_t ws = wave_sum_u64(cnt.spheres), wp = wave_sum_u64(S.paths);
        if (lane == 0) {
            atomicAdd(&P.counters[1], (unsigned long long)wb);
            atomicAdd(&P.counters[2], (unsigned long long)wt);
            atomicAdd(&P.counters[3], (unsigned long long)ws);
            atomicAdd(&P.counters[4], (unsigned long long)wp);
            // scheduling diagnostics (variant 1): lane-slots offered by traversal steps / leaf rounds,
            // and wave-level trace calls (all uniform per wave)
            atomicAdd(&P.counters[5], 64ull * cnt.step_slots);
            atomicAdd(&P.counters[6], 64ull * cnt.round_slots + ((unsigned long long)cnt.trace_calls << 40));
            atomicAdd(&P.counters[8], (unsigned long long)cnt.cyc_regen);
            atomicAdd(&P.counters[9], (unsigned long long)cnt.cyc_step);
            atomicAdd(&P.counters[10], (unsigned long long)cnt.cyc_round);
            atomicAdd(&P.counters[11], (unsigned long long)cnt.passes);
            atomicAdd(&P.counters[12], 1ull);
            atomicAdd(&P.counters[13], (unsigned long long)cnt.cyc_shade);
            atomicAdd(&P.counters[14], (unsigned long long)cnt.cyc_next);
            atomicAdd(&P.counters[7], (unsigned long long)cnt.cyc_sph);
        }
    }
    if (lane == 0) atomicAdd(&P.counters[0], (unsigned long long)wr);
#ifdef CRT_PROFILE_PASS
    if (!COUNT && TILED && lane == 0 && (int)blockIdx.x < CRT_PROFILE_PASS_FIRST) {
        const unsigned long long v[17] = {cnt.cyc_step, cnt.cyc_round, cnt.cyc_regen, cnt.cyc_shade, cnt.cyc_sph,
                                          cnt.cyc_next, cnt.cyc_setup, cnt.cyc_top, cnt.cyc_head, cnt.passes, 1ull,
                                          shader_clock() - prof_life0, cnt.step_slots, cnt.round_slots, wave_rays,
#ifdef CRT_PROFILE_ROWS
                                          cnt.cyc_rows, cnt.cyc_prims
#else
                                          0ull, 0ull
#endif
        };
        for (int k = 0; k < 17; ++k) atomicAdd(&g_pass_prof[k], v[k]);
    }
#endif
#ifdef CRT_PROFILE_LOOPS
    if (lane == 0 && !P.probe_cost)
        for (int k = 0; k < 8; ++k) atomicAdd(&g_loop_prof[k], lp[k]);
#endif
#ifdef CRT_PROFILE_SITES
    if (lane == 0 && !P.probe_cost)
        for (int k = 0; k < 12; ++k) atomicAdd(&g_site_prof[k], sites[k]);
#endif
#ifdef CRT_PROFILE_WAVE_TIMES
    {
        const unsigned wid = (blockIdx.y * gridDim.x + blockIdx.x) * (unsigned)WGW + (threadIdx.x >> 6);
        if (lane == 0 && wid < 4u * 65536u) {
            g_wave_prof[2 * wid] = prof_t0;
            g_wave_prof[2 * wid + 1] = __builtin_amdgcn_s_memrealtime();
#ifdef CRT_PROFILE_CRIT_TRACE
            g_wave_hw[2 * wid] = __builtin_amdgcn_s_getreg(4 | (31 << 11));        // HW_REG_HW_ID
            g_wave_hw[2 * wid + 1] = __builtin_amdgcn_s_getreg(20 | (3 << 11));    // HW_REG_XCC_ID [3:0]
#endif
        }
    }
#endif
