// The body of the stream kernels (crt_trace.h), included once per kernel: `T` is the launch's TraceParams, TRACE_BODY_N
// the number of rays and TRACE_BODY_BLOCK the indices per reservation.  crt_trace_kernel takes both from T; the indirect
// kernel from the device count it read.  An include and not a function: as an inlined function the same text compiles to
// other code for crt_trace_kernel (DESIGN.md §18).
    const RenderParams& P = T.P;
    constexpr int SD = CRT_STACK6;           // LDS stack entries per lane at 6 one-wave workgroups per SIMD
    constexpr int TOPN = TOP_NODES;
    __shared__ WaveLdsWide L;
    __shared__ uint32_t stk[SD * 64];
    __shared__ __attribute__((aligned(16))) float sph_lds[32];   // the two per-ray spheres, as crt_render_kernel stages them
    __shared__ float4 top_lds[TOPN > 0 ? 8 * TOPN : 1];
    if (threadIdx.x < 32) {
        const int k = threadIdx.x & 15;
        const int src = k < 4 ? k : k < 9 ? k + 1 : k == 9 ? 10 : k == 10 ? 4 : -1;
        sph_lds[threadIdx.x] = src < 0 ? 0.f : P.sph2[threadIdx.x >> 4][src];
    }
    if (TOPN > 0 && threadIdx.x < 8u * TOPN) {
        const uint32_t m = threadIdx.x >> 3, k = threadIdx.x & 7;
        int n = 0;
        if (m > 0) {
            const float4 rm = node_row(P.nodes, node_base(0), 6);
            n = (int)(m - 1) < (__float_as_int(rm.y) & 0xff) ? __float_as_int(rm.x) + (int)(m - 1) : -1;
        }
        if (n >= 0 && n < P.n_nodes) top_lds[threadIdx.x] = node_row(P.nodes, node_base(n), k);
    }
    __syncthreads();
    const int lane = threadIdx.x;
    // the overflow stack region is indexed by grid lane, not by ray: (stack_cap - stack_lds) x grid lanes entries
    const size_t gl = (size_t)blockIdx.x * 64 + (size_t)lane, n_gl = (size_t)gridDim.x * 64;
    const float INF = __builtin_inff();
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t NONE = 0xffffffffu;
    TraceCounts cnt{};
    uint64_t n_rays = 0, n_active = 0;       // COUNT only
    // lane state: the ray, its traversal and its index; nothing else lives across the loop
    V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 1.f), inv = v3(0.f, 0.f, 0.f);
    float tmax = INF, closest = INF;
    uint32_t rows = 0, idx = NONE;
    int node = -1, sp = 0, hit = -1;
    // wave-uniform: first index of the reserved block, indices handed out.  Variant 7 reserves 64 pixels per
    // atomicAdd; a ray is ~4 node steps where a pixel is whole paths, and at 64 rays per atomicAdd the one counter's
    // address bounds the kernel (about 12 ns per atomic: 0.7 ms for 3.7 M rays whatever the grid, profiles/ray_query),
    // so the host sizes the block with the query (trace_enqueue)
    uint32_t pool = 0, used = TRACE_BODY_BLOCK;
    bool exhausted = false;
    L.owner_at[lane] = 0;
    for (;;) {
        const bool idle = idx != NONE && node < 0;             // holds a finished ray
        const int n_idle = __popcll(wave_ballot(idle));
        const int n_have = __popcll(wave_ballot(idx != NONE));
        if (n_idle >= T.refill_threshold || n_idle == n_have) {
            if (idle) {
                // the per-ray spheres against the traversal's closest hit, as finish_ray tests them (an occlusion
                // lane that retired on a hit within tmax is occluded whatever they add)
                if (!(ANY && hit >= 0 && closest <= tmax)) {
                    if (COUNT) cnt.spheres += P.n_ray_spheres;
                    ray_spheres<true>(P.prims, P.sphere_chain, P.n_chain, P.sphere_first, P.n_ray_spheres, o, d,
                                      sphere_inv(d, inv), closest, hit, sph_lds);
                }
                trace_store(T, idx, o, d, tmax, closest, hit);
                idx = NONE;
            }
            while (!exhausted) {                 // lanes without a ray take the next indices
                const uint64_t need = wave_ballot(idx == NONE);
                if (need == 0) break;
                if (used >= TRACE_BODY_BLOCK) {
                    uint32_t b = 0;
                    if (lane == 0) b = atomicAdd(T.next, TRACE_BODY_BLOCK);
                    pool = __builtin_amdgcn_readfirstlane(b);
                    used = 0;
                    if (pool >= TRACE_BODY_N) { exhausted = true; break; }
                }
                const uint32_t take = min((uint32_t)__popcll(need), TRACE_BODY_BLOCK - used);
                const uint32_t rank = (uint32_t)__popcll(need & below);
                if (idx == NONE && rank < take && pool + used + rank < TRACE_BODY_N) {
                    idx = pool + used + rank;
                    const float4 r0 = T.rays[2 * (size_t)idx], r1 = T.rays[2 * (size_t)idx + 1];
                    o = v3(r0.x, r0.y, r0.z);
                    tmax = r0.w;
                    d = v3(r1.x, r1.y, r1.z);
                    if (COUNT) ++n_rays;
                    node = 0;
                    sp = 0;
                    closest = INF;
                    hit = -1;
                    inv = box_inv(recip3_exact(d));   // the traversal's 1/d (wide_boxes)
                    rows = ray_rows(inv);
                    L.ray0[lane] = make_float4(o.x, o.y, o.z, d.x);
                    if (TOPN > 0) top_steps<COUNT, TOPN>(P, top_lds, o, inv, rows, node, sp, cnt, stk, gl, n_gl);
                }
                used += take;
            }
            if (!wave_ballot(idx != NONE)) break;     // the counter is past the end and every lane is done
        }
        if (COUNT) n_active += node >= 0;
        traverse_step4<COUNT>(P, o, d, inv, rows, node, sp, closest, hit, cnt, L, stk, lane, gl, n_gl);
        // occlusion: the closest t is no larger than any accepted t, so the first accepted hit within tmax decides;
        // the lane drops its stack and waits for the pass
        if (ANY && node >= 0 && hit >= 0 && closest <= tmax) {
            node = -1;
            sp = 0;
        }
    }
    if (COUNT) trace_add_stats(T, lane, n_rays, cnt, n_active);
