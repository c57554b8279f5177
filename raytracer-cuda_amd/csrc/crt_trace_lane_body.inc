// The body of the lane kernels (crt_trace.h), included once per kernel: `T` is the launch's TraceParams and TRACE_BODY_N
// the number of rays (see crt_trace_stream_body.inc).
    const RenderParams& P = T.P;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    TraceCounts cnt{};
    if (i < TRACE_BODY_N) {
        const float4 r0 = T.rays[2 * (size_t)i], r1 = T.rays[2 * (size_t)i + 1];
        const V3 o = v3(r0.x, r0.y, r0.z), d = v3(r1.x, r1.y, r1.z);
        float t;
        const int hit = T.width == 4 ? trace4(P.nodes, P.prims, P.sphere_chain, P.n_chain, P.sphere_first,
                                              P.n_ray_spheres, o, d, t)
                                     : trace<COUNT>(P.nodes, P.prims, P.n_nodes,
                                                    layout_base(d, P.n_layouts, P.n_nodes), o, d, t, cnt);
        trace_store(T, i, o, d, r0.w, t, hit);
    }
    if (COUNT) trace_add_stats(T, threadIdx.x & 63, i < TRACE_BODY_N ? 1u : 0u, cnt, 0);
