// The body of the advance kernels (crt_paths.h), included once per kernel: `Q` is the launch's PathAdvanceParams and
// ADVANCE_BODY_N the number of input entries (see crt_trace_stream_body.inc).
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    AdvanceRows out[ADV_CHUNKS];
    bool keep[ADV_CHUNKS];
    uint32_t rank[ADV_CHUNKS], cnt[ADV_CHUNKS];              // the lane's place among its wave's appending lanes, their number
#pragma unroll
    for (int c = 0; c < ADV_CHUNKS; ++c) {
        const uint32_t i = (blockIdx.x * (uint32_t)ADV_CHUNKS + (uint32_t)c) * 256u + threadIdx.x;
        keep[c] = false;
        if (i < ADVANCE_BODY_N) keep[c] = advance_entry(Q, i, out[c]);
        const unsigned long long b = __builtin_amdgcn_ballot_w64(keep[c]);
        rank[c] = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        cnt[c] = (uint32_t)__builtin_popcountll(b);
    }
    if constexpr (ADV_PER_WAVE) {
        uint32_t base = 0;
        if (lane == 0 && cnt[0]) base = atomicAdd(Q.count, cnt[0]);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (keep[0]) advance_store(Q, base + rank[0], out[0]);
    } else {
        __shared__ uint32_t wave_cnt[ADV_CHUNKS * 4];        // appending lanes per (chunk, wave)
        __shared__ uint32_t group_base;
        if (lane == 0)
#pragma unroll
            for (int c = 0; c < ADV_CHUNKS; ++c) wave_cnt[c * 4 + (int)wave] = cnt[c];
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0;
            for (int k = 0; k < ADV_CHUNKS * 4; ++k) total += wave_cnt[k];
            group_base = total ? atomicAdd(Q.count, total) : 0u;
        }
        __syncthreads();
        uint32_t at = group_base;
#pragma unroll
        for (int c = 0; c < ADV_CHUNKS; ++c) {
            uint32_t before = 0, whole = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t k = wave_cnt[c * 4 + w];
                if ((uint32_t)w < wave) before += k;
                whole += k;
            }
            if (keep[c]) advance_store(Q, at + before + rank[c], out[c]);
            at += whole;
        }
    }
