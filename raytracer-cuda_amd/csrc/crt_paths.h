// crt_paths.h — path steps over ray batches: camera rays and one bounce of material scattering, kernels + C ABI.
//
// Textually part of crt_hip.hip (included at its end, after crt_trace.h): the kernels call that file's and
// crt_device.h's device functions unchanged -- next_ray's camera block, the XORWOW draws, unit, reflect, refract,
// schlick_r0, cannot_refract_exact, recip_exact_wave, sky_unit, rand_in_unit_sphere -- so a batch step computes what the
// render kernels compute between two traces, bit for bit.  Nothing here is used by a render or trace kernel.
//
//   crt_camera_rays_kernel   one lane per pixel of the batch: next_ray() for a new sample on the pixel's RNG stream.
//   crt_path_step_kernel     one lane per path: shade_rec()'s body on the crt_hit record instead of the per-rank
//                            shading record (the normal, the face and the material index come from the record, the
//                            material's code and payload from the scene's per-material rows), then next_ray()'s
//                            bounce-limit test and Russian roulette for the bounce that follows.
//
// unit(), the reciprocal and the glass test pick their fast or IEEE sequence by a ballot over the lanes that run them;
// both sequences are correctly rounded, so the lanes a wave happens to hold (a partial last wave, entries that came in
// ended) change no bit of any lane's result.
#pragma once

struct CameraRaysParams {
    crt_camera_desc cam;
    int width, height;
    float rcp_w, rcp_h;
    int fast_uv;
    const int32_t* __restrict__ pixels;    // null: entry k is pixel k
    uint32_t n;
    uint32_t* __restrict__ rng;            // 6 words per pixel of the frame
    float4* __restrict__ rays;             // 2 rows per entry
    float4* __restrict__ paths;            // 2 rows per entry
};

__global__ __launch_bounds__(256) void crt_camera_rays_kernel(CameraRaysParams Q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= Q.n) return;
    const int pix = Q.pixels ? Q.pixels[i] : (int)i;
    const float INF = __builtin_inff();
    if ((uint32_t)pix >= (uint32_t)(Q.width * Q.height)) {   // not a pixel of the frame: nothing drawn, an ended path
        Q.rays[2 * (size_t)i] = make_float4(0.f, 0.f, 0.f, INF);
        Q.rays[2 * (size_t)i + 1] = make_float4(0.f, 0.f, 1.f, 0.f);
        Q.paths[2 * (size_t)i] = make_float4(0.f, 0.f, 0.f, __int_as_float(0));
        Q.paths[2 * (size_t)i + 1] = make_float4(__int_as_float(pix), __int_as_float(CRT_PATH_ENDED), 0.f, 0.f);
        return;
    }
    const crt_camera_desc& Cd = Q.cam;
    CamRegs C;
    C.pos = v3(Cd.origin[0], Cd.origin[1], Cd.origin[2]);
    C.llc = v3(Cd.lower_left[0], Cd.lower_left[1], Cd.lower_left[2]);
    C.hor = v3(Cd.horizontal[0], Cd.horizontal[1], Cd.horizontal[2]);
    C.ver = v3(Cd.vertical[0], Cd.vertical[1], Cd.vertical[2]);
    C.right = v3(Cd.right[0], Cd.right[1], Cd.right[2]);
    C.up = v3(Cd.up[0], Cd.up[1], Cd.up[2]);
    C.lens = Cd.lens_radius;
    C.fw = (float)Q.width;
    C.fh = (float)Q.height;
    C.rfw = Q.rcp_w;
    C.rfh = Q.rcp_h;
    C.fast_uv = Q.fast_uv;
    PathState S{};
    uint32_t* r = Q.rng + 6 * (size_t)pix;
    S.s = Rng{r[0], r[1], r[2], r[3], r[4], r[5]};
    S.pixel = v3(0.f, 0.f, 0.f);
    S.thr = v3(1.f, 1.f, 1.f);
    S.remaining = 1; S.bounce = 0; S.need_new = true; S.rays = 0; S.paths = 0;
    next_ray(S, C, pix % Q.width, pix / Q.width, 1);       // a new sample: the camera block alone
    r[0] = S.s.v0; r[1] = S.s.v1; r[2] = S.s.v2; r[3] = S.s.v3; r[4] = S.s.v4; r[5] = S.s.d;
    Q.rays[2 * (size_t)i] = make_float4(S.o.x, S.o.y, S.o.z, INF);
    Q.rays[2 * (size_t)i + 1] = make_float4(S.d.x, S.d.y, S.d.z, 0.f);
    Q.paths[2 * (size_t)i] = make_float4(1.f, 1.f, 1.f, __int_as_float(0));
    Q.paths[2 * (size_t)i + 1] = make_float4(__int_as_float(pix), __int_as_float(CRT_PATH_ACTIVE), 0.f, 0.f);
}

struct PathStepParams {
    float4* __restrict__ rays;             // 2 rows per entry, in place
    const float4* __restrict__ hits;       // 2 rows per entry
    float4* __restrict__ paths;            // 2 rows per entry, in place
    const float4* __restrict__ rows;       // per material: (code, 0, 0, 0) (payload)
    uint32_t* __restrict__ rng;            // 6 words per pixel
    float* __restrict__ linear;            // 3 floats per pixel
    uint32_t n, n_pix;
    int n_mats, max_bounces;
};

__global__ __launch_bounds__(256) void crt_path_step_kernel(PathStepParams Q) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= Q.n) return;
    const float4 p0 = Q.paths[2 * (size_t)i], p1 = Q.paths[2 * (size_t)i + 1];
    const uint32_t pix = __float_as_uint(p1.x);
    if (__float_as_int(p1.y) != CRT_PATH_ACTIVE || pix >= Q.n_pix) return;
    const float4 ray0 = Q.rays[2 * (size_t)i], ray1 = Q.rays[2 * (size_t)i + 1];
    const float4 h0 = Q.hits[2 * (size_t)i], h1 = Q.hits[2 * (size_t)i + 1];
    uint32_t* rp = Q.rng + 6 * (size_t)pix;
    Rng s{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5]};
    V3 o = v3(ray0.x, ray0.y, ray0.z), d = v3(ray1.x, ray1.y, ray1.z), thr = v3(p0.x, p0.y, p0.z);
    int bounce = __float_as_int(p0.w);
    const float INF = __builtin_inff();

    // ---- rayColor's loop body after the hit query: shade_rec() on the hit record
    constexpr uint32_t SHADE_MISS = 15;
    const float t = h0.x;
    const bool miss = t < 0;
    uint32_t code = SHADE_MISS;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!miss) {
        const uint32_t mat = __float_as_uint(h0.w);
        code = SHADE_INVALID;                                // CUDAKernels.h:127
        if (mat < (uint32_t)Q.n_mats) {
            code = __float_as_uint(Q.rows[2u * mat].x);
            m = Q.rows[2u * mat + 1u];
        }
    }
    const V3 hp = o + t * d;                                 // Ray::pointAtDistance
    const V3 outward = v3(h1.x, h1.y, h1.z);
    const bool front = __float_as_int(h1.w) != 0;            // HitInfo::setFaceNormal, as the query stored it
    const V3 n = front ? outward : -outward;
    bool ended = false;
    V3 add = v3(0.0f, 0.0f, 0.0f);                           // what an ending path adds to its pixel
    V3 q = d;                                                // dielectric, sky (CRTUtility.cuh:35)
    if (code == SHADE_LAMBERT || code == SHADE_METAL) q = rand_in_unit_sphere(s);
    V3 uq = q;
    if (code <= SHADE_DIELECTRIC || miss) uq = unit(q);      // one normalisation for all four users, as shade_rec
    if (miss) {                                              // :137-142
        add = thr * sky_unit(uq);
        ended = true;
    } else if (code == SHADE_INVALID) {                      // :127 invalid material: same ray again
        ++bounce;
    } else if (code == SHADE_LAMBERT) {                      // Material.cuh:66-77
        V3 sd = n + uq;
        if (fabsf(sd.x) < 1e-8f && fabsf(sd.y) < 1e-8f && fabsf(sd.z) < 1e-8f) sd = n;
        thr = thr * v3(m.x, m.y, m.z);
        o = hp;
        d = sd;
        ++bounce;
    } else if (code == SHADE_METAL) {                        // :89-96
        V3 refl = reflect(d, n);
        refl = unit(refl) + (m.w * uq);
        if (dot(refl, n) > 0) {
            thr = thr * v3(m.x, m.y, m.z);
            o = hp;
            d = refl;
            ++bounce;
        } else {                                             // absorbed: return Material::emit() = 0
            ended = true;
        }
    } else if (code == SHADE_DIELECTRIC) {                   // :109-128
        const float ri = front ? m.y : m.x;
        const float r0 = front ? m.z : m.w;
        const V3 ud = uq;
        const float cos_theta = fminf(dot(-ud, n), 1.0f);
        const bool cannot_refract = cannot_refract_exact(cos_theta, ri);
        V3 dir;
        if (cannot_refract || schlick_r0(cos_theta, r0) > uniform(s))
            dir = reflect(ud, n);
        else
            dir = refract(ud, n, ri);
        o = hp;
        d = dir;
        ++bounce;
    } else {                                                 // DiffuseLight: return emit() raw; unknown type: 0
        if (code == SHADE_LIGHT) add = v3(m.x, m.y, m.z);
        ended = true;
    }

    // ---- the next iteration's head (CUDAKernels.h:110-121), next_ray()'s first block
    if (!ended) {
        if (bounce >= Q.max_bounces) {                       // loop exhausted: final_color = 0
            ended = true;
        } else if (bounce >= 3) {
            float p = fmaxf(thr.x, fmaxf(thr.y, thr.z));
            p = fminf(p, 0.95f);
            if (uniform(s) > p) ended = true;
            else thr = recip_exact_wave(p) * thr;            // 1 / p, exact (crt_device.h)
        }
    }

    rp[0] = s.v0; rp[1] = s.v1; rp[2] = s.v2; rp[3] = s.v3; rp[4] = s.v4; rp[5] = s.d;
    if (ended) {
        float* L = Q.linear + 3 * (size_t)pix;
        const V3 sum = v3(L[0], L[1], L[2]) + add;           // pixel_color += ..., the (0, 0, 0) of a killed path too
        L[0] = sum.x; L[1] = sum.y; L[2] = sum.z;
    } else {
        Q.rays[2 * (size_t)i] = make_float4(o.x, o.y, o.z, INF);
        Q.rays[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, 0.f);
    }
    Q.paths[2 * (size_t)i] = make_float4(thr.x, thr.y, thr.z, __int_as_float(bounce));
    Q.paths[2 * (size_t)i + 1] = make_float4(p1.x, __int_as_float(ended ? CRT_PATH_ENDED : CRT_PATH_ACTIVE), p1.z, p1.w);
}

// ------------------------------------------------------------------ host side
namespace {

// The argument checks both device entries share; they come before any device use.
int path_batch_args(const char* what, int64_t n, const void* a, const void* b, const void* c) {
    if (n < 0 || n >= ((int64_t)1 << 31))
        return set_error(CRT_ERR_INVALID_ARGUMENT, std::string(what) + ": n must be in [0, 2^31)");
    if (n == 0) return CRT_OK;
    if (!a || !b || !c) return set_error(CRT_ERR_INVALID_ARGUMENT, std::string(what) + ": null array");
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u)
        return set_error(CRT_ERR_INVALID_ARGUMENT, std::string(what) + ": ray, hit and path arrays must be 16-byte aligned");
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_renderer_camera_rays_device(crt_renderer* R, const int32_t* d_pixels, int64_t n, uint32_t* d_rng,
                                    crt_ray* d_rays, crt_path* d_paths, void* stream) {
    if (!R) return set_error(CRT_ERR_INVALID_ARGUMENT, "camera rays: null renderer");
    if (int rc = path_batch_args("camera rays", n, d_rays, d_paths, d_rays)) return rc;
    if (n == 0) return CRT_OK;
    if (!R->has_camera) return set_error(CRT_ERR_INVALID_ARGUMENT, "camera rays: the renderer has no camera (crt_renderer_set_camera)");
    if (((uintptr_t)d_pixels | (uintptr_t)d_rng) & 3u)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "camera rays: pixel and RNG arrays must be 4-byte aligned");
    HIP_TRY(hipSetDevice(R->device));
    CameraRaysParams Q{};
    Q.cam = R->cam;
    Q.width = R->width; Q.height = R->height;
    Q.rcp_w = R->rcp_w; Q.rcp_h = R->rcp_h; Q.fast_uv = R->fast_uv;
    Q.pixels = d_pixels;
    Q.n = (uint32_t)n;
    Q.rng = d_rng ? d_rng : R->d_rng;
    Q.rays = reinterpret_cast<float4*>(d_rays);
    Q.paths = reinterpret_cast<float4*>(d_paths);
    hipLaunchKernelGGL(crt_camera_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

int crt_scene_path_step_device(const crt_scene* S, crt_ray* d_rays, const crt_hit* d_hits, crt_path* d_paths, int64_t n,
                               int max_bounces, uint32_t* d_rng, float* d_linear, int64_t n_pixels, void* stream) {
    if (!S) return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: null scene");
    if (int rc = path_batch_args("path step", n, d_rays, d_hits, d_paths)) return rc;
    if (max_bounces < 1) return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: max_bounces must be >= 1");
    if (n_pixels < 0 || n_pixels > ((int64_t)1 << 31) / 6)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: n_pixels must be in [0, 2^31 / 6]");
    if (n == 0) return CRT_OK;
    if (!d_rng || !d_linear) return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: null RNG state or sums");
    if (((uintptr_t)d_rng | (uintptr_t)d_linear) & 3u)
        return set_error(CRT_ERR_INVALID_ARGUMENT, "path step: RNG state and sums must be 4-byte aligned");
    HIP_TRY(hipSetDevice(S->device));
    PathStepParams Q{};
    Q.rays = reinterpret_cast<float4*>(d_rays);
    Q.hits = reinterpret_cast<const float4*>(d_hits);
    Q.paths = reinterpret_cast<float4*>(d_paths);
    Q.rows = S->d_mat_rows;
    Q.rng = d_rng;
    Q.linear = d_linear;
    Q.n = (uint32_t)n;
    Q.n_pix = (uint32_t)n_pixels;
    Q.n_mats = S->n_mats;
    Q.max_bounces = max_bounces;
    hipLaunchKernelGGL(crt_path_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Q);
    HIP_TRY(hipGetLastError());
    return CRT_OK;
}

int crt_scene_export_shade_rows(const crt_scene_desc* D, float* out, int64_t* n_materials) {
    if (!D || !n_materials) return set_error(CRT_ERR_INVALID_ARGUMENT, "null argument");
    if (D->n_materials < 0 || (D->n_materials > 0 && !D->materials)) return set_error(CRT_ERR_INVALID_ARGUMENT, "bad materials");
    *n_materials = D->n_materials;
    if (out) {
        const std::vector<float4> rows = material_shade_rows(D);
        if (!rows.empty()) std::memcpy(out, rows.data(), rows.size() * sizeof(float4));
    }
    return CRT_OK;
}

}  // extern "C"
