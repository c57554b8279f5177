// crt_render — headless equivalent of the reference's EntryPoint.cu:14-42 + Raytracer.h:77-102:
// build the scene with SceneManager, set the camera, render one frame with CUDARenderer and
// write it as PNG or binary PPM by extension (rows flipped like WindowManager::drawFrame's flipVertically).
//
//   crt_render [-w W] [-h H] [-spp N] [-seed S] [-o out.ppm] [-pos x y z] [-fov deg] [-bvh reference|rebuilt]
//              [-leaf N] [-sbvh] [-aov depth|normal|object] [-adaptive TOL [-spp-min N]]
//              [-denoise SC:SN:SX [-denoise-iters N]] model.obj...
//   (-sbvh: rebuilt tree with spatial splits)
//
// -adaptive TOL: adaptive sampling (crt_renderer_render_adaptive): every pixel gets -spp-min samples (default 16, even),
// then only the 8x8 tiles whose error estimate exceeds TOL are refined, up to -spp samples; the JSON line gains samples,
// passes, tiles_at_max and mean_spp (samples per pixel of the frame).
//
// -denoise SC:SN:SX: the frame through the edge-avoiding a-trous filter (crt_renderer_compute_guides,
// crt_renderer_denoise, crt_renderer_resolve_denoised) with the colour, normal and position sigmas given (`inf` switches a
// term off; there are no defaults), -denoise-iters iterations (default 5).  With -adaptive the filter takes each tile's own
// scale.  The JSON line gains guides_ms and filter_ms.
//
// -aov: instead of a frame, one ray per pixel through the pixel centre (CRT::RayQuery::centreRays: Camera::getRay with
// u = (x + 0.5) / W, v = (y + 0.5) / H, lens offset 0) and an RGBA8 image of the closest hit, rows as for frames:
// depth = grey 1 / (1 + t); normal = 0.5 * n + 0.5; object = a fixed 8-colour palette by object & 7; a miss is black.
// A channel c in [0, 1] is stored as the byte (int)(255 * c + 0.5).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "crt/CUDARenderer.h"
#include "crt/Camera.h"
#include "crt/ImageIO.h"
#include "crt/RayQuery.h"
#include "crt/SceneManager.h"

// "SC:SN:SX" -> three sigmas; "inf" is +infinity.
static bool parseSigmas(const char* text, float out[3]) {
    const char* p = text;
    for (int k = 0; k < 3; ++k) {
        char* end = nullptr;
        out[k] = std::strtof(p, &end);
        if (end == p || *end != (k < 2 ? ':' : '\0')) return false;
        p = end + 1;
    }
    return true;
}

// The frame in the renderer's RGBA8 buffer becomes the denoised one; returns the stats.
static crt_denoise_stats denoiseFrame(crt_renderer* r, const crt_scene* scene, const float sigma[3], int iterations,
                                      bool tileScale, float scale) {
    const crt_denoise_options o{iterations, sigma[0], sigma[1], sigma[2], tileScale ? CRT_DENOISE_TILE_SCALE : 0u, 0};
    crt_denoise_stats s{};
    CRT_CHECK(crt_renderer_compute_guides(r, scene, nullptr, nullptr));
    CRT_CHECK(crt_renderer_denoise(r, &o, scale, &s, nullptr));
    CRT_CHECK(crt_renderer_resolve_denoised(r, nullptr));
    CRT_CHECK(crt_renderer_synchronize(r, nullptr));
    return s;
}

static uint8_t aovByte(float c) { return (uint8_t)(int)(255.0f * c + 0.5f); }

// The -aov image of `hits` (row 0 = the bottom row, like CUDARenderer's frames).
static std::vector<uint8_t> aovImage(const std::string& aov, const std::vector<crt_hit>& hits) {
    static const uint8_t palette[8][3] = {{230, 25, 75}, {60, 180, 75}, {255, 225, 25}, {0, 130, 200},
                                          {245, 130, 48}, {145, 30, 180}, {70, 240, 240}, {240, 50, 230}};
    std::vector<uint8_t> img(hits.size() * 4, 0);
    for (size_t i = 0; i < hits.size(); ++i) {
        const crt_hit& h = hits[i];
        uint8_t* px = img.data() + 4 * i;
        px[3] = 255;
        if (h.t < 0.f) continue;                                  // a miss: black
        if (aov == "depth") {
            px[0] = px[1] = px[2] = aovByte(1.0f / (1.0f + h.t));
        } else if (aov == "normal") {
            for (int c = 0; c < 3; ++c) px[c] = aovByte(0.5f * h.normal[c] + 0.5f);
        } else {
            for (int c = 0; c < 3; ++c) px[c] = palette[h.object & 7][c];
        }
    }
    return img;
}

int main(int argc, char** argv) {
    try {
        int W = 2560, spp = 1, sppMin = 16;
        bool adaptive = false;
        float tolerance = 0.f;
        bool denoise = false;
        float sigma[3] = {0.f, 0.f, 0.f};
        int denoiseIters = 5;
        int H = -1;
        unsigned long long seed = 41;
        float fov = 80.0f, aperture = 0.000001f;
        float pos[3] = {0.f, 0.f, 0.3f};
        std::string out = "frame.png";
        std::string aov;
        std::vector<std::string> files;
        crt_scene_options opts{};
        for (int i = 1; i < argc; ++i) {
            std::string a = argv[i];
            auto need = [&](int k) { if (i + k >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } };
            if (a == "-w") { need(1); W = std::atoi(argv[++i]); }
            else if (a == "-h") { need(1); H = std::atoi(argv[++i]); }
            else if (a == "-spp") { need(1); spp = std::atoi(argv[++i]); }
            else if (a == "-spp-min") { need(1); sppMin = std::atoi(argv[++i]); }
            else if (a == "-adaptive") { need(1); adaptive = true; tolerance = (float)std::atof(argv[++i]); }
            else if (a == "-denoise") {
                need(1);
                denoise = true;
                if (!parseSigmas(argv[++i], sigma)) {
                    std::fprintf(stderr, "-denoise takes SC:SN:SX (numbers or inf)\n");
                    return 2;
                }
            }
            else if (a == "-denoise-iters") { need(1); denoiseIters = std::atoi(argv[++i]); }
            else if (a == "-seed") { need(1); seed = std::strtoull(argv[++i], nullptr, 10); }
            else if (a == "-o") { need(1); out = argv[++i]; }
            else if (a == "-fov") { need(1); fov = (float)std::atof(argv[++i]); }
            else if (a == "-pos") { need(3); for (float& p : pos) p = (float)std::atof(argv[++i]); }
            else if (a == "-bvh") { need(1); std::string m = argv[++i]; opts.bvh = m == "rebuilt" ? CRT_BVH_REBUILT : CRT_BVH_REFERENCE; }
            else if (a == "-leaf") { need(1); opts.leaf_size = std::atoi(argv[++i]); }
            else if (a == "-sbvh") { opts.bvh = CRT_BVH_REBUILT; opts.spatial_splits = 1; }
            else if (a == "-aov") {
                need(1);
                aov = argv[++i];
                if (aov != "depth" && aov != "normal" && aov != "object") {
                    std::fprintf(stderr, "-aov takes depth, normal or object\n");
                    return 2;
                }
            }
            else files.push_back(a);
        }
        const float ASPECT_RATIO = 16.0f / 9.0f;                 // EntryPoint.cu:16-20
        if (H < 0) H = static_cast<int>(W / ASPECT_RATIO);
        if (files.empty()) files = {"assets/models/CornellBox-Original.obj", "assets/models/bunny.obj"};

        CRT::Camera camera(ASPECT_RATIO, fov, CRT::Vec3(pos[0], pos[1], pos[2]), CRT::Vec3(0, 0, 0), CRT::Vec3(0, 1, 0),
                           aperture, 0.3f);
        camera.setSamplesPerPixel(spp);
        auto config = CUDAHelpers::createRenderConfig(W, H);
        SceneManager scene(W, H);
        scene.setModelFiles(files);
        scene.setSceneOptions(opts);
        auto t0 = std::chrono::steady_clock::now();
        if (!aov.empty()) {                                       // a query needs the scene only: no renderer, no RNG state
            scene.initializeScene(config);
            auto t1 = std::chrono::steady_clock::now();
            const CRT::RayQuery query(scene.getWorld());
            const std::vector<crt_hit> hits = query.trace(CRT::RayQuery::centreRays(camera.toDesc(), W, H));
            auto t2 = std::chrono::steady_clock::now();
            const std::vector<uint8_t> img = aovImage(aov, hits);
            CRT::writeImage(out, img.data(), W, H, true);
            size_t n_hit = 0;
            for (const crt_hit& h : hits) n_hit += h.t >= 0.f;
            std::printf("{\"width\": %d, \"height\": %d, \"aov\": \"%s\", \"rays\": %zu, \"hits\": %zu, \"setup_s\": %.4f, "
                        "\"query_s\": %.4f, \"kernel_ms\": %.3f, \"out\": \"%s\"}\n",
                        W, H, aov.c_str(), hits.size(), n_hit, std::chrono::duration<double>(t1 - t0).count(),
                        std::chrono::duration<double>(t2 - t1).count(), query.lastStats().kernel_ms, out.c_str());
            return EXIT_SUCCESS;
        }
        CUDARenderer renderer(W, H);
        renderer.initialize(config, seed);
        scene.initializeScene(config, renderer.getRandState());
        auto t1 = std::chrono::steady_clock::now();
        renderer.updateCamera(camera);
        if (adaptive) {
            const crt_adaptive_options ao{sppMin, spp, tolerance, 0};
            crt_adaptive_stats as{};
            CRT_CHECK(crt_renderer_render_adaptive(renderer.handle(), scene.getBVHNodes(), &ao, 20, 0u, &as, nullptr));
            CRT_CHECK(crt_renderer_resolve_adaptive(renderer.handle(), nullptr));
            CRT_CHECK(crt_renderer_synchronize(renderer.handle(), nullptr));
            crt_denoise_stats ds{};
            if (denoise) ds = denoiseFrame(renderer.handle(), scene.getBVHNodes(), sigma, denoiseIters, true, 1.f);
            auto t2 = std::chrono::steady_clock::now();
            std::vector<uint8_t> img = renderer.readImage();
            CRT::writeImage(out, img.data(), W, H, true);
            std::printf("{\"width\": %d, \"height\": %d, \"spp\": %d, \"spp_min\": %d, \"tolerance\": %g, \"samples\": %llu, "
                        "\"passes\": %u, \"tiles_at_max\": %u, \"mean_spp\": %.4f, \"setup_s\": %.4f, \"frame_s\": %.4f, "
                        "\"adaptive_ms\": %.3f, ",
                        W, H, spp, sppMin, (double)tolerance, (unsigned long long)as.samples, as.passes, as.tiles_at_max,
                        (double)as.samples / ((double)W * H), std::chrono::duration<double>(t1 - t0).count(),
                        std::chrono::duration<double>(t2 - t1).count(), as.ms);
            if (denoise) std::printf("\"guides_ms\": %.3f, \"filter_ms\": %.3f, ", ds.guides_ms, ds.filter_ms);
            std::printf("\"out\": \"%s\"}\n", out.c_str());
            return EXIT_SUCCESS;
        }
        renderer.render(scene.getBVHNodes(), scene.getWorld());
        crt_denoise_stats ds{};
        if (denoise)
            ds = denoiseFrame(renderer.handle(), scene.getBVHNodes(), sigma, denoiseIters, false,
                              camera.toDesc().pixel_sample_scale);
        auto t2 = std::chrono::steady_clock::now();
        crt_work_counters c{};
        CRT_CHECK(crt_renderer_get_counters(renderer.handle(), &c));
        std::vector<uint8_t> img = renderer.readImage();
        CRT::writeImage(out, img.data(), W, H, true);   // flipVertically (WindowManager.h:88); .png or .ppm
        double setup = std::chrono::duration<double>(t1 - t0).count();
        double frame = std::chrono::duration<double>(t2 - t1).count();
        std::printf("{\"width\": %d, \"height\": %d, \"spp\": %d, \"rays\": %llu, \"setup_s\": %.4f, \"frame_s\": %.4f, "
                    "\"kernel_ms\": %.3f, \"mrays_per_s\": %.2f, ",
                    W, H, spp, (unsigned long long)c.rays, setup, frame, crt_renderer_last_kernel_ms(renderer.handle()),
                    c.rays / frame / 1e6);
        if (denoise) std::printf("\"guides_ms\": %.3f, \"filter_ms\": %.3f, ", ds.guides_ms, ds.filter_ms);
        std::printf("\"out\": \"%s\"}\n", out.c_str());
        return EXIT_SUCCESS;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
