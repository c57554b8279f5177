// RayQuery.h — batch ray queries over a device scene (no reference counterpart: the reference traces only the rays
// its render kernel generates).  A header-only wrapper over the C ABI's crt_scene_trace / crt_scene_occluded; errors
// throw std::runtime_error through CRT_CHECK like the other wrappers.
//
//   CRT::RayQuery q(scene.getWorld());
//   std::vector<crt_hit> hits = q.trace(rays);          // closest hit over [0.001, inf), reported when t <= tmax
//   std::vector<uint8_t> shadowed = q.occluded(rays);   // 1 where trace() would report a hit
#pragma once
#include <cstdint>
#include <limits>
#include <vector>

#include "CUDAHelpers.h"
#include "crt_hip.h"

namespace CRT {

class RayQuery {
public:
    explicit RayQuery(const crt_scene* scene, crt_trace_options options = crt_trace_options{})
        : m_Scene(scene), m_Options(options) {}

    static crt_ray makeRay(const float o[3], const float d[3], float tmax = std::numeric_limits<float>::infinity()) {
        return crt_ray{{o[0], o[1], o[2]}, tmax, {d[0], d[1], d[2]}, 0.f};
    }

    std::vector<crt_hit> trace(const std::vector<crt_ray>& rays) const {
        std::vector<crt_hit> hits(rays.size());
        CRT_CHECK(crt_scene_trace(m_Scene, rays.data(), (int64_t)rays.size(), &m_Options, hits.data()));
        return hits;
    }
    std::vector<uint8_t> occluded(const std::vector<crt_ray>& rays) const {
        std::vector<uint8_t> out(rays.size());
        CRT_CHECK(crt_scene_occluded(m_Scene, rays.data(), (int64_t)rays.size(), &m_Options, out.data()));
        return out;
    }
    crt_trace_stats lastStats() const {
        crt_trace_stats s{};
        CRT_CHECK(crt_scene_trace_last_stats(m_Scene, &s));
        return s;
    }

    // One ray per pixel through the pixel centre, row 0 = the bottom row like the frames: Camera::getRay
    // (Camera.cuh:32-44) with u = (x + 0.5) / W, v = (y + 0.5) / H and lens offset 0.
    static std::vector<crt_ray> centreRays(const crt_camera_desc& c, int width, int height) {
        std::vector<crt_ray> rays((size_t)width * height);
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) {
                const float u = ((float)x + 0.5f) / (float)width, v = ((float)y + 0.5f) / (float)height;
                crt_ray& r = rays[(size_t)y * width + x];
                for (int a = 0; a < 3; ++a) {
                    r.origin[a] = c.origin[a];
                    r.dir[a] = ((c.lower_left[a] + u * c.horizontal[a]) + v * c.vertical[a]) - c.origin[a];
                }
                r.tmax = std::numeric_limits<float>::infinity();
                r.reserved = 0.f;
            }
        return rays;
    }

private:
    const crt_scene* m_Scene;
    crt_trace_options m_Options;
};

}  // namespace CRT
