/*
 * crt_hip.h — C ABI of the MI355X (gfx950) render layer: libcrt_hip.so.
 *
 * This is the drop-in boundary for the reference's device path
 * (Mordentary/RayTracer-Cuda, paths relative to CudaRayTracer/src/):
 *
 *   reference                                            replaced by
 *   ---------------------------------------------------  ------------------------------------
 *   CUDARenderer::initialize  (CUDARenderer.cuh:39-49)   crt_renderer_create + crt_renderer_init_rand
 *     initRandState<<<>>>     (CUDAKernels.h:18-26)      crt_renderer_init_rand
 *   CUDARenderer::updateCamera (CUDARenderer.cuh:51-53)  crt_renderer_set_camera
 *     cudaMemcpyToSymbol(d_camera) (Camera.cuh:213)
 *   CUDARenderer::render      (CUDARenderer.cuh:55-60)   crt_renderer_render + crt_renderer_resolve
 *     render<<<>>> / rayColor (CUDAKernels.h:102-166)    (crt_renderer_render_frame does both)
 *   CUDARenderer::getImageData (CUDARenderer.cuh:16)     crt_renderer_rgba_device_ptr / _read_rgba8
 *   CUDARenderer::getRandState (CUDARenderer.cuh:17)     crt_renderer_rng_device_ptr
 *   SceneManager::initializeScene device half           crt_scene_create (flat arrays; the host
 *     createRandomWorld / initMesh / createBVH <<<1,1>>>   builds the BVHs with the reference's
 *     (CUDAKernels.h:28-100, SceneManager.h:77-98)         semantics, see crt_host.h)
 *   SceneManager::getBVHNodes / getWorld (SceneManager.h:25-26)  the crt_scene handle
 *   CUDA_CHECK -> throw (CUDAHelpers.h:19-26)            int status + crt_last_error()
 *
 * Plain C: pointers and sizes only.  All device memory is owned by the opaque
 * handles; the caller owns every host buffer.  Handles are not thread-safe; use
 * one renderer per device (one process per GPU for multi-GPU).
 */
#ifndef CRT_HIP_H
#define CRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRT_ABI_VERSION 3

enum crt_status {
    CRT_OK = 0,
    CRT_ERR_INVALID_ARGUMENT = -1,
    CRT_ERR_HIP = -2,          /* a HIP runtime call failed; see crt_last_error() */
    CRT_ERR_OUT_OF_MEMORY = -3,
    CRT_ERR_NO_DEVICE = -4,
    CRT_ERR_UNSUPPORTED = -5
};

/* Material.cuh:8-14 MaterialType */
enum crt_material_type { CRT_LAMBERTIAN = 0, CRT_METAL = 1, CRT_DIELECTRIC = 2, CRT_DIFFUSE_LIGHT = 3 };

/* Material.cuh:16-47 MaterialData (roughness is clamped to <= 1 like the Metal ctor, Material.cuh:86). */
typedef struct crt_material_desc {
    int32_t type;
    float albedo[3];
    float emission[3];
    float roughness;
    float ior;
} crt_material_desc;

/* One reference BVHNode (BVHNode.cuh:158-165 fields): box + children / leaf range. */
typedef struct crt_bvh_node_desc {
    float bmin[3];
    float bmax[3];
    int32_t left, right;          /* internal nodes */
    int32_t obj_index, obj_count; /* leaves: mesh = index range [obj_index, obj_index+obj_count) step 3;
                                     scene = object index */
    int32_t is_leaf;
} crt_bvh_node_desc;

/* One Mesh (Mesh.cuh:18-53 ctor arguments + its built BVH). */
typedef struct crt_mesh_desc {
    uint32_t vertex_offset, vertex_count;
    uint32_t index_offset, index_count;
    uint32_t face_offset;          /* into face_materials */
    uint32_t material_id_offset;   /* Mesh::m_MatIDOffset */
    const crt_bvh_node_desc* nodes;/* Mesh::m_MeshBVH in builder index order (root = 0) */
    int32_t node_count;
    float aabb[6];                 /* Mesh::m_BoundingBox  min xyz, max xyz */
} crt_mesh_desc;

/* Sphere.cuh:20-25 */
typedef struct crt_sphere_desc {
    float center[3];
    float radius;
    int32_t material;
} crt_sphere_desc;

enum crt_object_kind { CRT_OBJECT_MESH = 0, CRT_OBJECT_SPHERE = 1 };
typedef struct crt_object_desc {   /* HittableList::m_Objects entry (HittableList.cuh:73) */
    int32_t kind;
    int32_t index;                 /* into meshes[] or spheres[] */
} crt_object_desc;

typedef struct crt_scene_desc {
    const float* positions;        /* vertex slots, xyz per slot (Vertex::Position, Mesh.cuh:5-10) */
    uint64_t n_positions;
    const uint32_t* indices;       /* per-mesh local vertex indices, AFTER the mesh BVH build permuted them */
    uint64_t n_indices;
    const int32_t* face_materials; /* per triangle, permuted with the indices */
    uint64_t n_faces;
    const crt_mesh_desc* meshes;
    int32_t n_meshes;
    const crt_sphere_desc* spheres;
    int32_t n_spheres;
    const crt_object_desc* objects;   /* HittableList order (CUDAKernels.h:64-73) */
    int32_t n_objects;
    const crt_bvh_node_desc* scene_nodes;  /* BVHNode::buildBVHScene output, root = 0 */
    int32_t n_scene_nodes;
    const crt_material_desc* materials;    /* HittableList::m_Materials order */
    int32_t n_materials;
} crt_scene_desc;

/* Camera POD as the kernel needs it (Camera.cuh:32-44 reads exactly these). */
typedef struct crt_camera_desc {
    float origin[3];       /* m_Position */
    float lower_left[3];   /* m_LowerLeftCorner */
    float horizontal[3];   /* m_Horizontal */
    float vertical[3];     /* m_Vertical */
    float right[3];        /* m_Right */
    float up[3];           /* m_Up */
    float lens_radius;     /* m_LensRadius */
    int32_t samples_per_pixel;   /* m_SamplesPerPixel */
    float pixel_sample_scale;    /* m_PixelSampleScale = 1.f / spp */
} crt_camera_desc;

typedef struct crt_scene_stats {
    int64_t device_nodes;      /* flattened (threaded, DFS-preorder) nodes incl. scene level */
    int64_t device_prims;      /* triangles + spheres */
    int64_t device_bytes;      /* node + prim + material bytes resident in HBM */
    int32_t max_depth;         /* deepest node (scene + mesh levels) */
    int32_t n_materials;
    int32_t bvh;               /* CRT_BVH_REFERENCE | CRT_BVH_REBUILT */
    int32_t layouts;           /* threaded node orders resident (device_nodes counts all of them) */
    int64_t excluded_prims;    /* REBUILT: triangles the reference can never hit (zero-thickness boxes) */
    int32_t width;             /* 2 (threaded binary nodes) or 4 (4-wide nodes) */
    int32_t stack_bound;       /* width 4: traversal-stack entries a ray can need */
    int64_t spatial_splits;    /* REBUILT with spatial_splits: nodes cut by a plane (SBVH) */
    int64_t references;        /* REBUILT: primitive references in the tree's leaves (> primitives with spatial splits) */
} crt_scene_stats;

typedef struct crt_work_counters {  /* filled by a CRT_RENDER_COUNT_WORK render */
    uint64_t rays;           /* closest-hit queries = calls of the scene-level hit (CUDAKernels.h:123) */
    uint64_t box_tests;      /* AABB::hit calls (scene + mesh levels) */
    uint64_t tri_tests;      /* rayTriangleIntersect calls */
    uint64_t sphere_tests;   /* Sphere::hit calls */
    uint64_t paths;          /* samples completed */
} crt_work_counters;

/* render flags */
#define CRT_RENDER_ACCUMULATE  1u   /* add into the existing linear sum instead of starting from 0 */
#define CRT_RENDER_COUNT_WORK  2u   /* counting kernel variant: fills crt_work_counters (slower) */

typedef struct crt_scene crt_scene;
typedef struct crt_renderer crt_renderer;

int crt_abi_version(void);
/* How this library was compiled: CRT_BUILD_CHECKED = the checked build (-DCRT_CHECKED, lib/checked/libcrt_hip.so):
 * the leaf rounds re-check every (owner, primitive) pair and report a bad one through crt_renderer_synchronize
 * instead of loading outside the primitive array.  Same frames, slower. */
#define CRT_BUILD_CHECKED 1
int crt_build_flags(void);
const char* crt_last_error(void);   /* thread-local message of the last failing call */
int crt_device_count(int* out);

/* Acceleration structure the device scene is traversed with.
 *   CRT_BVH_REFERENCE — the reference's own scene + mesh BVHs, flattened unchanged (default).  Bit-exact:
 *     same boxes, same visiting order, same culling, same work counters as BVHNode::hit / Mesh::hit.
 *   CRT_BVH_REBUILT   — a binned-SAH BVH over the same primitives with small padded leaves, collapsed to
 *     4-wide nodes (default; width 2 = threaded binary layouts).  Same hit rule as the
 *     reference: closest t in [0.001, closest], ties to the primitive the reference visits LAST
 *     (every primitive carries its reference DFS rank), primitives the reference can never reach
 *     (inside a zero-thickness box) excluded.  Results differ from the reference only where the
 *     reference's unpadded boxes round away a genuine hit; see DESIGN.md §4b for the measured rate. */
#define CRT_BVH_REFERENCE 0
#define CRT_BVH_REBUILT   1

typedef struct crt_scene_options {
    int32_t bvh;              /* CRT_BVH_REFERENCE | CRT_BVH_REBUILT */
    int32_t leaf_size;        /* REBUILT: max triangles per leaf, 1..16 (0 = default 4) */
    int32_t layouts;          /* REBUILT: 1 (single left-first order) or 6 (direction-ordered, default) */
    float traversal_cost;     /* REBUILT: SAH cost of one node step relative to one triangle test (0 = default 2) */
    int32_t width;            /* REBUILT: 4 (default) = 4-wide nodes, stack traversal (kernel variant 4); the
                                 tree holds at most 2^24 - 1 primitive references (24-bit record addressing in the
                                 leaf rounds; larger scenes fail with CRT_ERR_INVALID_ARGUMENT);
                                 2 = threaded binary layouts (variants 0-3) */
    int32_t gpu_build;        /* REBUILT: 1 = build the binned-SAH tree on the GPU (crt_scene_create_ex: the scene's
                                 device; crt_scene_export: device 0), 0 = on the host (default) */
    int32_t stack_cap;        /* REBUILT width 4: 0 = the traversal-stack bound computed from the tree (default); > 0
                                 overrides it.  Testing only: a value below the bound makes a render that needs more
                                 entries report CRT_ERR_HIP at synchronisation (the entries are dropped). */
    int32_t spatial_splits;   /* REBUILT: 1 = binned SAH with spatial splits (SBVH, Stich et al. 2009): a primitive
                                 straddling a split plane is referenced from both sides, each reference boxed by its
                                 part of the triangle.  Built on the host (gpu_build is ignored).  0 = object splits
                                 only (default). */
    float spatial_alpha;      /* spatial_splits: try a spatial split where the object split's children overlap by more
                                 than this fraction of the root's surface area (0 = default 1e-5) */
    float spatial_max_dup;    /* spatial_splits: stop splitting once references exceed (1 + this) x primitives
                                 (0 = default 1.0) */
} crt_scene_options;

/* ---- scene (SceneManager device half) ---- */
/* Host-only: build the device arrays crt_scene_create_ex would upload and copy them out (no GPU needed;
 * used by the CPU tests to validate the rebuilt BVH).  4-wide nodes are returned in their logical row order;
 * crt_scene_create_ex uploads them swizzled (row k of node n at 16-B slot k ^ (n & 7) of its 128-B record).
 * Call with null arrays to get the sizes:
 * info = {node float4s, prim float4s, ranks, nodes per layout, layouts, width, stack bound, excluded,
 *         first per-ray sphere prim, per-ray spheres}. */
int  crt_scene_export(const crt_scene_desc* desc, const crt_scene_options* opts, float* nodes, float* prims,
                      int32_t* rank_code, int64_t info[10]);
int  crt_scene_create(const crt_scene_desc* desc, int device, crt_scene** out);
/* crt_scene_create with options (NULL = defaults = CRT_BVH_REFERENCE).
 * A scene needs at least one object; there is no sky-only scene.  n_objects == 0 is CRT_ERR_INVALID_ARGUMENT: "scene
 * has no BVH nodes" when n_scene_nodes is 0 as well, "scene leaf object out of range" when scene_nodes still holds a
 * leaf (every leaf must name an object below n_objects).  Any number of spheres is accepted.  CRT_BVH_REBUILT, width 4: up to 8
 * spheres are tested once per ray behind the reference's own box test for them; with more, the spheres of radius
 * below 1 go into the tree's leaves and those of radius >= 1 stay per ray, of which there may then be at most 8
 * (more: CRT_ERR_INVALID_ARGUMENT; width 2 takes any number).  Only per ray is a sphere's reference box replayed,
 * which a large sphere needs: its f32 roots can land outside its own box.
 * Both create calls return after the uploads have completed on the device: the scene may be used on any stream at once. */
int  crt_scene_create_ex(const crt_scene_desc* desc, int device, const crt_scene_options* opts, crt_scene** out);
int  crt_scene_get_stats(const crt_scene* scene, crt_scene_stats* out);
void crt_scene_destroy(crt_scene* scene);

/* Diagnostic (no reference counterpart): renders spp samples per pixel following scene A (the
 * renderer's RNG state is consumed, its framebuffer is left untouched) and traces every ray through
 * scene B as well.  out = {rays, rays whose hit primitive differs, rays with the same primitive but a
 * different t, of the differing rays those B misses, those A misses}.  Both scenes must come from the
 * same crt_scene_desc.  Synchronous. */
int  crt_scene_compare(crt_renderer* r, const crt_scene* a, const crt_scene* b, int spp, int max_bounces,
                       uint64_t out[5]);
/* As crt_scene_compare, also copying up to max_dump differing rays to dump (10 floats each:
 * o.xyz, d.xyz, rank in a, rank in b (int bits), t in a, t in b). */
int  crt_scene_compare_dump(crt_renderer* r, const crt_scene* a, const crt_scene* b, int spp, int max_bounces,
                            uint64_t out[5], float* dump, int max_dump);

/* ---- ray queries (no reference counterpart: the reference traces only the rays its render kernel generates) ----
 * A batch of caller-supplied rays against a device scene: closest hit or occlusion (DESIGN.md "Ray queries").
 * Closest hit = the reference's own query, scene.hit(ray, Interval(0.001f, INFINITY)) (CUDAKernels.h:123), with the
 * render kernels' hit rule (closest t, ties to the higher reference DFS rank); it is reported only when t <= tmax.  The
 * traversal always runs over [0.001, inf): tmax filters the result, it never changes which boxes or primitives the
 * traversal accepts.  Occlusion = "the closest-hit query reports a hit".
 * Preconditions per ray: every component of origin and dir finite, dir not all-zero (zero components of either sign
 * are fine), |origin| < 2^59, tmax not NaN.  The host-pointer entries check them before anything is launched; for the
 * device-pointer entry they are the caller's duty. */
typedef struct crt_ray { float origin[3]; float tmax; float dir[3]; float reserved; } crt_ray;   /* dir: not normalised; t is in units of dir */
/* object: index into desc.meshes, or -1 - index into desc.spheres; primitive: triangle of the mesh after the build
 * permutation (indices[index_offset + 3 * primitive ..]), 0 for a sphere; material: the index shade() uses (triangle:
 * face_materials[face_offset + primitive] + material_id_offset; sphere: its material), as is even when out of range;
 * normal: the outward geometric unit normal, not flipped (triangle: the shading record's unit(cross(e1, e2)), Mesh.cuh:
 * 303-304; sphere: (1 / r) * (P - c), P = o + t * d, Sphere.cuh:44); front_face = dot(dir, normal) < 0 (HitInfo.cuh:16).
 * A miss: t = -1.f, every other field 0. */
typedef struct crt_hit { float t; int32_t object, primitive, material; float normal[3]; int32_t front_face; } crt_hit;
typedef struct crt_trace_options {
    int32_t mode;        /* 0 = automatic (4-wide scenes: 2 from 2^20 rays per call, else 1; the records are the same);
                            1 = one ray per lane (trace / trace4); 2 = wave-cooperative stream kernel (4-wide scenes only).
                            Over 4-wide nodes mode 1 keeps a fixed 64-entry stack per lane, three entries per level:
                            a tree with 3 * stack_bound > 64 is CRT_ERR_UNSUPPORTED in mode 1, and mode 0 takes 2 */
    int32_t grid_waves;  /* 0 = automatic; > 0: testing only, caps the persistent grid so few rays still refill lanes */
    int32_t stack_lds;   /* 0 = default; 1..16 as crt_renderer_set_stack_lds (1 forces the HBM overflow path); the stream
                            kernel keeps at most 12 entries in LDS (one-wave workgroups at 6 per SIMD), so 13..16 act as 12 */
    int32_t refill_threshold; /* 0 = default; idle lanes (1..64) that trigger a refill pass */
} crt_trace_options;
typedef struct crt_trace_stats {
    float kernel_ms;               /* HIP events */
    uint64_t rays, box_tests, tri_tests, sphere_tests; /* only when counting was requested */
    uint64_t step_lane_slots, step_active_lanes;  /* traversal steps x 64, and lanes with a node in them: lane fill */
} crt_trace_stats;
#define CRT_TRACE_COUNT_WORK 1u   /* crt_scene_trace_device flags bit 0 */

/* Host only, no GPU: CRT_OK, or CRT_ERR_INVALID_ARGUMENT with *first_bad (optional) = the first ray that breaks a
 * precondition (crt_last_error names it too). */
int crt_trace_validate_rays(const crt_ray* rays, int64_t n, int64_t* first_bad);
/* Host only like crt_scene_export: the per-rank identity table, n_ranks x 3 ints (object, primitive, material), the
 * same for every bvh mode of one description.  out == NULL: only *n_ranks is set. */
int crt_scene_export_identity(const crt_scene_desc* desc, const crt_scene_options* opts, int32_t* out, int64_t* n_ranks);
/* Host pointers, synchronous; n up to 2^31 - 1 (traced in chunks through staging buffers the scene owns).  n == 0:
 * CRT_OK, nothing launched.  A device error (e.g. a traversal-stack entry dropped below the tree's bound) is
 * CRT_ERR_HIP.  A scene handle serves one trace call at a time. */
int crt_scene_trace(const crt_scene* scene, const crt_ray* rays, int64_t n, const crt_trace_options* opts, crt_hit* hits_out);
int crt_scene_occluded(const crt_scene* scene, const crt_ray* rays, int64_t n, const crt_trace_options* opts, uint8_t* out);
/* Device pointers on the scene's device, 16-B aligned; enqueued on `stream`, asynchronous.  d_hits / d_occluded: either
 * may be NULL, not both (only d_occluded: the occlusion query, whose lanes retire at the first accepted hit).  Device
 * errors of the launch are reported by crt_scene_trace_last_stats. */
int crt_scene_trace_device(const crt_scene* scene, const crt_ray* d_rays, int64_t n, const crt_trace_options* opts,
                           crt_hit* d_hits, uint8_t* d_occluded, unsigned flags, void* stream);
/* The indirect query (DESIGN.md "Device-side batch sizes"): traces rays [0, min(*d_n, capacity)), where *d_n is a 4-byte
 * aligned device word that the kernel reads on `stream` when it runs; the host never reads it.  capacity, in [0, 2^30]
 * (one launch serves one query), is what the host sizes the launch by: the grids, and automatic mode's choice between
 * the two kernels.  The clamp is in the kernel: whatever the word holds, no row at or beyond capacity is read or
 * written, and rows of d_hits / d_occluded from min(*d_n, capacity) on are not written.  The rows that are written
 * hold crt_scene_trace_device's records of the same rays, bit for bit, in every mode; with CRT_TRACE_COUNT_WORK the
 * `rays` of crt_scene_trace_last_stats is the clamped count.  capacity == 0: CRT_OK, nothing launched.  Everything else
 * as crt_scene_trace_device.  Joined ABI version 3 after its first release, like the path steps below. */
int crt_scene_trace_indirect_device(const crt_scene* scene, const crt_ray* d_rays, const uint32_t* d_n, int64_t capacity,
                                    const crt_trace_options* opts, crt_hit* d_hits, uint8_t* d_occluded,
                                    unsigned flags, void* stream);
/* Of the last trace on this scene; synchronises with it.  The work counts are 0 unless it counted (the host entries
 * never count; mode 1 over a 4-wide scene counts rays only). */
int crt_scene_trace_last_stats(const crt_scene* scene, crt_trace_stats* out);

/* ---- path steps (no reference counterpart: the reference keeps them inside rayColor) ----
 * What a path tracer does between two ray queries, over batches (DESIGN.md "Path steps"): camera rays on the pixels'
 * own RNG streams, and one bounce of material scattering with the bounce limit and Russian roulette.  With
 * crt_scene_trace_device in between they form a wavefront path tracer whose sums, RNG state and ray count equal
 * crt_renderer_render's bit for bit: every lane draws in the render kernels' order (disk candidates, the two pixel
 * uniforms, then per bounce the roulette draw, the trace, the material's draws), and a pixel's sum receives the same
 * additions in the same order, the + (0, 0, 0) of a killed path included.
 * RNG state and sums have the renderer's layouts: 6 words per pixel (v[5], d) and W*H*3 floats, both indexed by pixel,
 * so the entries run on crt_renderer_rng_device_ptr / crt_renderer_linear_device_ptr (or an attached buffer) and
 * crt_renderer_init_rand / crt_renderer_resolve serve them unchanged.  Both device entries are asynchronous on
 * `stream`; rays, hits and paths are 16-B aligned device arrays; n == 0 is CRT_OK with nothing launched; a null
 * pointer, n < 0 or n >= 2^31 is CRT_ERR_INVALID_ARGUMENT, checked before any device use.  These entries joined ABI
 * version 3 after its first release: a caller that may meet an older library looks the symbols up. */
/* One path of a batch; two 16-B rows like crt_ray / crt_hit. */
typedef struct crt_path { float throughput[3]; int32_t bounce; int32_t pixel; int32_t status; int32_t reserved[2]; } crt_path;
#define CRT_PATH_ACTIVE 0
#define CRT_PATH_ENDED  1
/* Camera::getRay (Camera.cuh:32-44) for n pixels of the renderer's frame, each on its own RNG stream: the unit-disk
 * rejection loop, then the two pixel uniforms, exactly the render kernels' camera block (with the fast or IEEE u, v
 * division the renderer chose for its frame size).  d_pixels[k] = y * width + x (NULL: pixels 0..n-1); no pixel may
 * appear twice in one call.  d_rng NULL = the renderer's own state.  Writes rays[k] = (o, +inf, d, 0) and paths[k] =
 * {(1, 1, 1), 0, pixel, CRT_PATH_ACTIVE}.  A pixel outside the frame draws nothing and gets a CRT_PATH_ENDED path.
 * CRT_ERR_INVALID_ARGUMENT for a renderer without a camera. */
int crt_renderer_camera_rays_device(crt_renderer* r, const int32_t* d_pixels, int64_t n, uint32_t* d_rng,
                                    crt_ray* d_rays, crt_path* d_paths, void* stream);
/* One bounce for n paths: rayColor's loop body after the hit query (CUDAKernels.h:123-142, Material.cuh:66-146), then
 * the NEXT iteration's bounce-limit test and Russian roulette (:110-121; nothing draws between the two).  hits[k] is
 * the crt_hit of rays[k] as the ray queries write it for tmax = +inf (t < 0: a miss, the sky): the step reads t,
 * material, normal and front_face; hit point = o + t * d, shading normal = front_face ? normal : -normal.  A material
 * index outside the scene's materials is the reference's invalid-material bounce (the same ray again, ++bounce).
 * A path that continues gets its scattered ray in rays[k] (tmax = +inf), its throughput and bounce updated and stays
 * CRT_PATH_ACTIVE.  One that ends -- sky, light, absorbed metal, bounce limit, roulette -- adds its contribution,
 * possibly (0, 0, 0), to d_linear[3 * pixel ..], keeps its ray and becomes CRT_PATH_ENDED.  Entries that come in
 * CRT_PATH_ENDED, or whose pixel is outside [0, n_pixels), are left untouched (ray, path, RNG, sum).  d_rng and
 * d_linear hold n_pixels pixels.  No two active entries of one call may name the same pixel.  max_bounces >= 1. */
int crt_scene_path_step_device(const crt_scene* scene, crt_ray* d_rays, const crt_hit* d_hits, crt_path* d_paths,
                               int64_t n, int max_bounces, uint32_t* d_rng, float* d_linear, int64_t n_pixels,
                               void* stream);
/* Step, regenerate and compact in one kernel (DESIGN.md "Path queues"): what crt_scene_path_step_device does for each
 * entry of a READ-ONLY input batch, then the entry's fate.  A path that goes on is appended to the output batch
 * (d_rays_out, d_paths_out: n entries each, overlapping neither each other nor an input).  One that ended adds its
 * contribution to its pixel's sum; while d_remaining[pixel] > 0 (int32 per pixel of the renderer's frame: samples not yet
 * started) it decrements that count, draws the pixel's next camera sample as crt_renderer_camera_rays_device does, on the
 * RNG state the lane already holds, and appends the new ray with the path {(1, 1, 1), 0, pixel, CRT_PATH_ACTIVE}.  One
 * that ended with no sample left appends nothing.  Entries that come in CRT_PATH_ENDED, or whose pixel is outside the
 * renderer's frame, draw nothing, add nothing and append nothing.  d_remaining NULL: never regenerate (step and compact).
 * *d_count (device) is set to 0 on `stream` before the kernel and counts the entries appended; they are entries
 * 0 .. *d_count - 1 of the outputs, in no particular order (no result depends on it), and the rest of the outputs is
 * unspecified.  d_rng / d_linear NULL: the renderer's own state and sums; the camera and the fast / IEEE u, v choice are
 * the renderer's, n_pixels its width * height.  No two active entries may name the same pixel.  Asynchronous.
 * CRT_ERR_INVALID_ARGUMENT before any device use: a null or misaligned array, n < 0 or n >= 2^31, overlapping outputs,
 * max_bounces < 1, scene and renderer on different devices, a renderer without a camera.  n == 0: CRT_OK, *d_count
 * zeroed, no kernel. */
int crt_scene_path_advance_device(const crt_scene* scene, crt_renderer* r, const crt_ray* d_rays, const crt_hit* d_hits,
                                  const crt_path* d_paths, int64_t n, int max_bounces, uint32_t* d_rng, float* d_linear,
                                  int32_t* d_remaining, crt_ray* d_rays_out, crt_path* d_paths_out, uint32_t* d_count,
                                  void* stream);
/* The indirect advance: what crt_scene_path_advance_device does for entries [0, min(*d_n, capacity)), with *d_n read by
 * the kernel on `stream` and the clamp in the kernel.  The arrays hold capacity entries (the overlap checks use it in
 * place of n); the grid is sized by it and workgroups beyond the count do nothing.  d_count, zeroed on the stream and
 * then counting the appended entries, must not be d_n.  d_totals: NULL, or two 8-byte aligned 64-bit device words that
 * the kernel adds to and never clears: [0] += the clamped input count, [1] += 1 if that count is not 0 -- how a loop
 * that runs ahead of the host still reports its rays and iterations.  Every input entry appends at most one output
 * entry, so *d_count <= min(*d_n, capacity): a chain of trace / advance calls may keep the first capacity. */
int crt_scene_path_advance_indirect_device(const crt_scene* scene, crt_renderer* r, const crt_ray* d_rays,
        const crt_hit* d_hits, const crt_path* d_paths, const uint32_t* d_n, int64_t capacity, int max_bounces,
        uint32_t* d_rng, float* d_linear, int32_t* d_remaining, crt_ray* d_rays_out, crt_path* d_paths_out,
        uint32_t* d_count, uint64_t* d_totals, void* stream);
/* Input entries per reservation of output slots in this build of the advance kernel (64: one per wave; 256 .. 1024: one
 * per 256-lane workgroup over 1 .. 4 chunks).  Host only; for measurements, no result depends on it. */
int crt_path_advance_entries(void);
/* A whole frame as a wavefront on the device: camera rays for every pixel, then trace / advance rounds over two
 * ping-pong batches until none is left, spp samples per pixel with regeneration (remaining = spp - 1).  Sums, RNG
 * state and the number of rays equal crt_renderer_render's bit for bit.  flags: CRT_RENDER_ACCUMULATE adds to the sums
 * (they are zeroed otherwise); CRT_RENDER_COUNT_WORK is CRT_ERR_UNSUPPORTED, and so is a pixel shard other than (0, 1).
 * trace_opts: the queries' options (NULL: defaults).  The host waits once per round, for the 4-byte size of the next
 * batch.  Synchronous on return; a device error of a query is CRT_ERR_HIP.  spp == 0 clears the sums (unless
 * accumulating) and traces nothing.  max_bounces >= 1.  The batches belong to the renderer handle: 164 B per pixel (two
 * ray, two path and one hit batch, the per-pixel sample counts), about 0.6 GB at 2560x1440, allocated by the first call
 * and freed with the handle.  stats_out (optional): rays traced, rounds, and HIP-event milliseconds round the loop. */
typedef struct crt_wavefront_stats { uint64_t rays; uint32_t iterations; float ms; } crt_wavefront_stats;
int crt_renderer_render_wavefront(crt_renderer* r, const crt_scene* scene, int spp, int max_bounces, unsigned flags,
                                  const crt_trace_options* trace_opts, crt_wavefront_stats* stats_out, void* stream);
/* The same frame with the loop enqueued ahead of the host: blocks of sync_every rounds of indirect trace and indirect
 * advance on two ping-pong count words, then one copy of the count, the totals and the error word and one host wait.
 * The last count the host read is the capacity of every round of the next block; rounds enqueued after the count
 * reached 0 trace nothing and append nothing, so the frame does not depend on sync_every.  stats_out->rays and
 * ->iterations come from the device totals and equal crt_renderer_render_wavefront's.  The queries of one call OR their
 * device errors into one word that is cleared once per call and reported as CRT_ERR_HIP.  sync_every >= 1 as is; 0 the
 * library's default; negative: CRT_ERR_INVALID_ARGUMENT.  At most 2^30 pixels.  Everything else, the refusals
 * included, as crt_renderer_render_wavefront, whose scratch it shares. */
int crt_renderer_render_wavefront_queued(crt_renderer* r, const crt_scene* scene, int spp, int max_bounces, unsigned flags,
                                         const crt_trace_options* trace_opts, int sync_every,
                                         crt_wavefront_stats* stats_out, void* stream);
/* Path finish (DESIGN.md "Path finish"): take a batch of paths and run them to their ends in one kernel, one lane per
 * entry of a READ-ONLY batch (rays and paths; no hits).  The lane loads its pixel's RNG state, sum and
 * d_remaining[pixel] once, then per ray: the lane kernels' closest-hit traversal in the lane, the crt_hit record in
 * registers, the step of crt_scene_path_step_device, and when the path ended its contribution added to the sum and,
 * while samples are left, one taken and its camera ray drawn as crt_scene_path_advance_device does.  At the end it
 * stores the state, the sum and d_remaining[pixel] = 0.  The entry's first ray keeps its row's tmax; every later ray
 * has +inf.  State, sums and d_remaining end as a loop of crt_scene_trace_device and crt_scene_path_advance_device run
 * until its count is 0 leaves them, bit for bit.  Every iteration increments the bounce or ends the path, and an
 * ended path takes a sample or leaves: a lane traces at most (d_remaining[pixel] + 1) * max_bounces rays, and the
 * kernel's time is its longest lane's.  Entries: capacity, or min(*d_n, capacity) with *d_n (NULL: capacity entries)
 * read by the kernel on `stream` and clamped there.  Entries that come in CRT_PATH_ENDED, whose pixel is outside the
 * renderer's frame, or at or beyond the count read and write nothing.  d_rng / d_linear NULL: the renderer's own;
 * d_remaining NULL: never regenerate, each path only to its own end.  d_totals: NULL, or the advance's two 64-bit
 * words: [0] += the rays this call traced, [1] += 1 if the clamped count is not 0.  No two active entries may name
 * the same pixel.  Asynchronous.  CRT_ERR_INVALID_ARGUMENT before any device use: a null or misaligned array, capacity
 * < 0 or >= 2^31, a misaligned d_n or d_totals, max_bounces < 1, scene and renderer on different devices, a renderer
 * without a camera.  CRT_ERR_UNSUPPORTED: a 4-wide scene whose stack bound the in-lane traversal's 64-entry stack
 * cannot hold (3 * bound > 64; ray-query mode 1 refuses the same trees).  capacity == 0: CRT_OK, nothing launched. */
int crt_scene_path_finish_device(const crt_scene* scene, crt_renderer* r, const crt_ray* d_rays, const crt_path* d_paths,
        const uint32_t* d_n, int64_t capacity, int max_bounces, uint32_t* d_rng, float* d_linear, int32_t* d_remaining,
        uint64_t* d_totals, void* stream);
/* crt_renderer_render_wavefront_queued with a hand-off: whenever the host holds a batch size m (the number of pixels
 * before the first round, then each block's read that gives m > 0) and m <= finish_below, the current batch goes to
 * crt_scene_path_finish_device with its count word and capacity m, and the frame is done after one more copy and
 * wait.  finish_below 0: never, the queued loop's frame, rounds and numbers; >= the number of pixels: the whole frame
 * through the finish kernel straight after the camera rays; -1: the library's default (921,600 in this build, DESIGN.md §19's
 * measurement, or 0 on a scene the finish call refuses); other negatives: CRT_ERR_INVALID_ARGUMENT.  finish_below > 0 on a scene the finish call refuses:
 * CRT_ERR_UNSUPPORTED before any work.  The same sums, RNG state and rays for every value; stats_out->iterations: the
 * rounds, plus one for a finish that got an entry.  Everything else as the queued entry. */
int crt_renderer_render_wavefront_finish(crt_renderer* r, const crt_scene* scene, int spp, int max_bounces, unsigned flags,
        const crt_trace_options* trace_opts, int sync_every, int64_t finish_below, crt_wavefront_stats* stats_out,
        void* stream);
/* ---- adaptive sampling (no reference counterpart; DESIGN.md "Adaptive sampling") ----
 * A frame whose 8x8 tiles (the tile kernels' own: tiles_x = (W + 7) / 8, tile t covers x = (t % tiles_x) * 8 .. + 7,
 * y = (t / tiles_x) * 8 .. + 7) stop receiving samples once they look converged.  Every pixel first receives spp_min
 * samples, in two ordinary renders of spp_min / 2 (the automatic kernel choice, fresh sums).  Then for n = spp_min,
 * 2 spp_min, ... while n < spp_max, the tiles that hold n samples get an error estimate from the two halves of their
 * samples (P = the sums after n / 2, Q = the sums of the other n / 2; per pixel d = |P - Q| summed over the channels,
 * I = the sum of the channels / n, e = I > 0 ? (d / (n / 2)) / sqrt(I) : 0, the term of Dammertz et al.'s stopping
 * condition; the tile's error E is the mean of e over its in-frame pixels).  A tile with !(E <= tolerance) is refined
 * to min(2n, spp_max) samples by one launch of the tile kernel (variant 8 on 4-wide scenes, 10 on threaded ones) over
 * the list of such tiles, in tile order; a tile with E <= tolerance is never looked at again.  The host waits once
 * per pass, for the 4-byte length of the list.  Because a pixel's samples come from its own RNG stream in order, a tile
 * that ends with n samples holds the sums and RNG state of crt_renderer_render(n), bit for bit.  The estimate is biased:
 * the stopping rule looks at the samples it stops, and a tile whose first spp_min samples miss a rare bright path is
 * declared converged.  tolerance = +inf is the frame of spp_min samples (with tile errors), tolerance < 0 that of spp_max.
 * reserved: 0; measurements only, no result depends on them: bit 0 lists the tiles of a pass by error, largest first
 * (measured slower than tile order);
 * bit 1 runs the first tiles of a pass's list at crt_renderer_set_critical_tiles' threshold (variant 8).
 * stats_out (optional): samples = the sum over tiles of in-frame pixels x samples; passes = refinement launches;
 * tiles_refined = tiles that got at least one; tiles_at_max = tiles that ended at spp_max; ms = HIP events round the call.
 * Synchronous on return; device errors as crt_renderer_synchronize reports them.  Before any device work,
 * CRT_ERR_INVALID_ARGUMENT: a null handle or options, spp_min < 2 or odd, spp_max < spp_min, a NaN tolerance, max_bounces
 * < 1, scene and renderer on different devices, no camera; CRT_ERR_UNSUPPORTED: any render flag, a pixel shard other than
 * (0, 1).  The state belongs to the renderer handle (W*H*3 floats and six words per tile), allocated by the first call
 * and freed with the handle.  The listed tiles are compacted by one workgroup (and, for the self-test's list and bit 0, ordered by
 * counting: listed^2 integer compares, DESIGN.md section 20 has the times).  These entries joined ABI version 3 after its first release. */
typedef struct crt_adaptive_options { int32_t spp_min, spp_max; float tolerance; int32_t reserved; } crt_adaptive_options;
typedef struct crt_adaptive_stats { uint64_t samples; uint32_t passes, tiles_refined, tiles_at_max; float ms; } crt_adaptive_stats;
int crt_renderer_render_adaptive(crt_renderer* r, const crt_scene* scene, const crt_adaptive_options* options,
                                 int max_bounces, unsigned flags, crt_adaptive_stats* stats_out, void* stream);
/* crt_renderer_resolve with each pixel's own scale, 1.f / (float)(the samples its tile holds): a tile at n samples gets
 * the bytes crt_renderer_resolve(1.f / n) gives a uniform n-spp frame.  After an adaptive render (or plan self-test). */
int crt_renderer_resolve_adaptive(crt_renderer* r, void* stream);
/* The per-tile state, tiles_y x tiles_x row-major: samples held, and the last error estimate (0 for a tile no plan
 * looked at).  crt_renderer_read_adaptive_prev: the W*H*3 half-buffer sums.  CRT_ERR_INVALID_ARGUMENT before the
 * renderer's first adaptive call.  They wait for the device. */
int crt_renderer_read_tile_spp(crt_renderer* r, int32_t* host_out);
int crt_renderer_read_tile_error(crt_renderer* r, float* host_out);
int crt_renderer_read_adaptive_prev(crt_renderer* r, float* host_out);
/* Self-test of one plan step (like crt_selftest_tile_schedule: no camera or scene): uploads sum (W*H*3, into the
 * renderer's own linear buffer), prev (W*H*3) and tile_spp (tiles) into the renderer's buffers and runs the host
 * function the loop calls with (n, next, tolerance).  list_out (capacity: tiles) gets the listed tiles, largest error
 * first, *n_listed_out their number; tile errors, tile samples and prev are read with the three readers. */
int crt_selftest_adaptive_plan(crt_renderer* r, const float* sum, const float* prev, const int32_t* tile_spp, int n,
                               int next, float tolerance, uint32_t* list_out, uint32_t* n_listed_out);
/* ---- denoiser (no reference counterpart; DESIGN.md "Denoiser") ----
 * The edge-avoiding a-trous wavelet filter of Dammertz, Sewtz, Hanika and Lensch (HPG 2010), guided by first-hit buffers.
 *
 * crt_renderer_compute_guides: one record of 8 floats per pixel of the renderer's frame, (normal.xyz, t) (position.xyz,
 * key), from three steps on `stream`: a kernel writes the pixel-centre rays (CRT::RayQuery::centreRays' operations:
 * u = ((float)x + 0.5f) / (float)W, v = ((float)y + 0.5f) / (float)H, dir = ((lower_left + u * horizontal) + v *
 * vertical) - origin, the camera's origin, lens offset 0, tmax = +inf); crt_scene_trace_device traces them with
 * trace_opts (NULL = defaults) into a hit buffer of the handle; a pack kernel fills the records: normal and t are the
 * crt_hit's own (the outward geometric normal, not flipped), position = o + t * d (a multiply, then an add), key = object
 * as int bits; a miss is t = -1, normal and position 0, key = 0x7fffffff.  No RNG state is consumed and no sum is touched.
 * The guides stay valid until the camera, the scene or the frame size changes; that is the caller's duty.  Asynchronous.
 * Before any device work, CRT_ERR_INVALID_ARGUMENT: null handles, scene and renderer on different devices, no camera;
 * CRT_ERR_UNSUPPORTED: a pixel shard other than (0, 1).
 *
 * crt_renderer_denoise: c_0 = scale * sum per channel (CRT_DENOISE_TILE_SCALE: scale = 1.f / (float)tile_spp[tile] as
 * crt_renderer_resolve_adaptive forms it, `scale` is ignored; without adaptive state CRT_ERR_INVALID_ARGUMENT).  Iteration
 * i = 0 .. iterations - 1 has stride s = 1 << i and maps c_i to c_{i+1}; the last one is the handle's `denoised` buffer
 * (W*H*3 floats).  The sums, the RNG state and the RGBA8 buffer are not touched.  Everything is f32, uncontracted, division
 * correctly rounded:
 *   h = (1/16, 1/4, 3/8, 1/4, 1/16), k(dy, dx) = h[dy + 2] * h[dx + 2] (exact constants).
 *   Host side, per call: inv_n = 1.f / (sigma_normal * sigma_normal), inv_x likewise from sigma_position, inv_c likewise
 *   from sigma_color for iteration 0, then inv_c = inv_c * 4.f after every iteration.  A term whose sigma is +inf is off:
 *   it is not computed and contributes +0.
 *   Per pixel p the taps q = (x + dx s, y + dy s), dy = -2 .. 2 outer, dx = -2 .. 2 inner; the centre in its place with
 *   w = 1 and nothing computed.  Any other tap is skipped if it lies outside the frame, if key(q) != key(p), or if
 *   !(X < 80.f); else w = exp_neg(X).  X = (dc * inv_c + dn * inv_n) + dx_ * inv_x with each d = ((a.x - b.x)^2 +
 *   (a.y - b.y)^2) + (a.z - b.z)^2 over c_i(p), c_i(q) / the normals / the positions.  Per tap kw = k * w;
 *   acc.c = acc.c + kw * q.c per channel; sw = sw + kw.  c_{i+1}(p) = acc / sw per channel (sw >= 9/64).  A skipped tap is
 *   not multiplied in: with the colour term on, a NaN or infinite neighbour (X is NaN or inf) never spreads and a NaN
 *   centre stays a NaN of that pixel alone.
 *   exp_neg(X), 0 <= X < 80: k = rintf(X * 0x1.715476p+0f); r = (X - k * 0.693359375f) - k * -0x1.bd0106p-13f; t = -r;
 *   p = ((((((C6 t + C5) t + C4) t + C3) t + 0.5f) t + 1.f) t + 1.f, C6 = 0x1.6c16c2p-10f, C5 = 0x1.111112p-7f,
 *   C4 = 0x1.555556p-5f, C3 = 0x1.555556p-3f, every * and + a separate operation; the result is the float whose bits
 *   are bits(p) - ((int)k << 23).  exp_neg(0) = 1; the relative error against exp is at most 2.5e-7.
 * There are no default sigmas: their scale depends on the scene.  flags bit 31 (CRT_DENOISE_DIRECT_ONLY) is a measurement
 * switch: every iteration through the direct kernel (one lane per pixel, taps from global memory) instead of the tiled
 * one (rows staged in LDS) at the strides where that one is used; the bits are the same.
 * stats_out (optional): guides_ms = HIP events round the last crt_renderer_compute_guides, filter_ms = round this call's
 * launches, iterations = those run, pixels_hit = the pixels whose guide is a hit (0 after crt_selftest_denoise's upload).
 * With stats_out the call waits for its last launch; without, it is asynchronous.  Before any device work,
 * CRT_ERR_INVALID_ARGUMENT: a null handle or options, iterations outside 0..8, a sigma that is NaN, <= 0, or outside
 * [2^-50, 2^50] and not +inf, unknown flag bits, reserved != 0, a scale that is NaN or <= 0 when no tile scale is asked
 * for, no guides computed yet; CRT_ERR_UNSUPPORTED: a pixel shard other than (0, 1).
 * The state belongs to the renderer handle, is allocated by the first crt_renderer_compute_guides (or self-test) and
 * freed with the handle: 140 bytes per pixel (rays 32, hits 32, guides 32, two colour buffers of 16-byte rows 32, denoised
 * 12) and one word per 64 pixels.  These entries joined ABI version 3 after its first release. */
#define CRT_DENOISE_TILE_SCALE 1u
#define CRT_DENOISE_DIRECT_ONLY 0x80000000u
typedef struct crt_denoise_options {
    int32_t iterations;                 /* 1..8; 0 = 5 */
    float sigma_color, sigma_normal, sigma_position;   /* each in [2^-50, 2^50], or +inf = that term off */
    uint32_t flags;                     /* CRT_DENOISE_TILE_SCALE 1u; bit 31: measurement switch */
    int32_t reserved;
} crt_denoise_options;
typedef struct crt_denoise_stats { float guides_ms, filter_ms; uint32_t iterations, pixels_hit; } crt_denoise_stats;
int crt_renderer_compute_guides(crt_renderer* r, const crt_scene* scene, const crt_trace_options* trace_opts, void* stream);
int crt_renderer_denoise(crt_renderer* r, const crt_denoise_options* o, float scale, crt_denoise_stats* stats_out, void* stream);
/* writeColor of the denoised buffer with scale 1 into the RGBA8 buffer (crt_renderer_resolve's kernel). */
int crt_renderer_resolve_denoised(crt_renderer* r, void* stream);
/* W*H*3 floats / W*H*8 floats; they wait for the device.  CRT_ERR_INVALID_ARGUMENT before the first denoise / guides. */
int crt_renderer_read_denoised(crt_renderer* r, float* host_out);
int crt_renderer_read_guides(crt_renderer* r, float* host_out);
/* Per launch of the last crt_renderer_denoise that had a stats pointer (it records an event after every launch; without
 * one it records none): out9[0] = the kernel that forms c_0, out9[1 + i] = iteration i, 0 for iterations not run.
 * Waits for that call's last launch.  CRT_ERR_INVALID_ARGUMENT when there was no such call. */
int crt_renderer_denoise_iteration_ms(crt_renderer* r, float* out9);
/* The denoised buffer on the device (W*H*3 floats), NULL before the handle's denoiser state exists. */
float* crt_renderer_denoised_device_ptr(crt_renderer* r);
/* Self-test of the filter (like crt_selftest_adaptive_plan: no camera or scene): uploads color (W*H*3, into the
 * renderer's own linear buffer, taken with scale 1) and guides (W*H*8) into the renderer's buffers, runs the host
 * function crt_renderer_denoise calls on the null stream and reads the result into out (W*H*3).  The tile scale flag is
 * CRT_ERR_INVALID_ARGUMENT here. */
int crt_selftest_denoise(crt_renderer* r, const float* color, const float* guides, const crt_denoise_options* options,
                         float* out);
/* ---- reprojection: a frame's history across camera moves (no reference counterpart; DESIGN.md "Reprojection") ----
 * (In this library "temporal" names the temporal tile order, crt_renderer_set_temporal_order; this feature is called
 * reproject / history throughout.)
 *
 * crt_renderer_reproject blends the frame in the sums, c = scale * sum per channel (formed as crt_renderer_denoise forms
 * c_0), into a per-pixel history that follows the camera: each pixel finds where its first hit (the current guides,
 * crt_renderer_compute_guides) lay in the previous frame and takes the history there if the previous guides vouch for it.
 * Everything is f32, uncontracted, division correctly rounded.  dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; dist2 is
 * the denoiser's d above.
 * State per renderer handle, allocated by the first call and freed with the handle: two history buffers of one 16-byte
 * row (r, g, b, len) per pixel (a ping-pong pair), a second guide buffer (the handle then holds two behind an index: the
 * one a call read as current is kept as the next call's previous, nothing is copied), the previous guide camera (the
 * crt_camera_desc crt_renderer_compute_guides made its rays from) and a `valid` flag: 64 bytes per pixel and one word per
 * 64-pixel row segment.  crt_renderer_read_guides and crt_renderer_denoise keep seeing the current guides.  Guides that
 * crt_selftest_denoise uploaded have no guide camera (all zero): as the previous frame of a later call they give no pixel
 * a history (LN = 0, so s > 0 fails), and that call starts over.
 * Per pixel p with current guide (n, t) (pos, key), W and H the frame's size in pixels:
 *   1. No history if the state is not valid (first call, after crt_renderer_reset_history), if key == 0x7fffffff (a miss)
 *      or if a channel of c is not finite: out = (c, 1.f).
 *   2. The previous guide camera (o, ll, hor, ver).  Host side, once per call: L = ll - o; N = cross(hor, ver), each
 *      component a * b - c * d as two products and a subtraction; LN = dot(L, N); hh = dot(hor, hor); vv = dot(ver, ver);
 *      tol2 = position_tolerance * position_tolerance.  Per pixel: d = pos - o; s = LN / dot(d, N); q = s * d - L (a
 *      multiply, then a subtraction); u = dot(q, hor) / hh; v = dot(q, ver) / vv; fx = u * (float)W - 0.5f; fy = v *
 *      (float)H - 0.5f.  No history unless s > 0 && fx > -1.f && fx < (float)W && fy > -1.f && fy < (float)H (a NaN fails).
 *      x0 = floorf(fx), ax = fx - x0, likewise y0, ay; lim = tol2 * dot(d, d).
 *   3. Four taps (x0 + i, y0 + j), j outer and i inner, w = (i ? ax : 1.f - ax) * (j ? ay : 1.f - ay).  A tap is skipped
 *      if it lies outside the frame, if !(w > 0.f), if the previous key differs from key, if !(dist2(pos, prev_pos) <= lim)
 *      (position_tolerance == +inf: off, lim is not computed and the test passes), if the normal term is on and
 *      !(dot(n, prev_n) >= normal_min) (normal_min == -inf: off, not computed, the previous normals are not loaded), or if
 *      one of the tap's three history colours is not finite.  Else acc = acc + w * row for the row's four components and
 *      sw = sw + w.
 *   4. If sw > 0: hist = acc / sw per component; m = fminf(hist.len + 1.f, max_history); a = 1.f / m; out.c = hist.c +
 *      (c.c - hist.c) * a per channel; out.len = m.  Else out = (c, 1.f).
 * After the launch the current guides and guide camera become the previous ones, the history buffers swap and valid is
 * set.  So a non-finite sample lives in the history for exactly one frame (its pixel shows it, no later tap takes it); a
 * pixel nothing vouches for restarts at len = 1; len never exceeds max_history: the running mean becomes an exponential
 * one with floor 1 / max_history.  The sums, the RNG state, the RGBA8 buffer, the guides and the denoised buffer are not
 * touched.
 * The history is biased where the frame changes and the first hit does not say so: what a glass or mirror surface shows
 * lags behind the camera by up to max_history frames, repeated bilinear resampling blurs it under motion, and a rim that
 * comes into view starts from one noisy sample.
 * There are no defaults for position_tolerance and max_history: the tolerance is relative to the distance from the
 * previous camera, and a useful value is a few pixel footprints (about 2 tan(fov_x / 2) / W each), so it depends on the
 * frame's width and field of view.
 * stats_out (optional): reproject_ms = HIP events round the launch, pixels_reprojected = the pixels with sw > 0 (ballot
 * population counts stored per wave, summed on the host), pixels_hit as crt_denoise_stats'.  With stats_out the call
 * waits for its launch; without, it is asynchronous.  Before any device work and before anything is allocated,
 * CRT_ERR_INVALID_ARGUMENT: a null handle or options, a position_tolerance that is NaN or outside [2^-50, 2^50] and not
 * +inf, a normal_min that is NaN or outside [-1, 1] and not -inf, a max_history that is NaN or outside [1, 2^24], flag
 * bits (none is defined), reserved != 0, a scale that is NaN or <= 0, no guides computed yet; CRT_ERR_UNSUPPORTED: a
 * pixel shard other than (0, 1).  These entries joined ABI version 3 after its first release. */
typedef struct crt_reproject_options {
    float position_tolerance;           /* [2^-50, 2^50] relative to the distance from the previous camera, or +inf = off */
    float normal_min;                   /* [-1, 1], or -inf = off */
    float max_history;                  /* [1, 2^24] */
    uint32_t flags;                     /* 0 */
    int32_t reserved;
} crt_reproject_options;
typedef struct crt_reproject_stats { float reproject_ms; uint32_t pixels_reprojected, pixels_hit; } crt_reproject_stats;
int crt_renderer_reproject(crt_renderer* r, const crt_reproject_options* o, float scale, crt_reproject_stats* stats_out, void* stream);
/* The next crt_renderer_reproject starts over (every pixel (c, 1)).  Nothing is freed. */
int crt_renderer_reset_history(crt_renderer* r);
/* crt_renderer_denoise with c_0 = the history colours (scale 1), through the same host function and kernels, guided by
 * the current guides; the result is the handle's `denoised` buffer (crt_renderer_resolve_denoised / _read_denoised).
 * CRT_DENOISE_TILE_SCALE is CRT_ERR_INVALID_ARGUMENT here, as is a handle without a history. */
int crt_renderer_denoise_history(crt_renderer* r, const crt_denoise_options* o, crt_denoise_stats* stats_out, void* stream);
/* writeColor of the history colours with scale 1 into the RGBA8 buffer. */
int crt_renderer_resolve_history(crt_renderer* r, void* stream);
/* W*H*4 floats (r, g, b, len); waits for the device.  CRT_ERR_INVALID_ARGUMENT before the first reprojection. */
int crt_renderer_read_history(crt_renderer* r, float* host_out);
/* The latest history on the device (W*H*4 floats), NULL before the first reprojection.  The two buffers alternate: ask
 * again after every crt_renderer_reproject. */
float* crt_renderer_history_device_ptr(crt_renderer* r);
/* Self-test of the reprojection (like crt_selftest_denoise: no camera or scene): uploads color (W*H*3, into the
 * renderer's own linear buffer, taken with scale 1), guides and prev_guides (W*H*8 each) and prev_history (W*H*4; NULL =
 * the state is not valid) into the renderer's buffers, takes prev_camera as the previous guide camera, runs the host
 * function crt_renderer_reproject calls on the null stream and reads the new history into out_history (W*H*4). */
int crt_selftest_reproject(crt_renderer* r, const float* color, const float* guides, const float* prev_guides,
                           const float* prev_history, const crt_camera_desc* prev_camera,
                           const crt_reproject_options* options, float* out_history);
/* ---- variance-guided filtering of the history (no reference counterpart; DESIGN.md "Variance-guided filter") ----
 * The spatiotemporal variance-guided filter of Schied et al. (HPG 2017) over the reprojection's history: the first two
 * luminance moments travel with the history, give a per-pixel variance, and that variance, itself filtered, sets the
 * width of the filter's luminance edge-stop per pixel and per level, so a pixel whose history is 32 frames long and one
 * that restarted a frame ago are no longer served by one sigma.  Everything is f32, uncontracted, division and sqrtf
 * correctly rounded.  lum(c) = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z.
 *
 * 1. crt_renderer_reproject_moments is crt_renderer_reproject with a second ping-pong pair of rows (m1, m2) per pixel,
 *    8 bytes each, allocated by the first call (16 bytes per pixel; a user of crt_renderer_reproject alone never pays
 *    them) and freed with the handle.  From the same state its history rows, stats and state transitions are
 *    crt_renderer_reproject's, bit for bit.  The frame's moments are l = lum(c), (l, l * l).  Where the pixel restarts
 *    (step 1 of the rule above, a failed projection, or sw == 0): out_m = (l, l * l).  Else, for exactly the taps the
 *    colour accumulation took and in its order: am = am + w * prev_m per component; hm = am / sw; out_m = hm + (new -
 *    hm) * a per component with the colours' a.  The moments are valid after this call and not valid after a
 *    crt_renderer_reproject or a crt_renderer_reset_history; a crt_renderer_reproject_moments on a history that is valid
 *    while its moments are not starts the whole history over: every pixel (c, 1), (l, l * l).
 *    crt_renderer_read_moments: W*H*2 floats, CRT_ERR_INVALID_ARGUMENT without valid moments.
 * 2. crt_renderer_denoise_history_variance first runs the estimate kernel: per pixel with history row (r, g, b, len) it
 *    writes c_0 = (r, g, b, v) into the filter's first colour buffer and v into a W*H buffer of the handle
 *    (crt_renderer_read_variance; 4 bytes per pixel, allocated by the first call).
 *      len >= min_history: v = fmaxf(0.f, m2 - m1 * m1).
 *      Else the 7 x 7 window, dy = -3 .. 3 outer and dx inner, the centre in its place: a tap q is taken if it lies
 *      inside the frame, key(q) == key(p) and both of its moments are finite; S1 = S1 + m1(q), S2 = S2 + m2(q), n = n +
 *      1.f.  n == 0: v = 0.  Else M1 = S1 / n, M2 = S2 / n, v = fmaxf(0.f, M2 - M1 * M1) * (min_history / len): the
 *      paper's boost for young pixels.
 *    fmaxf(0, NaN) is 0, so for a len in [1, 2^24], as the reprojection writes it, v is never NaN.  It is +inf where m2
 *    overflowed.
 * 3. Then the filter: iterations, strides, k, the frame test, the key test, the normal and position terms, the !(X < 80.f)
 *    skip, exp_neg and the last iteration's write into `denoised` are crt_renderer_denoise's.  The differences:
 *      The prefiltered variance g at p: a 3 x 3 Gaussian over the v of this level at +-1 pixel whatever the stride, dy
 *      outer, kg = hg[dy + 1] * hg[dx + 1], hg = (1/4, 1/2, 1/4); taps outside the frame or of another key are skipped;
 *      gs = gs + kg * v(q), gw = gw + kg, g = gs / gw.
 *      The colour term: den = sigma_luminance * sqrtf(g) + 0x1p-20f; inv_den = 1.f / den; xc = fabsf(lum(c) - lum(qc)) *
 *      inv_den (X = (xc + xn) + xx).  sigma_luminance is not halved per level: the shrinking variance does that.
 *      sigma_luminance == +inf: the term is off, g is not computed, the variance is still propagated.
 *      Per tap kw = k * w (the centre: kw = k): acc.c = acc.c + kw * qc.c; av = av + (kw * kw) * qc.w; sw = sw + kw.
 *      c_{i+1} = acc / sw per channel, v_{i+1} = av / (sw * sw).
 *    A non-finite sample: its pixel's moments are NaN, so its v is 0 (long history) or comes from its neighbours (short);
 *    as a tap its lum is not finite, X is NaN and it is skipped, so with the luminance term on no other pixel's colour
 *    becomes non-finite; as a centre it stays a NaN of that pixel alone.  A v of +inf: every pixel within +-1 of it has
 *    g = +inf, den = +inf, inv_den = 0 and xc = 0 for every finite tap: at those pixels the luminance term is as good as
 *    off for this level and the normal and position terms alone stop edges (a tap whose luminance difference is not
 *    finite gives 0 * inf = NaN and is skipped).  The +inf travels on in v (and becomes NaN where kw * kw underflows
 *    to 0); a NaN g makes X NaN for every tap, so that pixel keeps its own colour through the level ((k * c) / k).  No case
 *    makes a finite colour non-finite.
 * The two kernels are crt_renderer_denoise's two with the variance in the colour rows' fourth lane: the direct one at
 * every stride with CRT_DENOISE_DIRECT_ONLY and at strides >= 32, the tiled one else; the bits are the same.
 * crt_renderer_denoise_history_variance fills the same `denoised` buffer (crt_renderer_resolve_denoised, _read_denoised,
 * _denoised_device_ptr); its stats are crt_renderer_denoise's, and crt_renderer_denoise_iteration_ms reports the estimate
 * kernel in out9[0].  There are no default sigmas and no default min_history (the paper uses sigma_luminance 4 and 4
 * frames).  Before any device work and before anything is allocated, CRT_ERR_INVALID_ARGUMENT: a null handle or options,
 * iterations outside 0..8, a sigma that is NaN or outside [2^-50, 2^50] and not +inf, a min_history that is NaN or outside
 * [1, 2^24], flag bits other than CRT_DENOISE_DIRECT_ONLY, reserved != 0, no history, a history without valid moments;
 * CRT_ERR_UNSUPPORTED: a pixel shard other than (0, 1).  crt_renderer_reproject_moments refuses what
 * crt_renderer_reproject refuses.  The variance is that of the history's luminance over time: it knows nothing of the
 * two half buffers of crt_renderer_render_adaptive, and the filter does not demodulate albedo.
 * These entries joined ABI version 3 after its first release. */
typedef struct crt_denoise_variance_options {
    int32_t iterations;                 /* 1..8; 0 = 5 */
    float sigma_luminance, sigma_normal, sigma_position;   /* each in [2^-50, 2^50], or +inf = that term off */
    float min_history;                  /* [1, 2^24]: below it the variance is the 7 x 7 spatial estimate */
    uint32_t flags;                     /* CRT_DENOISE_DIRECT_ONLY (bit 31): measurement switch */
    int32_t reserved;
} crt_denoise_variance_options;
int crt_renderer_reproject_moments(crt_renderer* r, const crt_reproject_options* o, float scale, crt_reproject_stats* stats_out, void* stream);
int crt_renderer_read_moments(crt_renderer* r, float* host_out);
int crt_renderer_denoise_history_variance(crt_renderer* r, const crt_denoise_variance_options* o, crt_denoise_stats* stats_out, void* stream);
/* W*H floats: the estimate kernel's v of the last crt_renderer_denoise_history_variance; waits for the device. */
int crt_renderer_read_variance(crt_renderer* r, float* host_out);
/* crt_selftest_reproject with prev_moments (W*H*2; it may be NULL only with a NULL prev_history) and out_moments (W*H*2). */
int crt_selftest_reproject_moments(crt_renderer* r, const float* color, const float* guides, const float* prev_guides,
                                   const float* prev_history, const float* prev_moments, const crt_camera_desc* prev_camera,
                                   const crt_reproject_options* options, float* out_history, float* out_moments);
/* Self-test of the estimate and the filter: uploads history (W*H*4), moments (W*H*2) and guides (W*H*8) into the
 * renderer's buffers, runs the host function crt_renderer_denoise_history_variance calls on the null stream and reads the
 * result into out (W*H*3) and the estimate's v into out_variance (W*H).  The uploaded history has no previous frame: a
 * reprojection after this starts over. */
int crt_selftest_denoise_variance(crt_renderer* r, const float* history, const float* moments, const float* guides,
                                  const crt_denoise_variance_options* options, float* out, float* out_variance);
/* Host only, no GPU (like crt_scene_export_identity): the per-material rows the step kernel reads, n_materials x 8
 * floats = (code, 0, 0, 0) (payload): code (int bits) 0 lambertian, 1 metal, 2 dielectric, 3 light, 4 unknown type
 * (emits 0); payload (albedo.xyz, 0), (albedo.xyz, min(roughness, 1)), (ior, 1 / ior, r0(1 / ior), r0(ior)) with
 * Schlick's r0(ri) = ((1 - ri) / (1 + ri))^2, (emission.xyz, 0), zeros -- the payloads of the render kernels' shading
 * records, from the same host function.  out == NULL: only *n_materials is set. */
int crt_scene_export_shade_rows(const crt_scene_desc* desc, float* out, int64_t* n_materials);
/* Debugging aid, no GPU needed: the device and pinned-host buffers the library holds in this process right now, over all
 * handles and devices, and their bytes.  Equal values before and after a sequence of calls that ends with its handles
 * destroyed mean the sequence released what it allocated, whatever other processes do on the device. */
int crt_debug_live_allocations(int64_t* buffers, int64_t* bytes);

/* ---- renderer (CUDARenderer) ----
 * Streams: every entry that takes `stream` enqueues all its device work on that stream (NULL = the null stream), a
 * non-blocking stream included, and nothing on any other.  Unless its comment says that it waits, an entry only
 * enqueues and returns; the first use of a path on a handle may allocate.  DESIGN.md section 5d lists which entries
 * wait on the host and why. */
/* Returns after the handle's buffers have been initialised on the device: its first call may come on any stream. */
int  crt_renderer_create(int width, int height, int device, crt_renderer** out);
void crt_renderer_destroy(crt_renderer* r);
/* curand_init(seed, subsequence_base + y*width + x, 0) per pixel (CUDAKernels.h:18-26).
 * subsequence_base = shard * width * height for spp sharding.  Asynchronous, except that the first call on a handle that
 * computes a state waits for the stream once (it allocates the cache of the initialised state); a repeated
 * (seed, base) is a device copy of that cache. */
int  crt_renderer_init_rand(crt_renderer* r, unsigned long long seed, unsigned long long subsequence_base, void* stream);
/* CRT_ERR_INVALID_ARGUMENT for a non-finite origin or lens radius, or |origin| >= 2^59 / lens_radius >= 2^58 (the
 * rebuilt tree's slab test needs |o| * 2^64 finite; every real scene is many orders of magnitude inside it). */
int  crt_renderer_set_camera(crt_renderer* r, const crt_camera_desc* cam);
/* Render-kernel variant (identical results, different wave scheduling).  Scenes with threaded binary nodes
 * (CRT_BVH_REFERENCE, or REBUILT width 2): 0 = per-lane BVH traversal with per-lane leaf loops; 1 = per-lane
 * traversal with wave-cooperative leaf intersection; 2 = 1 + traversal-step scheduling with parked-lane regeneration
 * (lanes start their next ray without waiting for the wave's slowest trace); 3 = 2 + next-node prefetch overlapping
 * the leaf rounds; 10 = 3 with one wave per workgroup over 8x8 tiles in cost-probe order; anything else = automatic:
 * 10 when the render runs the cost probe (spp >= its minimum), else 3.  Scenes with 4-wide nodes (CRT_BVH_REBUILT,
 * width 4): 4 = the variant-3 scheduling over 4-wide nodes with a per-lane stack, 16x16-pixel workgroups; 7 = 4 with a
 * persistent grid whose lanes take pixels from a global queue (no lane waits for its wave's slowest pixel); 8 = 4 with
 * one wave per workgroup over 8x8 tiles in cost-probe order (crt_renderer_set_schedule); anything else = automatic: 8
 * when the render runs the cost probe, else 7.  Accepted values: -1 (automatic, the default), 0-4, 7, 8, 10. */
int  crt_renderer_set_kernel_variant(crt_renderer* r, int variant);
/* Work order of variants 7 and 8 (4-wide scenes).  Cost probe: before the render, variant 4 traces probe_spp samples
 * per pixel over the same RNG state without writing anything, and the per-pixel work estimates order the work
 * most-expensive-first (variant 7: pixels handed to lanes from a global queue; variant 8: 8x8 tiles, one wave per
 * workgroup).  Renders with fewer than min_spp samples per pixel skip the probe.  flags bits 16-19: variant 8's tile
 * key (0 = slowest pixel, 1 = slowest + mean pixel, 2 = 0 raised to 3/4 of the neighbours'; the renderer starts with
 * 2, the measured best); bits 20-23: variant 8's probe stride (1 = every pixel, 2 or 4 = every 2nd / 4th pixel in x and
 * y, 1/4 or 1/16 of the probe's work; 0 = automatic: 2 below 1000 spp, else 1); other bits are ignored.
 * Default -1 (automatic: 4 probe samples for renders of >= 1000 spp, else 2), 64, 2 << 16; probe_spp 0 disables the
 * probe.  Results never depend on the order. */
int  crt_renderer_set_schedule(crt_renderer* r, int probe_spp, int min_spp, int flags);
/* Variants 2-4, 7, 8: number of parked lanes (1..64) that triggers a shading/regeneration pass; default 24 for
 * variants 2/3 and 44 for the 4-wide variants (setting it sets both). */
int  crt_renderer_set_regen_threshold(crt_renderer* r, int lanes);
/* Variant 8 with the cost probe: the first `tiles` tiles of the cost order (the most expensive; -1 = automatic, 4 per
 * CU, the default) trigger their shading/regeneration passes at `lanes` parked lanes (default 16) instead of the
 * regeneration threshold.  A frame with few tiles per wave slot ends with its most expensive tile, whose pixels' sample
 * chains are sequential; waiting less for the wave's other lanes shortens that chain.  Results never depend on it. */
int  crt_renderer_set_critical_tiles(crt_renderer* r, int tiles, int lanes);
/* 4-wide variants (4, 7, 8): a new ray's first `levels` node steps -- the root's, then the one of the internal child it
 * continues to -- run in the regeneration pass from a copy of those nodes in LDS instead of in traversal steps that
 * load them through L1/L2 (-1 = the compiled default, 1; at most the compiled CRT_TOP_LEVELS).  The box tests, their
 * order and the stack entries are the traversal's own, so results never depend on it (a ray whose step hits a leaf
 * child takes that node through the regular step). */
int  crt_renderer_set_top_levels(crt_renderer* r, int levels);
/* Variant 8's leaf-pair carry, a round-4 experiment that was measured and removed (DESIGN.md §8,
 * profiles/r04c/leaf_carry.patch).  Kept for ABI stability: returns CRT_ERR_UNSUPPORTED. */
int  crt_renderer_set_leaf_carry(crt_renderer* r, int lanes, int max_pairs);
/* Variant 7 without the cost probe (the interactive loop's 1-spp frames): 1 = dispatch its 8x8 tiles most expensive
 * first by the rays per pixel the previous variant-7 render of this renderer counted (consecutive frames share the cost
 * map; the first frame, and any after this call, use row order); 0 = row order (default for the renderer; the
 * CRT::Raytracer loop turns it on).  Results never depend on it. */
int  crt_renderer_set_temporal_order(crt_renderer* r, int on);
/* Variant 7 (frames below 64 spp): once its pixel queue is empty, a wave only drains, and its last paths' passes run
 * at `lanes` parked lanes (1..64) instead of the regeneration threshold, so they wait less for each other; 0 = the
 * regeneration threshold (the default).  Results never depend on it. */
int  crt_renderer_set_drain_threshold(crt_renderer* r, int lanes);
/* Variants 4 and 8: once fewer than the regeneration threshold of a wave's lanes still have samples, a shading pass
 * runs when `sixty_fourths`/64 of those live lanes are parked (1..64; 64 = only when all of them are; default 48), so
 * the wave's last pixels wait less for each other's paths.  Results never depend on it. */
int  crt_renderer_set_wave_drain(crt_renderer* r, int sixty_fourths);
/* Variant 8 with the cost probe: 1 = the blocks that share an XCD (block index mod 8, MI355X's round-robin dispatch)
 * render one screen strip of equal probe cost, most expensive tile first, so each XCD's L2 holds its strip's geometry;
 * 0 = one global cost order (default).  Ignored with pixel sharding.  Results never depend on it. */
int  crt_renderer_set_xcd_regions(crt_renderer* r, int on);
/* Pixel sharding, the bit-exact multi-GPU mode: renders of this renderer draw only shard `shard` of
 * `shards` -- the 8x8 tiles whose row-order index t has t % shards == shard, dispatched most expensive first when the
 * cost probe runs (row order without it) -- with all samples, and leave every other pixel of the linear framebuffer
 * at 0.  Summing the shards' framebuffers (the same reduce as spp
 * sharding, every rank with subsequence base 0) gives the unsharded frame bit for bit.  4-wide rebuilt scenes only
 * (variant 8); no CRT_RENDER_ACCUMULATE.  (0, 1) = unsharded, the default. */
int  crt_renderer_set_pixel_shard(crt_renderer* r, int shard, int shards);
/* Variant 4: per-lane traversal-stack entries kept in LDS (1..16, default 16); deeper entries spill to a
 * per-pixel region in HBM.  Results do not depend on it (tests force the HBM path with 1). */
int  crt_renderer_set_stack_lds(crt_renderer* r, int entries);
/* Register-allocation occupancy target in waves per SIMD (1 = compiler default, 4-8; 0 = auto, the default: 7 for
 * variant 8 when the frame has at least 4 of its 8x8 tiles per wave slot; below that, 4 when the cost probe finds the
 * frame chain-bound (its largest tile work over the mean work per occupancy-6 wave slot above 1.6; the host then waits
 * for the probe and the tile sort before launching the main kernel) and 6 otherwise; 6 for the other 4-wide launches
 * and for variants 3 and 10, 5 for variants 0-2).  Variant 8 at 4 loads each lane's next node rows during the leaf
 * round (crt_render_kernel<false, 8, 4>).  The 4-wide kernels keep 16 traversal-stack entries per lane in LDS at 4-5
 * waves, 12 at 6 and 8 at 7+ (LDS is allocated in 1-KiB steps per workgroup). */
int  crt_renderer_set_occupancy_target(crt_renderer* r, int waves_per_simd);
/* Trace `spp` samples per pixel continuing each pixel's RNG stream; the per-pixel
 * linear sum (pixel_color, CUDAKernels.h:157-162) is kept in an fp32 W*H*3 buffer.  Asynchronous, except that it waits
 * for the stream once where it allocates (the first use of variants 7, 8 and 10 on a handle, the first variant-7 frame
 * with the temporal order, a grown overflow stack), and for the probe and the tile sort where variant 8's automatic
 * occupancy reads the probe's statistics (crt_renderer_set_occupancy_target). */
int  crt_renderer_render(crt_renderer* r, const crt_scene* scene, int spp, int max_bounces, unsigned flags, void* stream);
/* RGBA8 = writeColor(scale * sum) (CRTUtility.cuh:14-32); row 0 is the bottom row.  Asynchronous, as are
 * crt_renderer_resolve_adaptive, crt_renderer_resolve_denoised and crt_renderer_resolve_history. */
int  crt_renderer_resolve(crt_renderer* r, float scale, void* stream);
/* The reference's CUDARenderer::render: fresh sum, camera spp, 20 bounces, resolve, synchronize.  Synchronous. */
int  crt_renderer_render_frame(crt_renderer* r, const crt_scene* scene, void* stream);
/* Waits for `stream`, then reports the device error word of the renders before it (CRT_ERR_HIP) and clears it. */
int  crt_renderer_synchronize(crt_renderer* r, void* stream);
int  crt_renderer_read_linear(crt_renderer* r, float* host_out);        /* W*H*3 floats */
int  crt_renderer_read_rgba8(crt_renderer* r, uint8_t* host_out);        /* W*H*4 bytes */
int  crt_renderer_read_rng(crt_renderer* r, uint32_t* host_out);         /* W*H*6 words: v[5], d */
int  crt_renderer_write_linear(crt_renderer* r, const float* host_in);  /* e.g. after a host-side reduce */
int  crt_renderer_get_counters(crt_renderer* r, crt_work_counters* out);/* of the last render call */
/* Scheduling diagnostics of the last CRT_RENDER_COUNT_WORK render (kernel variant 1), read by
 * crt_renderer_get_counters: [0] lane-slots of traversal steps (compare box_tests), [1] lane-slots
 * of cooperative leaf rounds (compare tri_tests), [2] wave-level trace calls. */
int  crt_renderer_get_schedule_stats(crt_renderer* r, unsigned long long* out3);
/* Section profile of the last counting render (variant 4), summed over waves, shader-clock cycles:
 * {shading/regeneration passes, traversal steps (box tests + stack), leaf rounds, passes, waves,
 *  shade() inside the passes, next_ray() inside the passes}. */
int  crt_renderer_get_section_profile(crt_renderer* r, unsigned long long* out7);
/* The same plus word 7: ray_spheres() inside the passes (part of word 5); copies min(n, 8) words. */
int  crt_renderer_get_section_profile_ex(crt_renderer* r, unsigned long long* out, int n);
float* crt_renderer_linear_device_ptr(crt_renderer* r);   /* for RCCL reduce of the framebuffer */
/* Bind the linear-sum framebuffer to caller-owned device memory of W*H*3 floats on the renderer's
 * device (e.g. a tensor the caller all-reduces with RCCL); NULL re-binds the internal buffer. */
int crt_renderer_attach_linear(crt_renderer* r, float* device_ptr);
uint8_t* crt_renderer_rgba_device_ptr(crt_renderer* r);
uint32_t* crt_renderer_rng_device_ptr(crt_renderer* r);
/* Milliseconds of the last render kernel launch(es), measured with HIP events on the launch stream. */
float crt_renderer_last_kernel_ms(crt_renderer* r);
/* The occupancy choice of the last variant-8 render: out[0] = rho, the probe's largest tile work over the mean work per
 * occupancy-6 wave slot (0 when the choice did not use the probe), out[1] = the occupancy launched (waves per SIMD; 0
 * for other variants), out[2] = the largest tile work and out[3] = the mean tile work (probe cost units).  An
 * extension of this port (the reference has one kernel shape), like crt_renderer_last_timings. */
int crt_renderer_last_schedule(crt_renderer* r, float out[4]);
/* HIP-event times of the last render, in ms: out[0] = the whole render (== crt_renderer_last_kernel_ms), out[1] = what
 * runs before the main render kernel (variant 8 / 7: the cost probe and the tile sort; 0 otherwise), out[2] = the main
 * render kernel alone. */
int crt_renderer_last_timings(crt_renderer* r, float out[3]);
/* The same three times for an earlier render: back = 0 is the last render, 1 the one before, up to
 * CRT_TIMING_RING - 1.  A caller that enqueues K frames without synchronising reads every frame's main-kernel time
 * afterwards (bench.py averages them for the roofline).  CRT_ERR_INVALID_ARGUMENT when fewer renders exist. */
#define CRT_TIMING_RING 32
int crt_renderer_timing_history(crt_renderer* r, int back, float out[3]);
/* Template instantiation of the last render-kernel launch as rocprofv3 names it, e.g.
 * "crt_render_kernel<false, 4, 6>" (empty before the first launch and for variant 5). */
const char* crt_renderer_last_kernel_name(const crt_renderer* r);
/* Which twin of that kernel the last render launched.  The plain variant-8 kernels ("crt_render_kernel<false, 8, W>")
 * exist twice under that one name: a frozen twin, in which the knobs of a default launch are compile-time constants
 * (every LDS stack entry of W in use, the LDS root step, no spheres in the tree, two per-ray spheres, one layout, no
 * probe, the default wave_drain and regeneration threshold), and an open twin that reads them per launch.  The
 * library picks per launch; both give the same bits for the same inputs.  1 = the frozen twin ran; 0 = the open twin,
 * any other kernel, no launch yet, or r == NULL.  Added within ABI 3: a caller that may load an older library looks
 * the symbol up first. */
int crt_renderer_last_launch_frozen(const crt_renderer* r);
/* Tail fill of a variant-8 launch (one 8x8 tile per one-wave workgroup, most expensive first).  Such a launch ends
 * with a drain: the last tiles leave most wave slots empty, and the smallest item is a whole tile's samples.  With
 * tail fill the heads of the first `tiles` tiles of the cost order render all but their last `spp` samples, and those
 * samples follow the launch's tiles as small items: each continues its pixels from the stored sums and RNG state,
 * every pixel on one lane and its samples in order, as a render with CRT_RENDER_ACCUMULATE continues a frame.  No
 * workgroup waits for another: a part that finds its tile's head unfinished is rendered by a second, short launch.
 * tiles < 0: automatic (the default): on where variant 8 runs with the cost probe at the automatically chosen
 * occupancy 7, unsharded and not counting, and the held-back samples reach a floor; off elsewhere.  tiles == 0: off.
 * tiles > 0: the first `tiles` tiles (clamped to the tile count) hold back `spp` samples in every plain variant-8
 * render on one shard; a render for which `spp` is not within 1 .. its samples - 1 runs without it.
 * Results never depend on it.  Added within ABI 3: a caller that may load an older library looks the symbol up first. */
int crt_renderer_set_tail_fill(crt_renderer* r, int tiles, int spp);
/* The last render's tail fill: out = {tiles, held-back samples, parts rendered inside the main launch, parts rendered
 * by the sweep launch after it}; the two counts add up to tiles.  All 0 when it rendered without tail fill.  Waits for
 * that render to end.  Results never depend on it.  Added within ABI 3 (looked up like the setter). */
int crt_renderer_last_tail_fill(crt_renderer* r, int out[4]);

/* ---- GPU-parallel mesh BVH build (replaces Mesh::buildBVHMesh <<<1,1>>>, Mesh.cuh:121-264, and the Mesh ctor
 * box, Mesh.cuh:39-47; launched by initMesh, CUDAKernels.h:28-33) ----
 * Same node array (reference allocation order, crt_bvh_node_desc as the host builder emits it) and the same
 * in-place permutation of indices / face_materials (swap_triplet, Core.cuh:25-39) as the reference's single-thread
 * builder, computed level-parallel on `device` (see csrc/crt_bvh_build.hip).  positions: vertex_count slots (xyz);
 * indices: index_count local indices (multiple of 3), permuted in place; nodes: capacity 2*(index_count/3) - 1;
 * mesh_box: min xyz, max xyz.  build_ms (optional): device time from the first upload to the last kernel.
 * Returns CRT_ERR_UNSUPPORTED (nothing written) for meshes where the reference's node cap decides the tree (a split
 * with an empty side) or index_count % 3 != 0: the caller uses the sequential host builder then.  Box bounds may
 * differ from a sequential build in the sign of a zero only. */
int crt_build_mesh_bvh(int device, const float* positions, uint32_t vertex_count, uint32_t* indices,
                       int32_t* face_materials, uint32_t index_count, crt_bvh_node_desc* nodes, int32_t* node_count,
                       float mesh_box[6], float* build_ms);

/* ---- self-test of the arithmetic the kernel depends on (IEEE f32/f64 div/sqrt) ---- */
/* For n inputs a[i], b[i] (f32) computes on the device: a/b, sqrtf(|a|), 1/a, (double)sqrt((double)|a|)
 * into out[4*i..4*i+3] (the last one converted to float bits as a double->float cast). */
int crt_selftest_math(const float* a, const float* b, int n, float* out, double* out_f64);
/* Exhaustive reciprocal self-test: counts floats x with bit patterns in [lo_bits, hi_bits) (and -x) for which
 * the kernel's fast reciprocal (v_rcp_f32 + FMA Newton step) differs from IEEE 1.f/x; first_bad = lowest such. */
int crt_selftest_rcp(uint32_t lo_bits, uint32_t hi_bits, unsigned long long* mismatches, uint32_t* first_bad);
/* Exhaustive square-root self-test: counts floats x with bit patterns in [lo_bits, hi_bits) for which the kernels'
 * fast square root (v_rsq_f32 + one FMA correction step, crt_device.h::sqrt_rsq) differs from the correctly rounded
 * sqrtf; first_bad = lowest such. */
int crt_selftest_sqrt(uint32_t lo_bits, uint32_t hi_bits, unsigned long long* mismatches, uint32_t* first_bad);
/* Vec3::unit as the shading pass runs it, one call for all lanes of a wave: in = n x 3 floats, 64 consecutive vectors
 * share a wave (and with it the wave-uniform choice between the fast and the IEEE square root and reciprocal);
 * out[3*i..] = (1 / sqrt(x*x + y*y + z*z)) * v, every operation correctly rounded f32. */
int crt_selftest_unit(const float* in, int n, float* out);
/* Exhaustive check of next_ray's image-coordinate division for one frame dimension (width or height): counts the
 * floats a in [2^-33, dim] (every value x + U can take) for which uv_div(a, dim, RN(1/dim)) differs from IEEE a / dim.
 * crt_renderer_create runs the same check and uses uv_div only when both dimensions have none. */
int crt_selftest_uv_div(int dim, unsigned long long* mismatches);
/* Wave64 scan self-test: for n_waves x 64 ints, out[3*i..] = DPP inclusive sum, ds_bpermute inclusive sum,
 * DPP inclusive max (per wave of 64 consecutive entries). */
int crt_selftest_scan(const int* in, int n_waves, int* out);
/* Known-answer self-test of the render path's primitive functions on the device (tests/golden/primitives.json).
 * kind 0: Möller–Trumbore (Mesh.cuh:266-308), in 17 floats per record (o3 d3 v0 v1 v2 tmin tmax; tmin is 0.001 in
 *         the render path), out t or -1;
 * kind 1: AABB::hit (AABB.cuh:123-146) against [0.001, inf), in 14 floats (o3 d3 lo3 hi3 tmin tmax), out 1 / 0;
 * kind 2: Sphere::hit (Sphere.cuh:27-47), in 12 floats (o3 d3 center3 radius tmin tmax), out t or -1;
 * kind 3: Camera::getRay (Camera.cuh:32-44), in 2 ints per pixel (x, y) of a width x height image, rng 6 words per
 *         pixel (continued in place), out o3 d3;
 * kind 4: the per-ray spheres' skip test (a root provably beyond the trace's closest hit), in 12 floats (o3 d3
 *         center3 radius closest unused), out 1 = skipped / 0 = tested exactly. */
int crt_selftest_geometry(int kind, const float* in, int n, const crt_camera_desc* cam, int width, int height,
                          uint32_t* rng, float* out);
/* Known-answer self-test of the render kernels' material step (tests/golden/scatter_kat.npz): per record shade_rec()
 * on a hand-made shading record, then next_ray() with no samples left (the bounce limit and the roulette of the bounce
 * that follows).  Blocks of 64 lanes: records 64 k .. 64 k + 63 share a wave.
 * in : 32 words per record: o3 d3 t hit | outward normal3, SHADE_* code | payload4 (crt_scene_export_shade_rows) |
 *      throughput3 bounce | max_bounces rng6 (hit, the code, bounce and max_bounces are integers; hit 0 = a miss).
 *      The face is dot(d, normal) < 0, as the render kernels take it.
 * out: 20 words per record: ended | o3 d3 | throughput3 | bounce | what the path added to its pixel | rng6. */
int crt_selftest_shade(const float* in, int n, float* out);
/* XORWOW device self-test: init(seed, subseq[i]) then n_draw uniforms per entry. */
int crt_selftest_rng(unsigned long long seed, const unsigned long long* subseq, int n, int n_draw,
                     uint32_t* state_out /* n*6 */, float* uniforms_out /* n*n_draw */);
/* Self-tests of the tile and pixel schedules (variants 7, 8, 10): the stages between a cost probe and the main kernel on
 * caller-supplied costs, run by the host functions the renders call, in the renderer's own buffers (so their sizes, the
 * scratch reuse and the guards are the renders').  No camera or scene is needed.  Synchronous; the results stay in the
 * renderer's buffers and are read with crt_selftest_schedule_buffer.  The order buffer is filled with 0xffffffff
 * first, so entries a stage did not write still hold that.  These entries joined ABI version 3 after its first release.
 * Variant 8 / 10's tile schedule: pix_cost = width * height costs as a probe of `stride` (1, 2, 4) leaves them (only
 * pixels with x, y % stride == 0 are read), key_mode 0..2 as crt_renderer_set_schedule's tile key, (shard, shards) as
 * crt_renderer_set_pixel_shard, xcd_regions as crt_renderer_set_xcd_regions; the renderer's own settings are kept.
 * Afterwards buffer 1 holds the tile keys as sorted (after the neighbour and shard steps) and buffer 0's first
 * tiles_x * tiles_y entries the tile order.  stats_out (optional): the two words of the probe statistics, the largest
 * tile work and the total work. */
int crt_selftest_tile_schedule(crt_renderer* r, const uint32_t* pix_cost, int stride, int key_mode, int shard, int shards,
                               int xcd_regions, unsigned long long* stats_out);
/* Variant 7's orders into buffer 0.  kind 0: the probe order, the pixels most expensive first by in = width * height
 * per-pixel costs (width * height entries).  kind 1: the temporal order from in = a rays-per-pixel map (uploaded as the
 * last frame's; the renderer's next frame starts in row order again): buffer 4 = the tiles most expensive first, buffer 1
 * their keys, buffer 0 = tiles * 64 pixel slots.  kind 2: the row-order slots.  kind 3: pixel sharding without the
 * probe, entry k = the k-th tile of (shard, shards).  in is ignored for kinds 2 and 3, the shard for kinds 0..2. */
int crt_selftest_pixel_order(crt_renderer* r, int kind, const uint32_t* in, int shard, int shards);
/* Reads a schedule buffer of the renderer, whole: which 0 = the order (max(width * height, tiles * 64) words), 1 = the
 * tile keys (tiles), 2 = the per-pixel probe costs (width * height; the sort scratch after a tile schedule), 3 = the
 * rays per pixel of the last temporal variant-7 frame (width * height), 4 = the temporal tile order (tiles).  *n = the
 * buffer's words, 0 while it is not allocated; min(*n, capacity) words are copied to out.  Waits for the device. */
int crt_selftest_schedule_buffer(crt_renderer* r, int which, uint32_t* out, int64_t capacity, int64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* CRT_HIP_H */
