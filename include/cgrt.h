/* cgrt.h -- C-ABI of the MI355X-native BVH traversal + ray/triangle path.
 *
 * The reference (mgokbulut/CG-RayTracer) has no FFI / plugin layer: its hot path is the C++ class
 * BoundingVolumeHierarchy (src/bounding_volume_hierarchy.h:15-56) plus the free functions of
 * src/ray_tracing.h:10-20, called one ray at a time from src/main.cpp:115,182,276.  This header is
 * the boundary a maintainer would bind instead; every entry names the reference
 * interface it replaces.  Plain C types only, caller-allocated outputs, no exceptions cross it.
 *
 * Every function that returns int returns 0 on success and a negative CGRT_E_* code on failure;
 * cgrt_last_error() then describes the failure (thread-local string).  There is NO CPU fallback:
 * without a usable HIP device cgrt_scene_create fails with CGRT_E_NO_DEVICE.
 *
 * Threads.  The reference calls BoundingVolumeHierarchy::intersect on one const object from an `omp parallel for`
 * (main.cpp:653-656), so:
 *   - cgrt_intersect_batch, cgrt_trace_primary, cgrt_generate_rays, cgrt_count_* (host pointers) may be called
 *     concurrently on ONE scene from any number of threads: each call runs on a private stream with private device
 *     scratch and pinned staging taken from a per-scene pool and waits for that stream only (no hipMalloc / hipFree /
 *     hipDeviceSynchronize once the pool has grown to the call sizes in use); cgrt_intersect_batch calls of at most 64 rays --
 *     BoundingVolumeHierarchy::intersect, one ray per call -- are COMBINED: concurrent callers append their rays to a shared
 *     pinned ring, one of them launches one kernel for all of them and everybody copies its own hits out (cgrt_set_call_combining);
 *   - the *_device entries only enqueue work on the caller's stream: concurrent too.  (cgrt_trace_primary_device keeps one piece of
 *     per-scene state, the frame hints -- see cgrt_set_frame_hints: a short mutex while the launch is issued, and launches that
 *     arrive on changing streams simply run without hints;)
 *   - cgrt_render* use one per-scene workspace: calls on the same scene are serialised by a mutex inside the library;
 *   - cgrt_set_* are process-wide options (mutex / atomic inside); cgrt_scene_set_walk and cgrt_scene_destroy must not
 *     race with calls on that scene.
 */
#ifndef CGRT_H
#define CGRT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CGRT_OK 0
#define CGRT_E_ARG (-1)       /* bad argument (null pointer, inconsistent counts, index out of range) */
#define CGRT_E_NO_DEVICE (-2) /* no HIP device / device index out of range */
#define CGRT_E_HIP (-3)       /* a HIP runtime call failed */
#define CGRT_E_ALLOC (-4)     /* host or device allocation failed */
#define CGRT_E_LIMIT (-5)     /* scene exceeds a structural limit (BVH deeper than 12 levels) */

#define CGRT_NO_PRIM 0xffffffffu
#define CGRT_DEVICE_NONE (-1) /* cgrt_scene_create: build on the host only, no device upload */

/* Ray: bit-compatible with the reference's `Ray` (framework/include/ray.h:9-13): 28 bytes. */
typedef struct CgrtRay {
    float origin[3];
    float direction[3];
    float t; /* in: current closest t (FLT_MAX for a fresh ray) */
} CgrtRay;

/* Result of BoundingVolumeHierarchy::intersect for one ray (bounding_volume_hierarchy.cpp:850-881).
 *   t           final ray.t (unchanged input t on a miss)
 *   prim_id     last accepted primitive: global triangle index (prefix over Scene::meshes in load
 *               order + index in Mesh::triangles), or ntris + sphere index; CGRT_NO_PRIM on a miss.
 *               The reference has no primitive id (HitInfo = normal + material, ray_tracing.h:4-8);
 *               this is the definition of SURVEY.md section 8(c).
 *   material_id index of the mesh whose Material the reference copies into hitInfo.material
 *               (bvh.cpp:547), -1 if never written (miss, or sphere-only hit: bvh.cpp:878-879).
 *   hit         the bool the reference returns. */
typedef struct CgrtHit {
    float t;
    uint32_t prim_id;
    int32_t material_id;
    uint32_t hit;
} CgrtHit;

/* Trackball camera state (framework/include/trackball.h:48-56; defaults src/main.cpp:730-731). */
typedef struct CgrtCamera {
    float look_at[3];
    float euler[3]; /* radians */
    float distance;
    float fovy;   /* radians, vertical */
    float aspect; /* Window::aspectRatio(), framework/src/window.cpp:334-337 */
} CgrtCamera;

/* Totals of the traversal work for a batch (SURVEY.md section 8(d) algorithmic-bytes definition). */
typedef struct CgrtCounters {
    uint64_t rays;
    uint64_t inner_visits; /* reference inner nodes visited (intersectNonLeaf calls, bvh.cpp:715) */
    uint64_t leaf_visits;  /* reference leaves visited (intersectLeaf calls, bvh.cpp:535) */
    uint64_t tri_tests;    /* triangle records tested on the device */
    uint64_t sub_visits;   /* 4-wide nodes visited: in-leaf accelerators (exact walk) and the fast tree (certified walk) */
    uint64_t cert_boxes;   /* certified walk: path boxes tested by certificates (24 B each) */
    uint64_t fallback_rays; /* certified walk: rays that got no certificate and took the exact walk afterwards */
    uint64_t tree_rays;    /* rays that passed the root gate (intersectDataStructure, bvh.cpp:835-836) and walked the tree */
} CgrtCounters;

typedef struct CgrtScene CgrtScene;

/* Replaces BoundingVolumeHierarchy::BoundingVolumeHierarchy(Scene*) (bvh.cpp:42-76): builds the
 * reference's 12-level median-split tree on the host (same topology, same leaf order), flattens it
 * and uploads it to `device`.  With device == CGRT_DEVICE_NONE nothing is uploaded: the tree can be
 * inspected (cgrt_num_levels, cgrt_get_nodes, cgrt_leaf_prims) but every trace/intersect entry fails with
 * CGRT_E_NO_DEVICE.
 *   pos_nrm   nverts x 6 floats (Vertex{p, n}, mesh.h:12-15), all meshes concatenated
 *   tri       ntris x 3 indices into pos_nrm, meshes concatenated in load order
 *   tri_mesh  ntris mesh indices, non-decreasing
 *   materials nmesh x 8 floats (Material{kd, ks, shininess, transparency}, mesh.h:17-23)
 *   spheres   nspheres x 5 floats {center, radius, material index or -1} (scene.h:36-40), may be NULL */
int cgrt_scene_create(const float* pos_nrm, uint32_t nverts, const uint32_t* tri, const uint32_t* tri_mesh,
                      uint32_t ntris, const float* materials, uint32_t nmesh, const float* spheres,
                      uint32_t nspheres, int device, CgrtScene** out);
void cgrt_scene_destroy(CgrtScene* scene);

/* In-leaf accelerator (no counterpart upstream; DESIGN.md "In-leaf accelerator").  The reference scans
 * a leaf's triangles linearly (bvh.cpp:535-553, ~390 per leaf at 800 K triangles).  By default every
 * scene also gets, per reference leaf, a small BVH that lets the kernel skip triangles the ray cannot
 * hit; results are identical with it on or off (that is tested), only the work differs.  Process-wide,
 * applies to scenes created afterwards.  sub_leaf_tris: triangles per accelerator leaf, 0 = default (4). */
int cgrt_set_leaf_accel(int enabled, int sub_leaf_tris);
int cgrt_num_subnodes(const CgrtScene* scene);
/* Scheduling of the fused primary-frame kernel (results are identical; tested): 0 = one wave per 8x8 tile,
 * 1 = persistent waves that pull tiles from per-XCD queues and refill finished lanes.  Process-wide. */
int cgrt_set_primary_mode(int mode);
/* Kernel shape of the certified walk, chosen per launch (no counterpart upstream; DESIGN.md "Latency shapes"; results are
 * identical, tested).  A launch ends when its hardest rays end, and a hard ray's dependent chain runs ~2x faster when it does not
 * share its wave with 63 others, so SHORT RAY LISTS are laid out sparsely:
 *   mode -1 (default) by size: lists of at most 8192 rays -> 4 rays per wave, 16 lanes per ray (four stack entries x four child
 *            boxes per round); of at most max_rays (default 131072) -> one ray per lane, 16 rays per single-wave workgroup (the wave
 *            is in the quad tail, four lanes per ray, from its first step); larger lists and every frame: 64 rays per wave.
 *            Lists sized on the device (cgrt_render's wavefront) choose between 16 and 64 per wave on the device.
 *   mode 0 = 64 rays per wave always (round 2's behaviour), 1 = quad per ray with 16 rays per wave (frames too), 2 = 16 rays per
 *            wave for every list, 3 = 4 rays per wave for every list: for tests and measurements.
 * max_rays = 0 keeps the current threshold.  Process-wide. */
int cgrt_set_kernel_shape(int mode, uint64_t max_rays);
int cgrt_get_kernel_shape(int* mode, uint64_t* max_rays);
/* Frame hints of the primary frame entries (cgrt_trace_primary*, one scene, frames of one shape after another): every wave of a
 * frame measures its own wall time, and the 8x8 tiles whose wave took long are traced differently by the NEXT frame of the same
 * shape -- first (mode 1: the long waves no longer start in the frame's last round) or as four waves of 16 rays (mode 2: for
 * small frames, whose time is the time of their longest wave).  -1 (default) = by frame size (<= 0.8 M rays: 2; a rank's share
 * of <= 1.3 M rays of a frame split over >= 4 ranks: 2; anything else: none -- mode 1 is only ever asked for), 0 = off.  The time from which a wave
 * counts as long starts at 45 us and follows the scene (it rises while more than 2 % of the frame's tiles are listed); a scene
 * whose lists stay empty is traced without hints for 56 of every 64 frames.  Only the order and the layout of the work change: every pixel is traced once, by the same arithmetic
 * (tested bit for bit); the first frames of a shape (hints are set up for a shape that has been traced three times in a row), the
 * instrumented and the multi-device (packed) launches take no hints.  The hint buffers belong to the scene: frames of one scene issued on ONE stream use them; when the caller changes
 * streams the library falls back to unhinted launches for a few frames (the *_device entries stay safe to call from several
 * threads, they are just not accelerated then).  Process-wide. */
int cgrt_set_frame_hints(int mode);
/* Frame order of the primary frame entries (cgrt_trace_primary*): whole frames and large shares -- single-wave
 * workgroups on a fast tree, not packed, no counters, left alone by the frame hints above -- are launched with an ORDER TABLE once one
 * shape has been traced three times in a row on one stream: the third launch also records the longest wave time of every 64x64
 * super-tile, a small kernel behind it deals the super-tiles with long waves to the earliest of the launch positions that heavy
 * super-tiles hold anyway (per blockIdx % 8 lane: XCD placement and the pattern of heavy and background work stay what they are), and
 * the launches after it read that table; the shape is profiled again every 32 launches.  Nothing waits for the host.  Only the order of
 * dispatch changes: every pixel is traced once, by the same arithmetic (tested bit for bit).  Streams and shapes as with the hints: a
 * change means eight launches without a table.  -1 (default) = the library's policy (on), 0 = off, 1 = on wherever a frame qualifies.
 * Process-wide; the CGRT_FRAME_ORDER environment variable overrides it (experiments). */
int cgrt_set_frame_order(int mode);
/* Tests.  cgrt_debug_set_frame_order installs `table` (n = the shape's super-tiles for this rank, padded to 8) for the next launches of
 * that shape on this scene, in place of the policy's profile frames, after a device synchronise; CGRT_E_ARG unless the table is a
 * permutation that keeps every position's % 8 residue and the padded positions and n is that length; table = NULL, n = 0 returns the
 * scene to the policy.  cgrt_debug_get_frame_order: *n = entries of the table in use (0: none) and, when `table` holds at least that
 * many (cap), the table, after a device synchronise; state2 = {0 none / 1 profiled: the builder follows the last launch / 2 active: the
 * last launch read the table, launches since the profile frame}.  cgrt_debug_build_frame_order runs the device builder alone on n
 * injected tick values (10 ns each; 500 and more: live) and returns the (n + 7) / 8 * 8 entries it makes. */
int cgrt_debug_set_frame_order(CgrtScene* scene, int W, int H, int x0, int y0, int x1, int y1, int rank, int nranks, const uint16_t* table, uint32_t n);
int cgrt_debug_get_frame_order(CgrtScene* scene, uint16_t* table, uint32_t cap, uint32_t* n, int* state2);
int cgrt_debug_build_frame_order(const uint32_t* ticks, uint32_t n, uint16_t* out);
/* Frame gate of the camera frames (cgrt_trace_primary*, cgrt_render* with one CgrtCamera): 1 (default) = the host projects the mesh
 * root box onto the screen per launch, and a wave whose pixels all lie outside that rectangle (widened by a margin)
 * writes its miss records without generating rays; 0 = every pixel takes the per-pixel root gate.  Same bytes either way (tested).
 * Scenes with spheres, cameras inside or on the box, a box that reaches behind the camera, launches that carry frame hints (small
 * frames, cgrt_set_frame_hints), ray cameras and multi-view batches are never gated.  Process-wide. */
int cgrt_set_frame_gate(int mode);
/* Diagnostics: the rectangle the host computes for this camera and a W x H frame, out5 = {x0, y0, x1, y1, valid}: with valid == 1
 * every pixel with x < x0, x >= x1, y < y0 or y >= y1 misses the root gate ({0, 0, 0, 0} when every pixel does); valid == 0: no
 * rectangle, the frame is not gated.  Does not depend on cgrt_set_frame_gate.  Works on host-only scenes. */
int cgrt_debug_frame_gate(const CgrtScene* scene, const CgrtCamera* cam, int W, int H, int* out5);
/* Tests: the wall time (s_memrealtime ticks, 100 MHz) from which a 64-ray / a 16-ray wave puts its tile on the hard list; 0 = the
 * default (4500 = 45 us, the floor of the adaptive threshold; a 16-ray wave counts from 5/9 of the threshold in force, the second
 * argument is ignored).  With a few ticks every tile that reaches the tree is "hard" and the lists overflow. */
int cgrt_debug_set_hint_thresholds(unsigned dense_ticks, unsigned sparse_ticks);
/* Diagnostics: the lengths of the scene's three rotating hard lists (synchronises the device). */
int cgrt_debug_hint_counts(CgrtScene* scene, uint32_t* out3);
/* cgrt_render*: 1 (default) = a frame of the same shape (size, rank, depth, light count) as the scene's previous one is issued in one
 * go, its launches sized from what that frame found per level, the counts checked once behind the frame (and the frame drawn again
 * the exact way when a list outgrew its launch); 0 = every frame waits for the device's hit count before it sizes the lists, as the
 * first frame always does.  The pixels are identical (tested); only the host round trips inside the frame differ.  Process-wide. */
int cgrt_set_render_prediction(int enabled);
/* How the scene's last cgrt_render* frame was drawn: 0 = exactly sized, 1 = as predicted, 2 = predicted, a list outgrew its launch,
 * drawn again exactly; -1 for a NULL scene.  (Tests, diagnostics.) */
int cgrt_debug_render_path(const CgrtScene* scene);
/* Certified walk (no counterpart upstream; DESIGN.md "Certified walk").  The exact walk takes every step of the
 * reference's ordered descent (bvh.cpp:572-758) because its culling quirks are part of the result.  A scene may also
 * carry a "fast tree" (a 4-wide tree over the reference LEAVES) and per-leaf box paths: a ray then searches the fast
 * tree with conservative tests, and its answer is kept only if a certificate holds -- unique strict minimum, no
 * origin-on-plane acceptance, and every box the reference tests on its way to that leaf is entered at the final t
 * (the reference's own box arithmetic); any other ray is walked exactly.  Results are identical either way (tested).
 *   cgrt_set_fast_tree: process-wide, for scenes created afterwards: -1 (default) = build it whenever the structures
 *     allow it, except for scenes of fewer than 16 triangles and scenes created with the in-leaf accelerator off;
 *     0 = never; 1 = whenever the structures allow it (finite geometry, tame float planes, every leaf accelerated or small).
 *   cgrt_scene_set_walk: per scene, 1 = certified walk (needs the fast tree: CGRT_E_ARG otherwise), 0 = exact walk only.
 *     Not to be changed while launches of the scene are being issued from other threads.
 *   cgrt_scene_walk: the current setting (1 / 0). */
int cgrt_set_fast_tree(int mode);
int cgrt_scene_set_walk(CgrtScene* scene, int certified);
int cgrt_scene_walk(const CgrtScene* scene);
/* What the host builder decided (also for host-only scenes): out4 = {1 if the fast tree was built, number of reference leaves
 * that hold a triangle whose float plane degenerates (such leaves keep the linear scan and veto the fast tree), 1 if every vertex
 * coordinate is finite, number of reference leaves}. */
int cgrt_scene_build_info(const CgrtScene* scene, uint32_t* out4);

/* BoundingVolumeHierarchy::numLevels() (bvh.cpp:214-224). */
int cgrt_num_levels(const CgrtScene* scene);
/* Tree introspection for builder-parity tests (the reference keeps std::vector<Node>, bvh.h:6-13).
 * meta: nnodes x 5 int32 {is_leaf, level, child0, child1, ntris}; boxes: nnodes x 6 floats. */
int cgrt_num_nodes(const CgrtScene* scene);
int cgrt_get_nodes(const CgrtScene* scene, int32_t* meta, float* boxes);
/* prim ids of leaf `node` in the order intersectLeaf scans them (bvh.cpp:538-551). Returns count. */
int64_t cgrt_leaf_prims(const CgrtScene* scene, int node, uint32_t* out, uint32_t cap);
double cgrt_build_seconds(const CgrtScene* scene);
uint64_t cgrt_device_bytes(const CgrtScene* scene);

/* Batched BoundingVolumeHierarchy::intersect(Ray&, HitInfo&) (bvh.cpp:850-881): n independent rays.
 * normals (optional, n x 3) receives hitInfo.normal for rays that hit (left untouched otherwise, as
 * the reference leaves HitInfo untouched on a miss).  Host pointers; synchronous. */
int cgrt_intersect_batch(CgrtScene* scene, const CgrtRay* rays, uint64_t n, CgrtHit* hits, float* normals);
/* Call combining for small cgrt_intersect_batch calls (see "Threads" above; DESIGN.md "Per-ray boundary"): 1 = on (default),
 * 0 = every call launches for itself (round 2's behaviour).  Results are identical.  Process-wide. */
int cgrt_set_call_combining(int enabled);
/* Diagnostic: out5 = {combined generations launched on this scene, rays in them, rays of the largest one, nanoseconds their
 * leaders spent between closing a generation and holding its results (waiting for the joiners' rays + launch + kernel + stream
 * wait), the part of that up to the return of the launch call}. */
int cgrt_debug_combiner_stats(const CgrtScene* scene, uint64_t* out5);
/* intersectRayWithShape(const Mesh&, Ray&, HitInfo&) (ray_tracing.cpp:202-213) for n rays: every triangle is tested, no
 * tree -- the reference's ground truth over all triangles (its BVH misses hits this loop finds: SURVEY.md F4).
 *   mesh >= 0: that mesh only (index into the scene's meshes); material_id stays -1, the loop never writes hitInfo.material.
 *   mesh <  0: every mesh in load order, then the spheres, material written: the pre-BVH body of
 *              BoundingVolumeHierarchy::intersect (bvh.cpp:854-868, commented out upstream).
 * Same outputs and conventions as cgrt_intersect_batch; O(n * ntris) work: a validation path, not a fast one. */
int cgrt_intersect_brute_batch(CgrtScene* scene, const CgrtRay* rays, uint64_t n, int mesh, CgrtHit* hits, float* normals);
/* Same, all pointers are DEVICE pointers on the scene's device; asynchronous on `stream`
 * (a hipStream_t, NULL = default stream). */
int cgrt_intersect_batch_device(CgrtScene* scene, const CgrtRay* d_rays, uint64_t n, CgrtHit* d_hits,
                                float* d_normals, void* stream);

/* Primary frame: fuses renderRayTracing's ray generation (main.cpp:691-694 + Trackball::generateRay,
 * trackball.cpp:92-103) with intersect; no rays are uploaded.  Pixel (x, y), 0 <= x < W, 0 <= y < H,
 * result index y*W + x (not y-flipped).  The rectangle [x0,x1) x [y0,y1) is cut into 64x64-pixel super-tiles
 * (row-major from (x0, y0)); only pixels whose super-tile index % nranks == rank are traced and written
 * (image tiling across GPUs). */
int cgrt_trace_primary(CgrtScene* scene, const CgrtCamera* cam, int W, int H, int x0, int y0, int x1, int y1,
                       int rank, int nranks, CgrtHit* hits, float* normals);
int cgrt_trace_primary_device(CgrtScene* scene, const CgrtCamera* cam, int W, int H, int x0, int y0, int x1,
                              int y1, int rank, int nranks, CgrtHit* d_hits, float* d_normals, void* stream);
/* The rays the fused kernel generates, written out for "same rays" parity checks (row-major over the
 * rectangle). Host pointer. */
int cgrt_generate_rays(CgrtScene* scene, const CgrtCamera* cam, int W, int H, int x0, int y0, int x1, int y1,
                       CgrtRay* rays);

/* renderRayTracing / getFinalColor (src/main.cpp:298-310, :648-720) for a whole frame, entirely on the device: primary
 * rays, then per recursion level the shadow rays of every hit (pointInShadow, :104-135), the Phong terms (:61-98,
 * :219-232) and the mirror rays (shade, :241-264).  max_level = 2 is the reference (`level >= 2` -> black, :267).
 * lights: nlights x 6 floats {position, color} (PointLight, scene.h:42-45); rgb: W*H*3 floats, index y*W+x, not
 * y-flipped and not clamped (Screen::setPixel / writeBitmapToFile do that, screen.cpp:30-49).  Host pointers. */
/* The scene keeps the device workspace of these calls between frames (about 0.3 KB per pixel at 1920x1080 with one light
 * and max_level 2; it grows with the frame, the lights and the depth) and releases it in cgrt_scene_destroy. */
typedef struct CgrtRenderStats {
    uint64_t primary_rays, shadow_rays, reflection_rays; /* rays that exist upstream */
    int32_t levels;                                      /* recursion levels actually evaluated */
    float device_ms;                                     /* HIP-event time of all kernels of the frame */
    uint64_t soft_shadow_rays;                           /* samples towards spherical lights (cgrt_render_soft) */
} CgrtRenderStats;
int cgrt_render(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, int max_level,
                float* rgb, CgrtRenderStats* stats);

/* The same frame with the spherical lights of `shading` (src/main.cpp:168-218): per hit and light, `samples` shadow rays
 * (200 upstream, :176) towards position + radius * randomUnitVector(); the light's diffuse and specular terms are scaled
 * by the fraction that reaches it (!intersect || ray.t > lightT, :183-199); spherical lights are accumulated before the
 * point lights (:168, :219).  Upstream draws randomUnitVector() from std::random_device (:46-59), which cannot be
 * reproduced by anyone; here the draws are DATA: `unit_vectors` holds nunits x 3 floats (normalised gaussian triples
 * give upstream's distribution) and sample `smp` of spherical light `l` at pixel p = y*W+x, recursion level `lv`, uses
 * entry  mix(mix(mix(mix(seed ^ 0x9e3779b9) ^ p) ^ (lv * 0x01000193 + l)) ^ smp) % nunits,  mix = murmur3's 32-bit
 * finaliser (h ^= h>>16; h *= 0x85ebca6b; h ^= h>>13; h *= 0xc2b2ae35; h ^= h>>16).  With the same table and seed the
 * frame is reproducible to the RGB parity bar; with another table it agrees statistically.
 * closest_hit = 0: a sample ray stops at the first leaf that accepts a triangle (the count needs the hit flag only and
 * that flag is the reference's); 1: full closest-hit walk, for checking that claim. */
typedef struct CgrtSoftShadows {
    const float* spherical;    /* nspherical x 7 {position, radius, color} (SphericalLight, scene.h:47-51) */
    const float* unit_vectors; /* nunits x 3 */
    uint32_t nspherical, samples, nunits, seed;
    int32_t closest_hit;
} CgrtSoftShadows;
int cgrt_render_soft(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                     const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats);
/* cgrt_render_soft without the last copy: *rgb receives a pointer to the frame in PINNED host memory owned by the scene (W*H*3
 * floats, index y*W+x), into which the device frame was downloaded with one asynchronous copy; it stays valid until the next
 * cgrt_render* call on this scene or cgrt_scene_destroy.  For callers that convert the frame anyway (Screen::setPixel's flip,
 * screen.cpp:30-36): a 1920x1080 float frame is 25 MB, and copying it once more costs several device frames.  soft may be NULL. */
int cgrt_render_mapped(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                       const CgrtSoftShadows* soft, int max_level, const float** rgb, CgrtRenderStats* stats);
/* Image tiling across GPUs for whole frames: this call traces and shades only the pixels whose
 * 64x64 super-tile index % nranks == rank (the ownership rule of cgrt_trace_primary); every secondary ray of a pixel
 * stays on the GPU that owns the pixel, so ranks exchange nothing.  rgb of pixels owned by other ranks is left as the
 * caller passed it; the ranks' frames merge by ownership into exactly the single-rank frame.  soft may be NULL. */
int cgrt_render_rank(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                     const CgrtSoftShadows* soft, int max_level, int rank, int nranks, float* rgb, CgrtRenderStats* stats);

/* cgrt_render with the instrumented kernels (a separate, never timed frame): work3[0] / [1] / [2] receive the traversal work of
 * the primary rays, of all shadow lists and of all mirror lists of the frame (SURVEY.md section 8(d) algorithmic bytes). */
int cgrt_render_counted(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                        int max_level, float* rgb, CgrtRenderStats* stats, CgrtCounters* work3);

/* One caller, N devices, ONE framebuffer (the reference's renderRayTracing fills one Screen,
 * main.cpp:648-720, its only parallel construct being rows of that frame, :653-656).  scenes[i] is a replica of the scene
 * created on its own device (cgrt_scene_create with different `device` arguments; the same device may repeat, every
 * replica must be a distinct handle).  Replica i traces / renders the 64x64 super-tiles i % nscenes; nothing is exchanged
 * between devices.  trace: all launches are issued first, each on a private stream of its replica; every device downloads
 * its pixels with one asynchronous copy and a host thread per replica scatters them into `hits` / `normals` (normals
 * only where hit == 1).  render: one host thread per replica runs cgrt_render_rank's wavefront into a frame of its own
 * and the owned pixels are merged into `rgb`; stats: ray counts summed, levels / device_ms = maximum over replicas.
 * The bytes written equal those of the single-device entries (tested). */
typedef struct CgrtMultiStats {
    int32_t replicas;
    float kernel_ms_max;   /* slowest replica's traversal kernel (HIP events on its stream) */
    float download_ms_max; /* slowest replica's device -> pinned host copy */
    double wall_ms;        /* first launch to last pixel scattered, host clock */
    uint64_t rays[64];     /* pixels traced by each replica */
} CgrtMultiStats;
int cgrt_trace_primary_multi(CgrtScene* const* scenes, int nscenes, const CgrtCamera* cam, int W, int H, CgrtHit* hits,
                             float* normals, CgrtMultiStats* stats);
int cgrt_render_multi(CgrtScene* const* scenes, int nscenes, const CgrtCamera* cam, int W, int H, const float* lights,
                      uint32_t nlights, const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats);

/* The reference's antiAliasing branch (src/main.cpp:663-687, checkbox "Add Anti Aliasing" :878-882): 2x2 sub-samples per pixel, each a
 * full getFinalColor, summed in loop order and divided by 5.0f (level * 2.5f upstream).  For pixel (x, y) of the W x H frame:
 *     color = 0;  for yc in {2y, 2y+1}: for xc in {2x, 2x+1}: color = color + getFinalColor(ray of ndc (xc/W*1.0f-1.0f, yc/H*1.0f-1.0f));
 *     rgb = color / 5.0f   (each channel ((0 + c[2y][2x]) + c[2y][2x+1]) + c[2y+1][2x]) + c[2y+1][2x+1], then an IEEE division)
 * Findings (DESIGN.md "Anti-aliasing"):
 *   AA1  upstream's accumulator `glm::vec3 color;` (:660) is uninitialised (glm 0.9.9.8 without GLM_FORCE_CTOR_INIT): restated as zero;
 *   AA2  the four samples are divided by 5, not 4 (:685): an AA frame is 4/5 as bright as its samples' mean -- reproduced, the library is
 *        a drop-in;
 *   AA3  sub-sample (xc, yc) gets the ray of pixel (xc, yc) of a 2W x 2H frame: upstream's float(xc)/W*1.0f-1.0f equals
 *        float(xc)/float(2W)*2.0f-1.0f bit for bit (scaling by powers of two is exact here; tested for every xc), and the aspect ratio
 *        (Window::aspectRatio) is the same for both frames;
 *   AA4  only 2x2 exists upstream (the loop bound 2 + level*y is hard-coded): nothing here generalises to k x k.
 * So with point lights an AA frame is the library's own 2W x 2H frame resolved as above; with spherical lights sub-sample (xc, yc)
 * hashes as pixel p = yc*2W + xc (cgrt_render_soft), so soft AA frames are the 2W x 2H soft frame of the same table and seed, resolved.
 * The wavefront (primary kernel, spawn / shadow / mirror lists, fold, soft-shadow kernels, frame prediction) runs unchanged over the
 * 4*W*H sub-samples; a device kernel resolves the frame and only W*H*3 floats come down.
 * rank/nranks as cgrt_render_rank (0/1 = whole frame), applied to the sub-sample frame: a rank owns the 64x64 super-tiles
 * (index % nranks == rank, row-major) of the 2W x 2H frame, i.e. the 32x32-pixel blocks of the W x H frame, so a pixel's four
 * sub-samples always belong to the rank that owns the pixel; pixels of other ranks keep the caller's contents.  soft may be NULL.
 * stats count the rays that exist upstream (primary_rays = 4*W*H).  Workspace: about 0.3 KB per SUB-SAMPLE (roughly 2.5 GB for a
 * 1920x1080 AA frame; extrapolated from the note at cgrt_render, not measured).
 * Every argument is checked before any device work: NULL pointers, nlights > 0 with lights NULL, W or H <= 0, 4*W*H > 0x7fffffff,
 * max_level outside 0..16, bad rank / nranks, bad soft -> CGRT_E_ARG; then a host-only scene -> CGRT_E_NO_DEVICE. */
int cgrt_render_aa(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                   const CgrtSoftShadows* soft, int max_level, int rank, int nranks, float* rgb, CgrtRenderStats* stats);
/* As cgrt_render_mapped: *rgb receives the scene's pinned W*H*3 frame (index y*W+x), valid until the next cgrt_render* call on it. */
int cgrt_render_aa_mapped(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                          const CgrtSoftShadows* soft, int max_level, const float** rgb, CgrtRenderStats* stats);
/* As cgrt_render_multi: replica i renders the sub-sample super-tiles i % nscenes (the ownership rule of cgrt_render_aa), resolves them
 * on its device and downloads only its own resolved pixels.  The bytes written equal those of cgrt_render_aa (tested). */
int cgrt_render_multi_aa(CgrtScene* const* scenes, int nscenes, const CgrtCamera* cam, int W, int H, const float* lights,
                         uint32_t nlights, const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats);

/* Shaded frames straight into DEVICE memory: the frame of cgrt_render_soft (aa = 0) or cgrt_render_aa (aa != 0) -- same wavefront,
 * same prediction, same soft-shadow hashing, same stats (device_ms does not include the export) -- is not downloaded; a device
 * kernel (k_export_frame) writes it into d_out in one of these formats: */
#define CGRT_FRAME_RGB_F32 0 /* W*H*3 f32, element (y*W + x)*3 + c: the bytes cgrt_render / cgrt_render_aa return */
#define CGRT_FRAME_CHW_F32 1 /* 3 planes of H rows x W f32 (torch's (3, H, W)): plane c, row y, column x = the same value */
#define CGRT_FRAME_RGBA8 2   /* the reference's 8-bit screen image (screen.cpp:30-49): row H-1-y (Screen::setPixel's flip), bytes R, G, B, */
                             /* 255, each (uint8_t)(min(max(v, 0.0f), 1.0f) * 255.0f) -- truncation; a NaN channel gives 0          */
/* The float formats hold the bit patterns of cgrt_render_soft / cgrt_render_aa.
 * row_bytes: 0 = packed rows; otherwise the distance between rows (at least the packed row, a multiple of 4; CHW: the plane stride is
 * row_bytes * H).  Padding bytes are never written.  d_out: device memory of the scene's device, 4-byte aligned.
 * rank/nranks: the ownership rule of cgrt_render_rank (64x64 super-tiles), or with aa that of cgrt_render_aa (32x32-pixel blocks of
 * the W x H frame); only owned pixels are written, so the ranks' outputs merge into exactly the single-rank output.
 * Stream: the call blocks until the frame's kernels are done (level sizing reads counts on the host, as in cgrt_render) and returns
 * with the export ENQUEUED on `stream` (a hipStream_t of the scene's device, NULL = default stream): work the caller enqueues on
 * `stream` afterwards sees the frame, and the export runs after everything the caller enqueued there before the call.  The export
 * reads the scene's workspace: the scene records an event of its own behind it, which every stream of the next cgrt_render* frame on
 * the scene waits for before writing that workspace (and which cgrt_scene_destroy waits for); the stream handle is not kept.
 * Arguments are checked in the order of cgrt_render_aa: NULL scene / cam / d_out, nlights > 0 with lights NULL, W or H <= 0, (aa)
 * 4*W*H > 0x7fffffff, max_level outside 0..16, bad rank / nranks, bad soft, unknown format, bad row_bytes, d_out not 4-byte aligned
 * -> CGRT_E_ARG; then a host-only scene -> CGRT_E_NO_DEVICE; then the bytes the frame spans from d_out not all device memory of the
 * scene's device -- one allocation, or allocations that follow one another in the address space (a pool mapped in pieces, such as
 * torch's expandable segments) -- (hipPointerGetAttributes, hipMemGetAddressRange: a pointer of another HIP runtime in the process
 * fails here too) -> CGRT_E_ARG, before the frame is rendered. */
int cgrt_render_device(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                       const CgrtSoftShadows* soft, int max_level, int aa, int rank, int nranks, void* d_out, int format,
                       uint64_t row_bytes, void* stream, CgrtRenderStats* stats);
/* Diagnostic: the export kernel of cgrt_render_device on a frame the caller supplies.  Host pointers: rgb (W*H*3 f32) is uploaded,
 * `out` (as many bytes as the format and row_bytes span) is uploaded too, every pixel is exported on device `device` and `out` comes
 * back -- bytes the export does not write keep their values.  Synchronous. */
int cgrt_debug_export_frame(int device, const float* rgb, int W, int H, int format, uint64_t row_bytes, void* out);

/* getFinalColor(scene, bvh, ray) (main.cpp:298-310) of the CALLER's rays: rgb[3i..3i+2] = the colour of rays[i], with the reference's
 * recursion cut at max_level (2 = upstream), the same wavefront as cgrt_render_soft from level 0 on.  Outputs are written for every
 * i < n and nowhere else.  A ray is taken as given: the walk starts from its t (the reference's `t >= ray.t` rule, so a ray whose t
 * ends before the first surface is black), its direction need not be unit length (the mirror ray's t is |d|, main.cpp:254).
 * Soft shadows: sample smp of ray i hashes with p = i in cgrt_render_soft's formula, so the row-major rays of cgrt_generate_rays over
 * a whole W x H frame give that frame's draws, and the frame itself, bit for bit.  The result does not depend on the list's order
 * (a permutation of the rays permutes the colours) nor on the kernel shape, but the speed does: rays next to each other in the list
 * share waves, and a list in the frame's 8 x 8 tile order traverses faster than the same rays row-major.
 * stats: as the render entries count them; primary_rays = n when max_level >= 1.  The call always takes the exactly sized path and
 * neither reads nor writes the scene's frame prediction or frame hints.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene, rgb, or rays with n > 0, or nlights > 0 with NULL
 * lights; n > 0x7fffffff; max_level outside 0..16; bad `soft` (cgrt_render_soft's rules).  Then a host-only scene: CGRT_E_NO_DEVICE.
 * n == 0 succeeds with zeroed stats and touches nothing; max_level == 0 writes black and traces nothing.
 * cgrt_shade_rays: host pointers (staged through pinned memory; synchronous). */
int cgrt_shade_rays(CgrtScene* scene, const CgrtRay* rays, uint64_t n, const float* lights, uint32_t nlights,
                    const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats);
/* cgrt_shade_rays_device: d_rays (n * 28 bytes) and d_rgb (n * 12 bytes) are device memory of the scene's device, each 4-byte aligned,
 * in one allocation or several that follow one another in the address space (checked as cgrt_render_device checks d_out; CGRT_E_ARG
 * before any work otherwise).  Stream order: the call's work runs after everything enqueued on `stream` before the call (where the
 * rays were written), and work enqueued on `stream` after the call returns sees the colours.  The colours are written straight into
 * d_rgb; the call returns when they are there.  The stream handle is not kept. */
int cgrt_shade_rays_device(CgrtScene* scene, const CgrtRay* d_rays, uint64_t n, const float* lights, uint32_t nlights,
                           const CgrtSoftShadows* soft, int max_level, float* d_rgb, void* stream, CgrtRenderStats* stats);

/* Multi-view frames: a batch of nviews >= 1 cameras that share one frame shape W x H, the lights, the soft-shadow settings and max_level,
 * in ONE primary launch and one set of wavefront lists.  View b is bit for bit the single-camera frame of
 * cams[b]; the views may differ in every camera field.  Pixel (x, y) of view b has index b*W*H + y*W + x.
 * Limits: nviews * W * H <= 0x7fffffff, and at most 2^18 64x64 super-tiles over all views.  Not batched (use the single-camera
 * entries): anti-aliasing, rank / nranks ownership, replicas on several devices, per-view frame sizes, per-view lights.
 * Checks, all CGRT_E_ARG and before any device work: NULL scene / cams / output, nlights > 0 with NULL lights, nviews == 0, W or H <= 0,
 * the limits above, max_level outside 0..16, bad `soft` (cgrt_render_soft's rules), unknown format, output not 4-byte aligned; then a
 * host-only scene -> CGRT_E_NO_DEVICE; then (device outputs) the bytes the batch spans not all device memory of the scene's device
 * (checked as cgrt_render_device checks d_out) -> CGRT_E_ARG.  No entry reads or writes the scene's frame prediction or frame hints:
 * a single-camera frame after a batch takes the path and gives the bytes it would have without the batch.
 *
 * cgrt_trace_primary_views_device: Trackball::generateRay (trackball.cpp:92-103) + intersect for every pixel of every view:
 * d_hits[b*W*H + y*W + x] (and d_normals, 3 floats each, may be NULL) = what cgrt_trace_primary_device(cams[b], W, H, whole frame,
 * rank 0 of 1) writes at y*W + x.  Nothing else is written.  Asynchronous on `stream` like cgrt_trace_primary_device: the camera table
 * is copied into the scene's own pinned memory before the call returns (the caller may reuse cams at once); the scene keeps four
 * such tables, and a call whose table slot is still in use by a launch four calls back waits for that launch. */
int cgrt_trace_primary_views_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, CgrtHit* d_hits,
                                    float* d_normals, void* stream);
/* cgrt_render_views: renderRayTracing's per-pixel loop (main.cpp:648-720) around getFinalColor (:298-310) for every view: rgb (host,
 * nviews*W*H*3 f32) holds the views back to back, view b's bytes those of cgrt_render_soft(cams[b], ...) (cgrt_render with soft NULL).
 * Spherical-light sample smp of pixel (x, y) of view b is drawn with p = y*W + x, as in the single frame.  stats: ray counts summed
 * over the views, device_ms for the whole batch; the call always takes the exactly sized path.  Synchronous. */
int cgrt_render_views(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                      const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats);
/* cgrt_render_views_device: the same views exported into device memory in one launch: view b starts at d_out + b * (the packed frame
 * bytes of `format`) and holds cgrt_render_device's packed bytes for cams[b] (aa = 0, rank 0 of 1) -- a contiguous (B, H, W, 3) f32,
 * (B, 3, H, W) f32 or (B, H, W, 4) u8 array.  Stream rules of cgrt_render_device: the call blocks until the batch's kernels are done
 * and returns with the export enqueued on `stream`, behind everything the caller enqueued there before; the scene's export event is
 * recorded behind it. */
int cgrt_render_views_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights,
                             uint32_t nlights, const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream,
                             CgrtRenderStats* stats);

/* Light sets: ONE camera, one W x H frame, one max_level and one set of soft-shadow sampling parameters rendered under nsets light setups
 * (the reference's Lights panel edits the lights and renders the same view again, src/main.cpp:812-870).  Set b
 * holds its own point lights (light_offsets[b] .. light_offsets[b+1] - 1, 6 floats each {position, color}, PointLight, scene.h:42-45) and
 * its own spherical lights (spherical_offsets[b] .. spherical_offsets[b+1] - 1, 7 floats each {position, radius, color}, SphericalLight,
 * scene.h:47-51); either count may be 0 and the counts may differ from set to set.  spherical_offsets NULL: no set has spherical lights.
 * Frame b is, bit for bit, what cgrt_render_soft (cgrt_render without spherical lights) returns for cam and set b's lights: spherical-light
 * sample smp of pixel p = y*W + x at level lv is drawn with l = the light's index WITHIN SET b, as in that single frame.
 * What is shared: a pixel's ray tree (primary hit, mirror rays, which levels exist) does not depend on the lights, so the primary launch,
 * every level's spawn and every mirror list run once per batch; a point light's shadow ray and its verdict (pointInShadow, main.cpp:104-135)
 * depend on its position alone, so shadow rays are traced once per DISTINCT point-light position over all sets; a spherical light's sample
 * count depends on its position, its radius and its in-set index, never on its colour, so counts are taken once per distinct (position,
 * radius, in-set index).  Colour enters only the Phong terms (shading, main.cpp:160-235), which are evaluated per set.  Positions and radii
 * are compared by BIT PATTERN: +0.0 and -0.0 are distinct, and so are NaN payloads.  The dedupe never changes a byte, only the counts:
 * stats: primary_rays, reflection_rays and levels are the single frame's; shadow_rays = (hits over all levels) x (distinct point-light
 * positions); soft_shadow_rays = (hits over all levels) x (distinct spherical keys) x samples; device_ms covers the whole batch.  These
 * differ from the sums over nsets single frames whenever sets share lights (a colour sweep traces exactly one frame's rays).
 * `soft` carries only the sampling parameters (unit_vectors, nunits, samples, seed, closest_hit): its spherical must be NULL and nspherical
 * 0; soft may be NULL only when no set has spherical lights.  Whole frames, rank 0 of 1, no anti-aliasing; the call always takes the exactly
 * sized path and neither reads nor writes the scene's frame prediction or frame hints.  Workspace beyond a single frame's: max_level x
 * (frame items) x nsets x 16 bytes of per-set colours (about 2 GB at 1920x1080, max_level 4, nsets 16) and nsets x W x H x 12 bytes of
 * frames.
 * Checks, all CGRT_E_ARG and before any device work: NULL scene / cam / sets / output; nsets 0 or above 1024; light_offsets NULL; offsets
 * that do not start at 0 or that decrease; lights (spherical) NULL while its count is > 0; spherical lights without a valid soft (unit
 * table, 1..2^24 samples), or a soft that carries spherical lights of its own; W or H <= 0; max_level outside 0..16; W*H > 0x7fffffff;
 * W*H x (distinct point-light positions) or W*H x (distinct spherical keys) above 0x7fffffff (the lists' 32-bit indices); (device form)
 * unknown format, d_out not 4-byte aligned.  Then a host-only scene -> CGRT_E_NO_DEVICE; then (device form) the bytes the batch spans not
 * all device memory of the scene's device (as cgrt_render_device checks d_out) -> CGRT_E_ARG.  A batch that fails writes nothing to the
 * output and leaves the scene usable. */
typedef struct CgrtLightSets {
    uint32_t nsets;                    /* B, 1 .. 1024 */
    const float* lights;               /* point lights of all sets, set after set: light_offsets[nsets] x 6 {position, color} */
    const uint32_t* light_offsets;     /* nsets + 1, [0] = 0, non-decreasing */
    const float* spherical;            /* spherical lights, set after set: spherical_offsets[nsets] x 7 {position, radius, color} */
    const uint32_t* spherical_offsets; /* nsets + 1 ([0] = 0, non-decreasing), or NULL: no set has spherical lights */
} CgrtLightSets;
/* cgrt_render_light_sets: rgb (host) holds nsets*W*H*3 floats, the sets' frames back to back (set b's pixel (x, y) at b*W*H + y*W + x).
 * Synchronous. */
int cgrt_render_light_sets(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const CgrtLightSets* sets, const CgrtSoftShadows* soft,
                           int max_level, float* rgb, CgrtRenderStats* stats);
/* cgrt_render_light_sets_device: set b starts at d_out + b * (the packed frame bytes of `format`) and holds cgrt_render_device's packed
 * bytes for cam and set b's lights (aa = 0, rank 0 of 1) -- a contiguous (B, H, W, 3) f32, (B, 3, H, W) f32 or (B, H, W, 4) u8 array.
 * Stream and export-event rules of cgrt_render_views_device: the call blocks until the batch's kernels are done and returns with the
 * export enqueued on `stream`, behind everything the caller enqueued there before. */
int cgrt_render_light_sets_device(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const CgrtLightSets* sets,
                                  const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, CgrtRenderStats* stats);

/* Enqueued frames: the three device entries above without waiting for the GPU.  Each takes its blocking
 * counterpart's arguments, with a ticket out-parameter (NULL allowed) in place of the stats, and writes exactly the bytes its counterpart
 * writes for the same arguments (every format, row pitch, aa, rank / nranks, soft-shadow setting and max_level 0..16); bytes outside the
 * output, and pixels of other ranks, are never written.  Arguments are checked in the counterpart's order with its error codes, before
 * anything is enqueued; a host-only scene is CGRT_E_NO_DEVICE.
 * Stream order: the whole frame, export included, runs on `stream` (NULL = default stream), after everything enqueued there before the call
 * (for ray lists: the kernel that wrote the rays); work enqueued there afterwards sees the finished output.  The library's own streams are
 * not used.  The lights, camera(s) and soft-shadow tables are copied at the call (through pinned memory, hipMemcpyAsync on `stream`): the
 * caller may reuse every host array as soon as the call returns.  Device buffers (d_out, d_rays, d_rgb) must stay valid until the frame
 * has run on `stream`.
 * The call returns without waiting for the GPU, except (1) when the scene's workspace has to grow -- the first frame of a larger shape, more
 * lights or a deeper level: it then waits for the scene's outstanding frames -- and (2) when all 8 of the scene's ticket slots are in
 * flight: it then waits for the oldest one.
 * Frames of one scene, enqueued and blocking, on any streams and in any order, each get their own bytes: every frame starts on the device
 * behind the scene's last enqueued frame and behind the export of its last blocking one.  cgrt_scene_destroy waits for every outstanding
 * frame.  Enqueued frames neither read nor write the scene's frame prediction record or its frame hints: a blocking frame takes the path
 * (cgrt_debug_render_path) and writes the bytes it would without them.
 * Ticket: the scene's frame sequence number of the enqueued frame (frames are numbered from 1, blocking ones included).  cgrt_enqueue_stats
 * waits for that frame and returns its CgrtRenderStats: ray counts and levels equal to the blocking call's, device_ms from events around
 * the frame on its stream.  A ticket that was never issued, or is older than the scene's last 8 enqueued frames, is CGRT_E_ARG. */
int cgrt_enqueue_render_device(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                               const CgrtSoftShadows* soft, int max_level, int aa, int rank, int nranks, void* d_out, int format,
                               uint64_t row_bytes, void* stream, uint64_t* ticket);
int cgrt_enqueue_render_views_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights,
                                     uint32_t nlights, const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream,
                                     uint64_t* ticket);
int cgrt_enqueue_shade_rays_device(CgrtScene* scene, const CgrtRay* d_rays, uint64_t n, const float* lights, uint32_t nlights,
                                   const CgrtSoftShadows* soft, int max_level, float* d_rgb, void* stream, uint64_t* ticket);
int cgrt_enqueue_stats(CgrtScene* scene, uint64_t ticket, CgrtRenderStats* stats);
/* Diagnostic: the cap, in waves, of every count-driven launch of an enqueued frame (each list of a paired launch gets it): 6144, or the
 * value of CGRT_STRIDED_WAVES (64 .. 2^24), read once per process. */
int cgrt_debug_strided_waves(void);

/* Multi-view light sets: V = nviews cameras under S = sets->nsets light setups in one call -- the two batch
 * families above together, for a relighting rig (every camera under every lighting) or a Lights-panel edit previewed from several
 * viewpoints.  The cameras share W x H, max_level and the soft-shadow sampling parameters; the sets are a CgrtLightSets as for
 * cgrt_render_light_sets, `soft` with its rules (sampling parameters only).  With nviews = 1 these are light sets for one camera, and the
 * enqueued form is the enqueued light-set batch.
 * Layout: frame (v, s) is frame number v*S + s of the batch, so its pixel (x, y) is element ((v*S + s)*H + y)*W + x.  The host form
 * writes V*S*W*H*3 floats; the device forms write frame (v, s) at d_out + (v*S + s) * (the packed frame bytes of `format`): a contiguous
 * (V, S, H, W, 3) f32, (V, S, 3, H, W) f32 or (V, S, H, W, 4) u8 array.
 * Bytes: frame (v, s) is, bit for bit, what cgrt_render_soft (cgrt_render without spherical lights) returns for cams[v] under set s's
 * lights: spherical-light sample smp draws with the in-view pixel p = y*W + x, the level and l = the light's index WITHIN ITS SET (the
 * rules of both families).  So out[v] is the byte image of cgrt_render_light_sets(cams[v], sets), and out[:, s] that of
 * cgrt_render_views(cams, set s's lights).
 * What is shared: the primary launch, every level's spawn and every mirror list run once for all views, as in cgrt_render_views; shadow
 * rays run once per hit and per DISTINCT point-light position over all sets, soft-shadow counts once per hit and per distinct (position,
 * radius, in-set index) key, compared by bit pattern as cgrt_render_light_sets compares them; light colour enters only the per-set Phong
 * terms.
 * stats: primary_rays = V*W*H when max_level >= 1; reflection_rays and levels those of cgrt_render_views(cams); shadow_rays = (hits over all
 * views and levels) x (distinct positions); soft_shadow_rays = (hits over all views and levels) x (distinct keys) x samples.  The four ray
 * counts are the sums over v of cgrt_render_light_sets(cams[v], sets)'s, levels their maximum; device_ms covers the whole batch.
 * Checks, all CGRT_E_ARG and before any device work, in this order: NULL scene / cams / sets / output; nviews == 0; the sets' rules of
 * cgrt_render_light_sets (nsets 1 .. 1024, light_offsets NULL, offsets that do not start at 0 or that decrease, lights or spherical NULL
 * while its count is > 0, a soft with spherical lights of its own, spherical lights without a valid soft); W or H <= 0; max_level outside
 * 0..16; V*W*H > 0x7fffffff or more than 2^18 64x64 super-tiles over all views; V*W*H x (distinct point-light positions) or V*W*H x
 * (distinct spherical keys) above 0x7fffffff, or V*W*H x (distinct keys) x samples above 64 x 0x7fffffff; V*S*W*H > 0x7fffffff; (device forms)
 * unknown format, d_out not 4-byte aligned.  Then a host-only scene -> CGRT_E_NO_DEVICE; then (device forms) the V*S frames' bytes not all
 * device memory of the scene's device (as cgrt_render_device checks d_out) -> CGRT_E_ARG.  A batch that fails writes nothing to the output
 * and leaves the scene usable.
 * Scene state: no entry reads or writes the scene's frame prediction or frame hints.  The blocking forms take the exactly sized path.
 * Memory: beyond a multi-view frame's workspace, max_level x (the batch's items, about V*W*H) x S x 16 bytes of per-set colours and
 * V*S*W*H*12 bytes of frames -- at 256x256, V = S = 16 and max_level 4 that is about 1.07 GB and 0.2 GB (arithmetic, not a measurement).
 * Not batched: anti-aliasing, rank / nranks, replicas on several devices, per-view frame sizes, prediction for batches; there is no C++
 * mirror (no reference function takes several cameras or light sets). */
/* cgrt_render_views_light_sets: rgb (host) holds the V*S frames in the layout above.  Synchronous. */
int cgrt_render_views_light_sets(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const CgrtLightSets* sets,
                                 const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats);
/* cgrt_render_views_light_sets_device: stream and export-event rules of cgrt_render_views_device: the call blocks until the batch's kernels
 * are done and returns with the export of all V*S frames enqueued on `stream`, behind everything the caller enqueued there before. */
int cgrt_render_views_light_sets_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const CgrtLightSets* sets,
                                        const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream,
                                        CgrtRenderStats* stats);
/* cgrt_enqueue_render_views_light_sets_device: the device form without waiting for the GPU, under the rules of the enqueued frames above
 * (the same bytes; the whole batch on `stream`; a wait only when the workspace grows or all 8 ticket slots are in flight).  The cameras,
 * the sets' plan table, the distinct light tables and the unit vectors are copied through the ticket slot's pinned staging, so the caller
 * may reuse every host array at once.  cgrt_enqueue_stats(ticket) returns the blocking call's ray counts and levels. */
int cgrt_enqueue_render_views_light_sets_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H,
                                                const CgrtLightSets* sets, const CgrtSoftShadows* soft, int max_level, void* d_out,
                                                int format, void* stream, uint64_t* ticket);

/* Geometry buffers ("AOVs") of a device frame: what the frame's primary rays saw -- depth, surface normal, hit
 * point, albedo, primitive / material id, coverage -- written by the call that writes the shaded frame, from level 0 of the frame's own
 * wavefront: no second trace.  Every pointer is device memory of the scene's device, aligned to its element size, or NULL (plane not
 * wanted: it costs nothing and is never touched). */
typedef struct CgrtAovOut {
    float*    depth;        /* 1 x f32 per pixel: CgrtHit.t of the pixel's primary ray (the untouched FLT_MAX on a miss)            */
    float*    normal;       /* 3 x f32: the normal cgrt_trace_primary_device writes for a hit; 0, 0, 0 on a miss                    */
    float*    position;     /* 3 x f32: the reference's pointOn, ray.origin + ray.direction * ray.t (main.cpp:164), of the primary  */
                            /*          ray, f32, product rounded, then sum rounded (no FMA); 0, 0, 0 on a miss                     */
    float*    albedo;       /* 3 x f32: kd of material_id's Material; 0, 0, 0 for material_id -1 (miss, sphere-only hit) -- the kd  */
                            /*          k_shade uses                                                                                */
    uint32_t* prim_id;      /* CgrtHit.prim_id (CGRT_NO_PRIM on a miss)                                                             */
    int32_t*  material_id;  /* CgrtHit.material_id                                                                                  */
    uint8_t*  mask;         /* CgrtHit.hit, 0 or 1                                                                                  */
    int       chw;          /* 3-channel planes: 0 = (H, W, 3), 1 = (3, H, W)                                                       */
} CgrtAovOut;
/* Planes are packed (no row pitch), row-major, pixel (x, y) at y*W + x, NOT y-flipped, whatever `format` the colour has.  Every owned pixel
 * of every requested plane is written, hit or miss (unlike the normals of cgrt_trace_primary_device); no byte outside a requested plane, and
 * no pixel of another rank, is written.  The values are, bit for bit, the fields cgrt_trace_primary_device returns for the same camera.
 * Each entry below is its counterpart plus `aov`, and writes the colour, the stats, the render path, the prediction record and the frame
 * hints exactly as the counterpart does; device_ms excludes the plane export as it excludes the colour export.
 *   cgrt_render_aov_device        cgrt_render_device + planes of (H, W).  With aa != 0 the planes are those of the 2W x 2H sub-sample frame
 *                                 the wavefront traces, (2H, 2W), equal to cgrt_trace_primary_device(cam, 2W, 2H); aa planes need nranks == 1.
 *   cgrt_render_views_aov_device  cgrt_render_views_device + planes with a leading view axis: (B, H, W), (B, H, W, 3) or (B, 3, H, W).
 *   cgrt_enqueue_render_aov_device, cgrt_enqueue_render_views_aov_device: the same two under the rules of the enqueued frames above; the
 *                                 planes are complete on `stream` when the colour is.
 * The planes are ordered on `stream` as the colour is -- written behind everything the caller enqueued there before the call, complete for
 * everything enqueued there after it -- and the scene's export event is recorded behind them too: the next frame on the scene and
 * cgrt_scene_destroy wait for them.  Arguments are checked in the counterpart's order with its codes; then aov NULL or without any plane,
 * max_level == 0 (no primary ray is traced at depth 0: nothing to export), aa with nranks > 1, a plane not aligned to its element size
 * -> CGRT_E_ARG; then a host-only scene -> CGRT_E_NO_DEVICE; then every requested plane's extent is checked to be device memory of the
 * scene's device as d_out is -> CGRT_E_ARG, all before any device work.
 * Not offered: light-set entries (the planes do not depend on the lights: render the views once with cgrt_render_views_aov_device), ray
 * lists (cgrt_intersect_batch_device returns exactly this for caller rays), host-memory outputs, the *_multi entries, aa planes per rank
 * (aa ownership is in packed 32 x 32 blocks), and the C++ host mirror (the reference has no such output). */
int cgrt_render_aov_device(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                           const CgrtSoftShadows* soft, int max_level, int aa, int rank, int nranks, void* d_out, int format,
                           uint64_t row_bytes, void* stream, CgrtRenderStats* stats, const CgrtAovOut* aov);
int cgrt_render_views_aov_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights,
                                 uint32_t nlights, const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream,
                                 CgrtRenderStats* stats, const CgrtAovOut* aov);
int cgrt_enqueue_render_aov_device(CgrtScene* scene, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                                   const CgrtSoftShadows* soft, int max_level, int aa, int rank, int nranks, void* d_out, int format,
                                   uint64_t row_bytes, void* stream, uint64_t* ticket, const CgrtAovOut* aov);
int cgrt_enqueue_render_views_aov_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights,
                                         uint32_t nlights, const CgrtSoftShadows* soft, int max_level, void* d_out, int format,
                                         void* stream, uint64_t* ticket, const CgrtAovOut* aov);

/* Ray cameras: a second, general way to make the primary ray of a pixel, next to the reference's Trackball
 * (CgrtCamera).  Origin and unnormalised direction are both affine in the pixel, which covers a pinhole with any intrinsic matrix K (skew,
 * non-square pixels, off-centre principal point) and any pose (origin_dx = origin_dy = 0), an orthographic camera (dir_dx = dir_dy = 0,
 * the origins on a plane) and pushbroom-like mixtures of the two. */
typedef struct CgrtRayCamera {      /* 80 bytes */
    float origin[3], origin_dx[3], origin_dy[3];
    float dir[3],    dir_dx[3],    dir_dy[3];
    int32_t x_off, y_off;
} CgrtRayCamera;
/* The ray of pixel (x, y) of a W x H frame, in f32, every operation rounded, nothing contracted:
 *   fx = (float)(x + x_off);  fy = (float)(y + y_off)         (32-bit integer add, then convert)
 *   o.c = (origin.c + fx * origin_dx.c) + fy * origin_dy.c     c = x, y, z
 *   v.c = (dir.c    + fx * dir_dx.c)    + fy * dir_dy.c
 *   d   = v * (1.0f / sqrt((v.x*v.x + v.y*v.y) + v.z*v.z))     (the library's normalise; IEEE sqrt and division)
 *   t   = FLT_MAX
 * W and H do not enter: the caller folds pixel centres, the principal point and the direction of y into `dir`.  A pixel whose v is zero
 * gets the NaN direction the formula gives and is treated as that ray is treated in a ray list.
 * Tiles are exact: the rays of a w x h frame with offsets (X, Y) are, bit for bit, the rays of pixels (X + x, Y + y) of the same camera
 * with zero offsets, so a large image can be split over calls, streams or devices and give the same bytes -- hits, every geometry plane
 * and the colour under point lights.  The one exception: the soft-shadow draws of spherical lights hash the tile's own pixel index
 * y*W + x, into which the offsets do not enter, so tiles lit by spherical lights agree with the full frame statistically, not bit for bit.
 * Camera checks, all CGRT_E_ARG, made where the Trackball twin checks `cams`: a non-finite field; dir, dir_dx and dir_dy all zero;
 * |x_off| + W or |y_off| + H above 2^24 (the int -> float conversion stays exact).
 *
 * Every entry is views-shaped (nviews >= 1; one view is the single frame; pixel (x, y) of view b at b*W*H + y*W + x) and is the twin of a
 * Trackball entry: the same argument checks in the same order with the same codes, the same limits (nviews * W * H <= 0x7fffffff, at
 * most 2^18 64x64 super-tiles over all views, max_level 0..16), the same stream, export-event, ticket and stats rules, the same output
 * layouts.  Like every views call they take the exactly sized path and neither read nor write the prediction record or the frame hints.
 * Everything behind level 0 -- lists, shading, export, geometry planes -- is the Trackball entries' own code.
 *   cgrt_generate_rays_raycam             the rays of a whole frame into host memory, row-major (cgrt_generate_rays's twin); synchronous
 *   cgrt_trace_primary_raycams_device     cgrt_trace_primary_views_device's twin: only enqueues; `cams` is reusable at once
 *   cgrt_render_raycams_device            twin of cgrt_render_views_device and, with aov != NULL, of cgrt_render_views_aov_device;
 *                                         aov.position is the formula's o + d*t, rounded as CgrtAovOut states
 *   cgrt_enqueue_render_raycams_device    twin of cgrt_enqueue_render_views_device / cgrt_enqueue_render_views_aov_device (aov may be NULL)
 *   cgrt_render_raycams_light_sets_device cgrt_render_views_light_sets_device's twin
 * Not offered: host-memory outputs, anti-aliasing, rank / nranks and the *_multi entries (tiles replace them), the enqueued light-set
 * form, a per-camera far limit, and the C++ host mirror (the reference has no such camera). */
int cgrt_generate_rays_raycam(CgrtScene* scene, const CgrtRayCamera* cam, int W, int H, CgrtRay* rays);
int cgrt_trace_primary_raycams_device(CgrtScene* scene, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, CgrtHit* d_hits,
                                      float* d_normals, void* stream);
int cgrt_render_raycams_device(CgrtScene* scene, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const float* lights,
                               uint32_t nlights, const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream,
                               CgrtRenderStats* stats, const CgrtAovOut* aov);
int cgrt_enqueue_render_raycams_device(CgrtScene* scene, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const float* lights,
                                       uint32_t nlights, const CgrtSoftShadows* soft, int max_level, void* d_out, int format,
                                       void* stream, uint64_t* ticket, const CgrtAovOut* aov);
int cgrt_render_raycams_light_sets_device(CgrtScene* scene, const CgrtRayCamera* cams, uint32_t nviews, int W, int H,
                                          const CgrtLightSets* sets, const CgrtSoftShadows* soft, int max_level, void* d_out, int format,
                                          void* stream, CgrtRenderStats* stats);

/* Surface attributes: WHERE inside its triangle a ray hit, and a per-vertex quantity carried there.  The
 * reference evaluates three area ratios for every accepted triangle hit (`alpha`, `beta`, `gamma`, src/ray_tracing.cpp:94-96, with
 * `magnitude` / `area` of :13-21), uses them once to mix the vertex normals (:97) and drops them; these entries return them, and mix a
 * caller's table with them.
 * Definition.  For a ray (o, d), a parameter t and a triangle prim_id < ntris:
 *   v0, v1, v2  the positions of tri[prim_id][0..2] as given to cgrt_scene_create (the f32 values the device's triangle records hold);
 *   p           = o + d * t                                 (f32, product rounded, then sum rounded)
 *   alpha       = area(p, v1, v2) / area(v0, v1, v2)        weighs vertex 0  (:94)
 *   beta        = area(p, v0, v2) / area(v0, v1, v2)        weighs vertex 1  (:95)
 *   gamma       = area(p, v0, v1) / area(v0, v1, v2)        weighs vertex 2  (:96)
 *   area(a,b,c) = magnitude(cross(b - a, c - a)) / 2.0f, cross and differences in f32, magnitude's squares, sum and sqrt in double and
 *                 narrowed (:13-21): cgrt_math.h area_ref.  These are the values cgrt_math.h hit_normal uses, bit for bit.
 * An attribute with C channels from a table attr[nverts][C] (f32, row v = vertex v of pos_nrm):
 *   out[c]      = (alpha * attr[i0][c] + beta * attr[i1][c]) + gamma * attr[i2][c],   i0..i2 = tri[prim_id][0..2]
 * the sum order of :97, every operation rounded, nothing contracted.  With attr = the vertex normals, out is the vector the reference
 * normalises and flips into hitInfo.normal (tested bit for bit against the normals cgrt_intersect_batch returns).
 * Findings:
 *   SA1  the weights are UNSIGNED area ratios: never negative, whatever side of an edge p is on;
 *   SA2  they are not renormalised: their sum is 1 only up to rounding (largest deviation seen on 20 000 rays of the blob scene: 2.4e-7);
 *   SA3  a zero-area triangle gives the inf / NaN the formula gives.
 * The value is a pure function of (ray, t, prim_id).  The ray and t are taken as given (as cgrt_shade_rays takes its rays); nothing checks
 * that p lies in the triangle.  Zeros are written to every requested output of an item that is a miss (hit == 0, or prim_id ==
 * CGRT_NO_PRIM), a sphere hit (prim_id >= ntris) or carries any other out-of-range prim_id: a caller-supplied id never indexes out of
 * bounds.  (The frame forms have no hit flag: a miss is the CGRT_NO_PRIM of the prim_id plane.)
 * Envelope.  The cross products are products of two differences: they and the areas grow as the SQUARE of the scene's size -- quadratic
 * where the closest points are quartic and the winding numbers cubic, because magnitude takes its squares, their sum and the square
 * root in double, where nothing an f32 can hold overflows or is lost.  Per item: every non-zero f32 intermediate of the definition is a
 * normal number -- the linear ones (o, d * t, p, the vertices and the two differences each of the four areas takes) and the quadratic
 * ones (the six products and three components of each cross product, each magnitude as narrowed, each area):
 *   min_lin * 2^k >= FLT_MIN,  max_lin * 2^k <= FLT_MAX,  min_quad * 2^2k >= FLT_MIN,  max_quad * 2^2k <= FLT_MAX
 * with the minima and maxima taken at scale 1 (tests/scale_ref.py in_surface_envelope).  Inside, multiplying every position, every ray
 * origin and t by 2^k is an exact symmetry: every operation rounds as at scale 1, both operands of each ratio carry the factor 2^2k,
 * and alpha, beta, gamma have the bits they have at scale 1.  E.g. a unit-sized mesh (4 097 items each on cube, cornell, monkey, a
 * 1 848-triangle blob and the 16 311-triangle dodge, one in eight on an edge, one in sixteen on a vertex): every item is inside from
 * 2^-31 to 2^+63; at 2^-40 93.7 % (dodge) to 99.7 % (cube) are, at 2^-56 a third to nine tenths, at 2^-75 none; at 2^+64 none of the
 * unit cube's (its area overflows), a fifth of cornell's, and still all of the three finer meshes'.  The condition is a proof, not a
 * margin: no inside item was seen with other bits.  Outside the envelope the bytes are still the defined ones, on every path --
 * subnormal differences, products and areas are kept, not flushed, and an overflowed area gives the 0 (finite / inf) or NaN (inf / inf)
 * the formula gives -- but they need not be the weights of scale 1 (tests/test_surface_scale_cpu.py prints the table).
 *
 * Ray lists.  rays / hits are what cgrt_intersect_batch[_device] took and returned (t and prim_id are read from hits[i], origin and
 * direction from rays[i]); bary is n x 3 f32 {alpha, beta, gamma}; out is n x channels f32; attr is nverts x channels f32 -- an argument
 * of the call, so a table that changes every iteration needs no registration.  In the device forms every pointer, d_attr included, is
 * device memory of the scene's device.
 * Frames.  cgrt_surface_views_device takes nviews Trackball cameras, cgrt_surface_raycams_device ray cameras; d_depth (f32) and d_prim_id
 * (u32) are (B, H, W) planes -- the depth and prim_id geometry planes of cgrt_render_views_aov_device / cgrt_render_raycams_device, or the
 * t and prim_id columns of cgrt_trace_primary_views_device's hits gathered into planes.  The primary ray of every pixel is regenerated
 * from the camera by the expressions the frame was traced with: no ray buffer exists and nothing is traced again.  d_bary is (B, H, W, 3),
 * d_out (B, H, W, C); with chw != 0 they are (B, 3, H, W) and (B, C, H, W).  Either may be NULL, not both; d_attr / channels are read only
 * with d_out.  Rows are not y-flipped and every pixel of every requested output is written.  For the planes of an anti-aliased frame
 * (cgrt_render_aov_device with aa) pass 2W, 2H: the sub-sample rays are the 2W x 2H frame's (finding AA3).
 * Streams.  The device forms only enqueue on `stream` (NULL = default stream), like cgrt_intersect_batch_device: they are concurrent on
 * one scene and neither read nor write the prediction record or the frame hints.  The frame forms copy the camera table as
 * cgrt_trace_primary_views_device does (`cams` is reusable at once; four table slots).  The host forms run on a call lane like
 * cgrt_intersect_batch and are synchronous.
 * Lookup.  The kernel needs, per prim_id, the triangle's record and its three vertex indices: a table of 16 bytes per triangle, built and
 * uploaded (synchronously) by the scene's FIRST surface call, under a mutex of the scene, and released by cgrt_scene_destroy;
 * cgrt_device_bytes grows by its size then.  A scene that never makes a surface call keeps its cgrt_device_bytes, its
 * cgrt_debug_layout_hash and every array it had before these entries existed.
 * Limits: channels 1..256; n <= 0x7fffffff; frames: the limits of cgrt_trace_primary_views_device (nviews * W * H <= 0x7fffffff, at most
 * 2^18 64x64 super-tiles); an output of n x channels x 4 bytes may not exceed 2^40 bytes (the kernel indexes with 64 bits; the bound is a
 * stated one.  For frames the views limits already imply it: 2^18 super-tiles hold 2^30 pixels, 2^40 bytes at 256 channels).
 * Checks, all CGRT_E_ARG, in this order and before any device work.
 *   Lists: NULL scene, or with n > 0 NULL rays / hits / bary / out / attr; n > 0x7fffffff; (interpolation) channels outside 1..256, the
 *   output above 2^40 bytes; (device forms) a pointer not 4-byte aligned.  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0 succeeds and
 *   touches nothing.  Device forms: then d_rays (n * 28 bytes), d_hits (n * 16), d_attr (nverts * channels * 4) and the output checked as
 *   device memory of the scene's device, as cgrt_shade_rays_device checks its buffers.
 *   Frames: NULL scene / d_depth / d_prim_id, d_bary and d_out both NULL, d_out with NULL d_attr; NULL cams, (ray cameras) the camera
 *   checks, nviews == 0, W or H <= 0, the views limits; (with d_out) channels outside 1..256; a pointer not 4-byte aligned.  Then a host-only scene: CGRT_E_NO_DEVICE.  Then d_depth, d_prim_id, d_attr, d_bary, d_out checked as device memory.
 * Not offered: planes inside the cgrt_render_*aov* calls (CgrtAovOut keeps its size: two enqueued calls on one stream give the same
 * result without a second trace); per-triangle attributes (a plain gather by prim_id); enqueued-ticket forms (these calls never block);
 * sphere parameterisations; derivatives other than the one with respect to the table (below: cgrt_interpolate_hits_grad and its kin);
 * the C++ host mirror (the reference's HitInfo has no such field). */
int cgrt_hit_barycentrics(CgrtScene* scene, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, float* bary);
int cgrt_hit_barycentrics_device(CgrtScene* scene, const CgrtRay* d_rays, const CgrtHit* d_hits, uint64_t n, float* d_bary, void* stream);
int cgrt_interpolate_hits(CgrtScene* scene, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, const float* attr, uint32_t channels,
                          float* out);
int cgrt_interpolate_hits_device(CgrtScene* scene, const CgrtRay* d_rays, const CgrtHit* d_hits, uint64_t n, const float* d_attr,
                                 uint32_t channels, float* d_out, void* stream);
int cgrt_surface_views_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                              const uint32_t* d_prim_id, const float* d_attr, uint32_t channels, float* d_bary, float* d_out, int chw,
                              void* stream);
int cgrt_surface_raycams_device(CgrtScene* scene, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                                const uint32_t* d_prim_id, const float* d_attr, uint32_t channels, float* d_bary, float* d_out, int chw,
                                void* stream);

/* Surface attributes, gradients back to the per-vertex table.  The interpolation above is linear in attr; these
 * entries apply its adjoint, so that a table can be fitted to images or ray samples: given grad_out, the gradient of some scalar with
 * respect to `out`, they add the gradient with respect to attr into grad_attr.
 * Definition.  An item is valid under the forward's rule, unchanged: hit != 0 (lists) and prim_id < ntris.  For a valid item i, with
 * (alpha, beta, gamma) the cgrt_math.h hit_weights of its ray, t and triangle -- the very bits the forward used --,
 * (i0, i1, i2) = tri[prim_id] and g = grad_out[i] (C channels):
 *   grad_attr[i0][c] += alpha * g[c]
 *   grad_attr[i1][c] += beta  * g[c]
 *   grad_attr[i2][c] += gamma * g[c]
 * Each product is rounded to f32 and nothing is contracted.  A triangle that names one vertex twice contributes twice to it.  Invalid
 * items (misses, sphere hits, any out-of-range prim_id) contribute nothing: their grad_out is not multiplied in (a NaN there stays
 * out) and they never index anything.
 * Accumulation.  The calls ADD into grad_attr: the caller zeroes it, or keeps a running gradient over several calls or frames.  Only
 * rows of vertices that received a contribution are touched.
 * Order.  The order of the additions into one element is unspecified: the value is the sum, in f32, of the element's previous content
 * and its contributions in SOME order (contributions of neighbouring items may be summed with each other first), and its last bits may
 * differ from run to run.  For an element with m contributions w*g and previous content a, every such order obeys
 *   |got - exact| <= gamma(m + 1) * S + (m + 1) * 2^-126,   gamma(k) = k*u / (1 - k*u),  u = 2^-24,  S = |a| + sum |w*g|
 * (exact: the sum of a and the products of the f32 weights, in real arithmetic); this is the bound the tests use.  The hardware add
 * (global_atomic_add_f32) KEEPS subnormals on gfx950, operands and sums alike: measured under every mapping of the kernel (the shipped
 * policy, and `element`, `item` and `item_plain` of CGRT_SURFACE_GRAD_MAP) on sums that are exact in every order -- 320 shuffled items
 * of the unit square, weights in sixteenths, grad_out and previous content integers times 2^e, e = -120, -130, -140 -- every element
 * was the exact subnormal image, bit for bit (tests/test_surface_scale_gpu.py asserts it).  The absolute term above is therefore slack
 * on this hardware; it stays in the bound, which does not depend on it.
 * Layouts.  grad_out has the layout of the forward's out: (n, C); (B, H, W, C); (B, C, H, W) with chw != 0.  grad_attr is nverts x C
 * f32.  cgrt_interpolate_hits_grad takes host pointers, runs on a call lane and is synchronous; the *_device forms only enqueue on
 * `stream`, are concurrent on one scene, neither read nor write the prediction record or the frame hints, and use the four camera-table
 * slots and the lookup table (built by the scene's first surface call, forward or gradient) as the forward does.
 * Checks, all CGRT_E_ARG: those of the forward twin, in its order, with grad_out / grad_attr in the places of out / attr (both are
 * required): NULL pointers; n > 0x7fffffff; channels outside 1..256; the 2^40-byte bound; 4-byte alignment; the camera checks; the views
 * limits.  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0 succeeds and touches nothing.  Device forms: then every buffer's extent is
 * checked as device memory of the scene's device (d_grad_attr over nverts * channels * 4 bytes).
 * Not offered: reproducible bits from THESE entries (the *_grad_repro* entries below are the bitwise-reproducible form; it is per call:
 * a gradient accumulated over several calls is reproducible because each call is, and it equals no single larger call);
 * gradients with respect to vertex positions, rays or cameras (the weights are piecewise-smooth in them: a different
 * feature); per-triangle tables; bf16 / f16 tables; planes inside the cgrt_render_*aov* calls; enqueued-ticket forms (these calls never
 * block); the C++ host mirror. */
int cgrt_interpolate_hits_grad(CgrtScene* scene, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, const float* grad_out,
                               uint32_t channels, float* grad_attr);
int cgrt_interpolate_hits_grad_device(CgrtScene* scene, const CgrtRay* d_rays, const CgrtHit* d_hits, uint64_t n, const float* d_grad_out,
                                      uint32_t channels, float* d_grad_attr, void* stream);
int cgrt_surface_views_grad_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                                   const uint32_t* d_prim_id, const float* d_grad_out, uint32_t channels, int chw, float* d_grad_attr,
                                   void* stream);
int cgrt_surface_raycams_grad_device(CgrtScene* scene, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                                     const uint32_t* d_prim_id, const float* d_grad_out, uint32_t channels, int chw, float* d_grad_attr,
                                     void* stream);

/* Surface attributes, the bitwise-reproducible form of the gradients above.  An opt-in second form of the table
 * adjoint whose result is a pure function of the call's inputs: it does not depend on the order in which the hardware performs the
 * additions, on the mapping of lanes to items, on a permutation of the items, or on the run.  The entries above are unchanged.
 * Definition.  Validity, weights, rows and products are those of the entries above.  A valid item i contributes
 * x = fl32(w_k * g[i][c]) to element (tri[prim][k], c), rounded on its own, nothing contracted; invalid items contribute nothing and
 * their grad_out is never read.  For an element with previous content a and contributions x_1..x_m (m >= 1), n the call's item count
 * (frames: n = B * H * W):
 *   S = min(24, 38 - bitlength(3 n))                      (n <= 0x7fffffff, so S >= 5)
 *   a finite x_j is +-M_j * 2^(e'_j - 150), e'_j = max(exponent field, 1), M_j the 24-bit significand (a subnormal: no implicit bit)
 *   E = max_j e'_j,  d_j = E - e'_j
 *   T_j = +-(M_j << (S - d_j)) if d_j <= S, else +-(M_j >> (d_j - S))   (the magnitude is truncated; 0 once the shift reaches 24)
 *   I = sum_j T_j in int64                                (no overflow: |I| < 2^(24 + S) * 3 n <= 2^62)
 *   new value = fl32( fl64(a) + fl64(I) * 2^(E - 150 - S) )
 * fl64(I) is the round-to-nearest-even conversion, the scaling is exact, the sum is rounded to double and then once to float,
 * subnormals kept.  If any x_j is not finite the element becomes fl32(a + s), s = NaN if a NaN contribution is present or both +inf and
 * -inf are, else the infinity that is present.  Every NaN result is stored as the quiet NaN 0x7fc00000.  Elements without a contribution
 * are not written: rows no valid item names keep their bytes.  A contribution of +-0 still counts: the element becomes fl32(a + 0).
 * Integer addition is associative, hence the order-freedom.  The result also obeys the bound of the entries above,
 * gamma(m + 1) * S_abs + (m + 1) * 2^-126: it is a legal value of the float form.  It is per call: S depends on n, and E on the call's
 * contributions, so a gradient accumulated over several calls equals no single larger call.
 * Workspace.  cgrt_surface_grad_repro_workspace reports the bytes a call on this scene with `channels` channels needs (12 per table
 * element: nverts * channels * 12).  The device forms take it as d_workspace / workspace_bytes: device memory of the scene's device,
 * 8-byte aligned, contents need no initialisation, owned by the caller, and not to be shared by calls in flight at the same time.  With
 * separate workspaces the device forms stay concurrent on one scene; they only enqueue (a clear, two passes over the items -- integer
 * atomic max / or, then 64-bit integer atomic add -- and one pass over the table) and touch neither the prediction record nor the frame
 * hints.  cgrt_interpolate_hits_grad_repro takes host pointers, runs on a call lane, is synchronous and allocates the workspace itself.
 * Checks: those of the float twin in its order (CGRT_E_ARG); then d_workspace NULL, not 8-byte aligned or workspace_bytes too small
 * (CGRT_E_ARG; the list form with n == 0 skips these as it skips its NULL checks); then a host-only scene: CGRT_E_NO_DEVICE; n == 0
 * succeeds and touches nothing; then the extents of the device buffers, the workspace included.
 * Not offered: a form reproducible across a split into several calls; gradients with respect to positions, rays or cameras; f16 / bf16
 * tables; the C++ host mirror. */
int cgrt_surface_grad_repro_workspace(CgrtScene* scene, uint32_t channels, uint64_t* bytes);
int cgrt_interpolate_hits_grad_repro(CgrtScene* scene, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, const float* grad_out,
                                     uint32_t channels, float* grad_attr);
int cgrt_interpolate_hits_grad_repro_device(CgrtScene* scene, const CgrtRay* d_rays, const CgrtHit* d_hits, uint64_t n,
                                            const float* d_grad_out, uint32_t channels, float* d_grad_attr, void* d_workspace,
                                            uint64_t workspace_bytes, void* stream);
int cgrt_surface_views_grad_repro_device(CgrtScene* scene, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                                         const uint32_t* d_prim_id, const float* d_grad_out, uint32_t channels, int chw,
                                         float* d_grad_attr, void* d_workspace, uint64_t workspace_bytes, void* stream);
int cgrt_surface_raycams_grad_repro_device(CgrtScene* scene, const CgrtRayCamera* cams, uint32_t nviews, int W, int H,
                                           const float* d_depth, const uint32_t* d_prim_id, const float* d_grad_out, uint32_t channels,
                                           int chw, float* d_grad_attr, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* Closest-point queries: "which point of the surface is nearest to p?" for a list of points -- the other question
 * put to a triangle BVH (distance fields, snapping and registration of point clouds, collision margins, carrying per-vertex data to
 * arbitrary points).  Nothing is traced; the reference has no such function, so the definition below IS the specification.
 * Definition (bit level).  All arithmetic is f32, every operation rounded, nothing contracted.  For a query point p and a triangle with
 * a, b, c = v0, v1, v2 of its record (the f32 positions of tri[prim_id][0..2] as given to cgrt_scene_create), with
 * dot(x, y) = (x0*y0 + x1*y1) + x2*y2:
 *   ab = b-a  ac = c-a  ap = p-a  bp = p-b  cp = p-c
 *   d1 = dot(ab,ap)  d2 = dot(ac,ap)  d3 = dot(ab,bp)  d4 = dot(ac,bp)  d5 = dot(ab,cp)  d6 = dot(ac,cp)
 *   vc = d1*d4 - d3*d2   vb = d5*d2 - d1*d6   va = d3*d6 - d5*d4   e1 = d4-d3   e2 = d5-d6
 *   the first region whose test is true:
 *     A   d1 <= 0 && d2 <= 0                v = 0, w = 0,  q = a
 *     B   d3 >= 0 && d4 <= d3               v = 1, w = 0,  q = b
 *     AB  vc <= 0 && d1 >= 0 && d3 <= 0     v = d1 / (d1-d3), w = 0
 *     C   d6 >= 0 && d5 <= d6               v = 0, w = 1,  q = c
 *     AC  vb <= 0 && d2 >= 0 && d6 <= 0     v = 0, w = d2 / (d2-d6)
 *     BC  va <= 0 && e1 >= 0 && e2 >= 0     w = e1 / (e1+e2), v = 1.0f - w
 *     else                                  den = 1.0f / ((va+vb)+vc), v = vb*den, w = vc*den
 *   non-vertex regions: q.k = (a.k + ab.k*v) + ac.k*w   (the full expression, also when v or w is 0)
 *   u = (1.0f - v) - w
 *   clamp: lo.k / hi.k = min / max of a.k, b.k, c.k;  q.k = q.k < lo.k ? lo.k : (q.k > hi.k ? hi.k : q.k)
 *   r = p - q;  dist2 = dot(r, r)
 * This is Ericson's region walk plus one clamp of q to the triangle's own bounding box; the clamp is part of the definition (it is what
 * makes the tree search exact, below).  A NaN anywhere makes every region test false and dist2 NaN.
 * Result of a query.  Among the triangles with dist2 <= max_dist2 (a NaN never qualifies) the one with the smallest dist2; equal dist2
 * goes to the smaller prim_id (queries at a shared vertex tie exactly).  out[i] = {point = q, dist2, prim_id, bary = {u, v, w}}; when
 * nothing qualifies, {0,0,0, +inf, CGRT_NO_PRIM, 0,0,0}.  A non-finite p gets that miss record without a search; in a scene without meshes
 * every query misses.  Spheres are ignored.  points is n x 3 f32; max_dist2 = +inf means unbounded.
 * Exactness.  Box lower bound: dx.k = max(max(lo.k - p.k, p.k - hi.k), 0), lb2 = (dx0*dx0 + dx1*dx1) + dx2*dx2 -- dist2's operations and
 * association.  Every box of the structures is the exact min / max of its triangles' vertices, the clamped q lies in its triangle's box,
 * hence in every ancestor box: per axis |p.k - q.k| >= dx.k in the reals, and rounding, squaring and same-order summing are monotone, so
 * lb2 <= dist2 holds in f32 with no slack.  The search skips a subtree iff `lb2 > bound` is TRUE (bound = the best dist2 so far, max_dist2
 * while nothing has been accepted; strict, a NaN never culls) and therefore returns exactly what cgrt_closest_points_brute -- every
 * triangle in turn, same function, same rule; a validation path, not a fast one -- returns, bit for bit.
 * Envelope.  va, vb, vc are products of dot products: they grow as the FOURTH power of the scene's size.  With E the largest triangle
 * edge, A the smallest non-zero (2 * area)^2 = |ab x ac|^2 of the triangles, S the largest |coordinate| and M the largest |p - vertex| of
 * the query:
 *   upper edge  8 * (E * M)^2 <= FLT_MAX   (|d1..d6| <= E * M, so va, vb, vc and (va+vb)+vc do not overflow)  and  3 * M^2 <= FLT_MAX
 *   lower edge  A >= 2^12 * FLT_MIN        ((va+vb)+vc = |ab x ac|^2 in the reals: it, and va, vb, vc down to 2^-12 of it, stay normal)
 *               max(S, |p|inf) >= 2^-39    (the square of a residual of one rounding, 2^-24 of the coordinates, stays normal)
 * e.g. a unit-sized mesh with edges of 1/16 and queries within its box: about 2^-24 .. 2^+32. Inside the envelope (a) the accuracy
 * bound holds -- sqrt(dist2) and the distance to the returned triangle are within 5.66 * 2^-24 * max(1, |p|inf, S) of the float64
 * distance (tests/test_closest_cpu.py: a measurement on well-shaped meshes, not a proof.  It does not hold on slivers: (va+vb)+vc is
 * |ab x ac|^2 computed from products of dot products, and where that is small against 2^-24 * (E * M)^2 the interior region's quotients
 * carry no correct digit.  On a triangle with edges of 0.3 and 3e-8, inside this envelope, the defined point was 0.017 from the nearest
 * one, 5.4e4 times the bound -- tools/fuzz_queries.py, seed 6606, iteration 3; every path returns those bytes) -- and (b) multiplying every position and every query by 2^k is an exact symmetry: the same
 * prim_id and bary bits, point * 2^k, dist2 * 2^2k.  The upper edge is a proof.  The lower one is a margin: a query whose weight towards
 * an edge is non-zero but below 2^-12 can have that va, vb or vc rounded as a subnormal.  Outside the envelope the result is still the
 * defined one, bit for bit, on every path, but can be far from the geometric answer: on a unit cube scaled by 2^33 about 5 % of
 * unbounded queries miss (every dist2 NaN), from 2^60 a fifth of the records have dist2 = +inf (which qualifies under max_dist2 = +inf),
 * and on a 1 848-triangle unit blob scaled by 2^-31 only 65 % of the queries are still covariant (DESIGN.md 5.20 has the table).
 * The search uses the structure every scene has (the reference tree, the in-leaf accelerators, linear leaves under
 * cgrt_set_leaf_accel(0)); the walk settings (cgrt_scene_set_walk, cgrt_set_fast_tree, cgrt_set_kernel_shape) do not change it.
 * Streams.  The host forms (host pointers, synchronous) run on a call lane like cgrt_occluded: any number of threads may query one scene
 * at once.  cgrt_closest_points_device reads no host array: it only enqueues on `stream` (NULL = default stream), asynchronously, like
 * cgrt_intersect_batch_device, and neither reads nor writes the prediction record or the frame hints.  Only records 0..n-1 are written.
 * cgrt_debug_closest_work: a separate counting launch of the same search (never part of a timed region); out2 = {node steps, triangles
 * evaluated}, summed over the n queries.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene; NULL points or out with n > 0; n > 0x7fffffff; max_dist2
 * NaN or negative; (device form) a pointer not 4-byte aligned.  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0 succeeds and touches
 * nothing.  Device form: then d_points (n * 12 bytes) and d_out (n * 32 bytes) checked as device memory of the scene's device, as
 * cgrt_shade_rays_device checks its buffers.
 * Not offered: sphere primitives; attribute interpolation at the closest point (k nearest and a per-query radius: "Neighbour queries")
 * (attr[tri[prim_id]] weighted by bary is a plain gather); the fast tree as a search structure; enqueued-ticket forms (the device form
 * never blocks); the C++ host mirror (the reference has no such function). */
typedef struct CgrtClosest {
    float point[3];   /* q, the nearest point of the triangle                   */
    float dist2;      /* |p - q|^2 as defined above; +inf on a miss             */
    uint32_t prim_id; /* CGRT_NO_PRIM on a miss                                 */
    float bary[3];    /* {u, v, w}: the weights of v0, v1, v2                   */
} CgrtClosest;
int cgrt_closest_points(CgrtScene* scene, const float* points, uint64_t n, float max_dist2, CgrtClosest* out);
int cgrt_closest_points_device(CgrtScene* scene, const float* d_points, uint64_t n, float max_dist2, CgrtClosest* d_out, void* stream);
int cgrt_closest_points_brute(CgrtScene* scene, const float* points, uint64_t n, float max_dist2, CgrtClosest* out);
int cgrt_debug_closest_work(CgrtScene* scene, const float* points, uint64_t n, float max_dist2, uint64_t* out2);

/* Crossing queries: "which surfaces does this ray pass through -- all of them, in order?"  The count_intersections
 * / list_intersections pair of other ray-casting scene interfaces: thickness and x-ray images, depth peeling, transparency, inside /
 * outside tests.  The reference has no such function; the definition below IS the specification.
 * Definition.  For a ray r = (o, d, t_in), triangle k is a CROSSING iff the reference's intersectRayWithTriangle (ray_tracing.cpp:86-114),
 * called on a fresh copy of r, returns true; its parameter t_k is the ray.t that call leaves.  With on = dot(o, n), den = dot(d, n) of the
 * triangle's plane (n, D) as trianglePlane gives it: onp = (on == D); tt = onp ? 0 : (D - on) / den; p = o + d * tt; inside =
 * pointInTriangle(v0, v1, v2, n, p) (three `>= 0` tests); crossing iff
 *     inside && (onp || (den != 0 && !(tt < 0) && !(tt >= t_in))),    t_k = tt.
 * An origin-on-plane acceptance has t = 0 and ignores t_in, as upstream does (ray_tracing.cpp:43-47).  A crossing is a pure function of
 * (ray, triangle): no tree, no visiting order, no running minimum enters.  The ray is taken as given: a segment sets t to its length, the
 * direction need not be of unit length.  Spheres are ignored.  A ray's crossings are ordered by t compared as floats (-0 equals +0), equal
 * t going to the smaller prim_id: a total order, so every output byte is determined.
 * Consequences.
 *   C1  On a scene without spheres, for a ray with no origin-on-plane acceptance, the first crossing is cgrt_intersect_brute_batch(mesh <
 *       0)'s t (bit pattern) and prim_id.  It is NOT always cgrt_intersect_batch's hit: the reference's tree walk misses hits (SURVEY.md
 *       F4); the list does not.
 *   C2  A ray through an edge shared by two triangles crosses both (pointInTriangle uses `>= 0`), so the parity of the count along one ray
 *       is only almost always the inside test.
 * Slots.  CgrtCrossing = {t, prim_id}, 8 bytes.  cgrt_count_crossings* write counts[i] = the number of crossings of ray i.  In the list
 * calls ray i owns the records [offsets[i], offsets[i + 1]) of out (offsets: n + 1 entries; the exclusive prefix sums of a count call give
 * the full list, CSR style) or, with offsets == NULL, the records [i * k, (i + 1) * k): exactly one of offsets and k > 0 must be given.  A
 * slot of s records receives the first min(s, count) crossings in order and {+inf, CGRT_NO_PRIM} in its remaining entries; counts[i] (may
 * be NULL in the list calls) is always the full number of crossings.  Every record of every slot is written, nothing outside the slots.
 * The host forms check that offsets start at 0, do not decrease and end <= capacity.  The device form never reads the offsets on the host:
 * the kernel treats a decreasing pair as an empty slot and clamps both ends to capacity, so no offset table makes it write outside the
 * first `capacity` records of d_out (slots that overlap are written by several rays, in no defined order).
 * Search.  One ray per lane over the structure every scene has (the reference tree, the in-leaf accelerators, linear leaves under
 * cgrt_set_leaf_accel(0)) with the conservative box test alone, bounded by t_in; while a slot is full and no count is asked for, the bound
 * shrinks to the largest t kept (non-strictly: an equal-t smaller prim_id still arrives).  The result is what cgrt_list_crossings_brute --
 * every triangle in turn, same function, same slot rule; a validation path -- returns, byte for byte.  Where the conservative argument does
 * not hold the search is not used: a scene with a wild leaf or a non-finite vertex (cgrt_scene_build_info [1] > 0 or [2] == 0) runs the
 * brute-force kernel for the whole call, and a ray outside the box test's envelope (non-finite or beyond 2^+-40, NaN t) tests every
 * triangle itself.  The walk settings (cgrt_scene_set_walk, cgrt_set_fast_tree, cgrt_set_kernel_shape) do not enter.
 * Envelope.  trianglePlane normalises cross(v1-v0, v2-v0), and |cross|^2 = (2 * area)^2 grows as the FOURTH power of the scene's size.
 * With E, A, S as in "Closest-point queries" and M the largest |o - vertex|: inside  8 * (E * M)^2 <= FLT_MAX,  A >= 2^12 * FLT_MIN
 * and  max(S, |o|inf) >= 2^-39, multiplying every position, every origin and every t by 2^k -- the directions kept -- is an exact
 * symmetry: the same counts, the same prim_id order, every t_k * 2^k.  For crossings NEITHER edge is a proof.  |cross|^2 <= E^4 and the
 * plane's D and dot(o, n) are covered, but pointInTriangle multiplies an edge by |p - vertex| with p = o + d * tt the hit of the PLANE,
 * which for a grazing ray lies arbitrarily far from the triangle: M does not bound it.  (Such a product overflows only where p is far
 * outside the triangle, where the three tests then fail through inf - inf = NaN as they fail in the reals; the tests hold the envelope
 * to the definition on their own rays, they do not prove it.)  Outside, the records are still the defined ones, byte for byte, on every
 * path, but need not mean anything: a |cross|^2 that overflows gives n = (0, 0, 0), D = 0, and the origin-on-plane rule then accepts
 * EVERY ray at t = 0 (from 2^33 on, a unit cube is crossed twelve times by almost every ray; a slot is insertion-sorted, so such lists
 * cost count^2); one that underflows gives a NaN normal and the triangle is never crossed.
 * cgrt_debug_crossing_work: a separate counting launch of the count search (never part of a timed region); out2 = {node steps, triangles
 * evaluated}, summed over the n rays.
 * Streams.  The host forms (host pointers, synchronous) run on a call lane like cgrt_closest_points: any number of threads may query one
 * scene at once.  The device forms read no host array and only enqueue on `stream` (NULL = default stream); they are concurrent on one
 * scene and neither read nor write the prediction record or the frame hints.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene; NULL rays or result array (counts of the count calls, out
 * of the list calls, out2) with n > 0; n > 0x7fffffff; (list calls) both or neither of offsets and k > 0; capacity above 2^37 records;
 * with k, n * k > capacity; (host list calls, n > 0) offsets not starting at 0, decreasing, or ending above capacity; (device forms) a
 * pointer not aligned to its element (4 bytes; 8 for d_offsets).  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0 succeeds and touches
 * nothing.  Device forms: then d_rays (n * 28 bytes), d_offsets ((n + 1) * 8), d_out (capacity records with offsets, n * k with k) and
 * d_counts (n * 4) checked as device memory of the scene's device, as cgrt_shade_rays_device checks its buffers.
 * Not offered: the fast tree as the search structure (there is no closest-first pruning for it to win on: one path); quad / 16-lane
 * shapes; spheres; normals or material ids per record (tri_mesh[prim_id] is a gather; barycentrics come from cgrt_hit_barycentrics_device
 * on gathered rays); frame / camera forms; enqueued-ticket forms (the device forms never block); the C++ host mirror. */
typedef struct CgrtCrossing {
    float t;          /* the crossing's parameter; +inf in an unused entry      */
    uint32_t prim_id; /* CGRT_NO_PRIM in an unused entry                        */
} CgrtCrossing;
int cgrt_count_crossings(CgrtScene* scene, const CgrtRay* rays, uint64_t n, uint32_t* counts);
int cgrt_count_crossings_device(CgrtScene* scene, const CgrtRay* d_rays, uint64_t n, uint32_t* d_counts, void* stream);
int cgrt_list_crossings(CgrtScene* scene, const CgrtRay* rays, uint64_t n, const uint64_t* offsets, uint32_t k, CgrtCrossing* out,
                        uint64_t capacity, uint32_t* counts);
int cgrt_list_crossings_device(CgrtScene* scene, const CgrtRay* d_rays, uint64_t n, const uint64_t* d_offsets, uint32_t k, CgrtCrossing* d_out,
                               uint64_t capacity, uint32_t* d_counts, void* stream);
int cgrt_list_crossings_brute(CgrtScene* scene, const CgrtRay* rays, uint64_t n, const uint64_t* offsets, uint32_t k, CgrtCrossing* out,
                              uint64_t capacity, uint32_t* counts);
int cgrt_debug_crossing_work(CgrtScene* scene, const CgrtRay* rays, uint64_t n, uint64_t* out2);

/* Neighbour queries: "which triangles lie within r of p -- all of them, nearest first?" and "which are the k
 * nearest?" for a list of points -- the point-side twin of the crossing queries: contact and proximity sets, neighbourhoods for smoothing
 * and robust normals, projection with fallbacks, per-particle radii.  The reference has no such function; the definition below IS the
 * specification.
 * Definition.  For a query point p with bound r2, triangle k is a NEIGHBOUR iff `dist2_k <= r2` is true, dist2_k being exactly the dist2
 * of "Closest-point queries": the same operations, the same clamp, a pure function of (p, triangle) -- no tree, no visiting order, no
 * running minimum enters.  A NaN dist2 never qualifies.  A dist2 of +inf (a finite point and finite vertices whose squares overflow: far
 * outside the envelope) qualifies under r2 = +inf, as `inf <= inf` is true, and under no other bound; all such records tie on dist2, so
 * they follow the finite ones in prim_id order, and a full slot whose largest dist2 is +inf culls nothing.  Spheres are ignored.
 * Bound.  r2 = radius2 ? radius2[i] : max_dist2 (radius2: n f32, or NULL).  The scalar max_dist2 is checked as cgrt_closest_points checks
 * it (NaN or negative: CGRT_E_ARG; +inf: unbounded), also where radius2 is given.  A per-query radius2[i] for which `radius2[i] >= 0` is
 * false (NaN or negative) gives that query no neighbours: this is decided in the kernel, identically in the host and the device forms;
 * the host forms do not scan the array.  A non-finite p has no neighbours; in a scene without meshes no query has any.
 * Order.  A query's neighbours are ordered by dist2 compared as floats, equal dist2 going to the smaller prim_id: a total order, so
 * every output byte is determined.
 * Slots.  CgrtNeighbor = {dist2, prim_id}, 8 bytes.  The rule is exactly that of "Crossing queries".  cgrt_count_neighbors* write
 * counts[i] = the number of neighbours of query i.  In the list calls query i owns the records [offsets[i], offsets[i + 1]) of out
 * (offsets: n + 1 entries; the exclusive prefix sums of a count call give the full list, CSR style) or, with offsets == NULL, the records
 * [i * k, (i + 1) * k): exactly one of offsets and k > 0 must be given.  A slot of s records receives the first min(s, count) neighbours
 * in order and {+inf, CGRT_NO_PRIM} in its remaining entries; counts[i] (may be NULL in the list calls) is always the full number of
 * neighbours.  Every record of every slot is written, nothing outside the slots.  The host forms check that offsets start at 0, do not
 * decrease and end <= capacity.  The device form never reads the offsets on the host: the kernel treats a decreasing pair as an empty
 * slot and clamps both ends to capacity, so no offset table makes it write outside the first `capacity` records of d_out (slots that
 * overlap are written by several queries, in no defined order).
 * Consequences.
 *   N1  With k = 1 and radius2 == NULL, record i is {dist2, prim_id} of cgrt_closest_points for the same max_dist2, bit for bit; a miss
 *       is {+inf, CGRT_NO_PRIM}.
 *   N2  With k > 0 and counts == NULL the call is "the k nearest within r2".
 *   N3  cgrt_count_neighbors, the exclusive prefix sums of its counts, then cgrt_list_neighbors with those offsets: the full CSR
 *       neighbour list.
 * Search.  One query per lane over the structure cgrt_closest_points walks (the reference tree, the in-leaf accelerators, linear leaves
 * under cgrt_set_leaf_accel(0)) with its box lower bound lb2; a subtree is skipped iff `lb2 > bound` is TRUE.  The bound is r2; while a
 * slot is full and no count is asked for it shrinks to the largest dist2 kept (non-strictly: an equal-dist2 smaller prim_id still
 * arrives).  Because lb2 <= dist2 holds in f32 with no slack for every triangle under a box ("Closest-point queries", Exactness), the
 * result is what cgrt_list_neighbors_brute -- every triangle in turn, same function, same slot rule; a validation path -- returns, byte
 * for byte, whatever the visiting order.  Non-finite vertices need no other path: a NaN lb2 never culls, and a NaN dist2 never
 * qualifies.  The walk settings (cgrt_scene_set_walk, cgrt_set_fast_tree, cgrt_set_kernel_shape) do not enter.  A slot is kept sorted
 * by insertion: a full list of c neighbours costs up to c^2 / 2 record moves.  Envelope and accuracy are those of dist2
 * ("Closest-point queries"): within 5.66 * 2^-24 * max(1, |p|inf, S) of the radius in distance, membership can differ from the float64
 * answer (tests/test_neighbors_cpu.py).
 * cgrt_debug_neighbor_work: a separate counting launch (never part of a timed region); out2 = {node steps, triangles evaluated}, summed
 * over the n queries.  k = 0: the count search; k > 0: the k-nearest search (k records per query, no counts: the shrinking bound).
 * Streams.  The host forms (host pointers, synchronous) run on a call lane like cgrt_closest_points: any number of threads may query one
 * scene at once.  The device forms read no host array and only enqueue on `stream` (NULL = default stream); they are concurrent on one
 * scene and neither read nor write the prediction record or the frame hints.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene; NULL points or result array (counts of the count calls,
 * out of the list calls, out2) with n > 0; n > 0x7fffffff; max_dist2 NaN or negative; (list calls) both or neither of offsets and k > 0;
 * capacity above 2^37 records; with k, n * k > capacity; (host list calls, n > 0) offsets not starting at 0, decreasing, or ending above
 * capacity; (device forms) a pointer not aligned to its element (4 bytes; 8 for d_offsets).  Then a host-only scene: CGRT_E_NO_DEVICE.
 * n == 0 succeeds and touches nothing.  Device forms: then d_points (n * 12 bytes), d_radius2 (n * 4), d_offsets ((n + 1) * 8), d_out
 * (capacity records with offsets, n * k with k) and d_counts (n * 4) checked as device memory of the scene's device, as
 * cgrt_shade_rays_device checks its buffers.
 * Not offered: the closest point and the barycentrics per record (cgrt_closest_points has them for the nearest; for the others they are
 * a function of (p, prim_id)); spheres; a per-query k (offsets give per-query slot sizes); grid forms; enqueued-ticket forms (the device
 * forms never block); the C++ host mirror. */
typedef struct CgrtNeighbor {
    float dist2;      /* |p - q|^2 as "Closest-point queries" defines it; +inf in an unused entry */
    uint32_t prim_id; /* CGRT_NO_PRIM in an unused entry                                           */
} CgrtNeighbor;
int cgrt_count_neighbors(CgrtScene* scene, const float* points, uint64_t n, const float* radius2, float max_dist2, uint32_t* counts);
int cgrt_count_neighbors_device(CgrtScene* scene, const float* d_points, uint64_t n, const float* d_radius2, float max_dist2, uint32_t* d_counts,
                                void* stream);
int cgrt_list_neighbors(CgrtScene* scene, const float* points, uint64_t n, const float* radius2, float max_dist2, const uint64_t* offsets,
                        uint32_t k, CgrtNeighbor* out, uint64_t capacity, uint32_t* counts);
int cgrt_list_neighbors_device(CgrtScene* scene, const float* d_points, uint64_t n, const float* d_radius2, float max_dist2,
                               const uint64_t* d_offsets, uint32_t k, CgrtNeighbor* d_out, uint64_t capacity, uint32_t* d_counts, void* stream);
int cgrt_list_neighbors_brute(CgrtScene* scene, const float* points, uint64_t n, const float* radius2, float max_dist2, const uint64_t* offsets,
                              uint32_t k, CgrtNeighbor* out, uint64_t capacity, uint32_t* counts);
int cgrt_debug_neighbor_work(CgrtScene* scene, const float* points, uint64_t n, const float* radius2, float max_dist2, uint32_t k,
                             uint64_t* out2);

/* Signed distance and occupancy: "how far is this point from the surface, and is it inside?" -- for point lists
 * and for regular grids (a mesh turned into an SDF volume).  The compute_signed_distance / compute_occupancy pair of other ray-casting
 * scene interfaces, meaningful for WATERTIGHT meshes.  One fused kernel: no rays, counts or closest records are written in between.
 * Definition.  For a finite point p, with the parameters' max_dist2 and directions dirs[0 .. ndirs) (ndirs == 0: the three rows of
 * CGRT_SDF_DEFAULT_DIRS):
 *   C      = the cgrt_closest_points record of p under max_dist2
 *   c_j    = the cgrt_count_crossings count of the ray {origin p, direction dirs[j], t = +inf}
 *   inside = (number of odd c_j) > ndirs / 2
 *   s      = sqrt(C.dist2), IEEE, correctly rounded (+inf stays +inf);   sdf = inside ? -s : s
 * so beyond max_dist2 the value is +-inf with the sign of the vote, and dist2 == 0 inside gives -0.0.  These are, bit for bit, the bytes
 * the Python compositions Scene.signed_distance_tensor and Scene.inside_tensor produce for finite points.  A non-finite p gets sdf = +inf,
 * inside = 0 without a search; in a scene without meshes every point gets the same.  Spheres are ignored, as in both underlying queries.
 * Outputs.  sdf (f32) and inside (u8, 0 or 1), n of each; either may be NULL, not both.  With sdf == NULL (occupancy only) the
 * closest-point search is not run.  Nothing outside records 0..n-1 is written.
 * Grid.  Point (ix, iy, iz) is p.c = origin.c + (float)i_c * spacing.c -- the product rounded, then the sum, nothing contracted -- and its
 * result is at index (iz * ny + iy) * nx + ix: a contiguous (nz, ny, nx) array with x fastest.  The value is what the list form returns
 * for that point.  Each dim is 1..2^24, nx * ny * nz <= 0x7fffffff, origin and spacing finite (zero or negative spacing is allowed).
 * Search.  One point per lane.  First the closest-point search of cgrt_closest_points keeping only the bound (the equal-dist2 tie rule
 * does not affect the value), then per direction the count search of cgrt_count_crossings keeping only the parity.  Once more than
 * ndirs / 2 walks agree (odd or even) the remaining walks are skipped; the outputs do not depend on this.  Where the conservative box
 * argument does not hold the parity walks do what the crossing entries do: on a scene with a wild leaf or a non-finite vertex they test
 * every triangle, and a ray outside the box test's envelope scans every record itself.  The closest search needs no such rule.
 * Envelope and meaning.  `inside` is a statement about geometry for CLOSED meshes only (every directed edge matched once by its reverse
 * after welding equal positions): there it equals |winding number| > 0.5 and |sdf| the float64 distance within 5.66 * 2^-24 * max(1,
 * |p|inf, S) for every point farther than 1e-4 extents from the surface (tests/test_point_scale_cpu.py, _gpu.py: a cube and a curved
 * 20 000-triangle mesh).  On an open mesh the vote is still the defined one, and means nothing.  The envelope is the intersection of
 * those of the two underlying queries with M the largest |p - vertex| ("Closest-point queries", "Crossing queries"): inside it,
 * multiplying every position, every point and the grid's origin and spacing by 2^k (max_dist2 by 2^2k) leaves `inside` unchanged and
 * multiplies sdf by 2^k, exactly; outside it the bytes are still the defined ones but the vote flips (for 23-27 % of the points of
 * unit-sized meshes of a few thousand triangles scaled by 2^-30, for 18 % on a unit cube scaled by 2^32).
 * cgrt_debug_sdf_work: a separate counting launch (never part of a timed region), want_sdf != 0 including the closest search; out5 =
 * {closest node steps, closest triangles evaluated, crossing node steps, crossing triangles evaluated, direction walks run}, summed over
 * the n points.
 * Streams.  The host forms (host pointers, synchronous) run on a call lane like cgrt_closest_points: any number of threads may query one
 * scene at once.  The device forms read no host array behind the call (the parameters travel in the kernel arguments) and only enqueue on
 * `stream` (NULL = default stream); they are concurrent on one scene and neither read nor write the prediction record or the frame hints.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene; NULL points (or grid) with n > 0; both outputs NULL (out5
 * of the work entry); n > 0x7fffffff, or the grid limits above; bad parameters (max_dist2 NaN or negative; ndirs even or above 7; a
 * direction with a non-finite component or all zero); (device forms) d_points or d_sdf not 4-byte aligned.  Then a host-only scene:
 * CGRT_E_NO_DEVICE.  n == 0 succeeds and touches nothing.  Device forms: then d_points (n * 12 bytes), d_sdf (n * 4) and d_inside (n)
 * checked as device memory of the scene's device, as cgrt_shade_rays_device checks its buffers.
 * Not offered: one parity ray per grid row (the crossing arithmetic depends on the origin, so it would not give these bytes);
 * spheres; gradients; enqueued-ticket forms (the device forms never block); the C++ host mirror.  (Signs
 * for open meshes: "Winding numbers" below.) */
#define CGRT_SDF_MAX_DIRS 7
#define CGRT_SDF_DEFAULT_NDIRS 3
#define CGRT_SDF_DEFAULT_DIRS \
    { {0.5310871f, 0.2178203f, 0.8188417f}, {-0.3319057f, 0.9047763f, -0.2670293f}, {0.6834621f, -0.5712349f, -0.4544671f} }
typedef struct CgrtSdfParams { /* NULL = all defaults */
    float max_dist2;           /* as cgrt_closest_points: +inf = unbounded; NaN or negative -> CGRT_E_ARG           */
    uint32_t ndirs;            /* 0 = the three default directions; otherwise odd, 1..7                             */
    float dirs[7][3];          /* read when ndirs > 0: every component finite, no all-zero row                      */
} CgrtSdfParams;
typedef struct CgrtGrid {
    float origin[3];
    float spacing[3];
    uint32_t dims[3]; /* nx, ny, nz */
} CgrtGrid;
int cgrt_signed_distance(CgrtScene* scene, const float* points, uint64_t n, const CgrtSdfParams* params, float* sdf, uint8_t* inside);
int cgrt_signed_distance_device(CgrtScene* scene, const float* d_points, uint64_t n, const CgrtSdfParams* params, float* d_sdf,
                                uint8_t* d_inside, void* stream);
int cgrt_signed_distance_grid(CgrtScene* scene, const CgrtGrid* grid, const CgrtSdfParams* params, float* sdf, uint8_t* inside);
int cgrt_signed_distance_grid_device(CgrtScene* scene, const CgrtGrid* grid, const CgrtSdfParams* params, float* d_sdf, uint8_t* d_inside,
                                     void* stream);
int cgrt_debug_sdf_work(CgrtScene* scene, const float* points, uint64_t n, const CgrtSdfParams* params, int want_sdf, uint64_t* out5);
/* How the grid forms map lanes to grid points (process-wide; a measuring switch, the results are the same bytes): 0 = each wave takes a
 * 4 x 4 x 4 brick of grid points, a block two bricks next to each other in x (the default); 1 = lanes follow the result index. */
int cgrt_debug_set_sdf_grid_mapping(int linear);

/* Winding numbers: a robust inside / outside for meshes that are NOT watertight -- for point lists and for
 * regular grids.  The generalised winding number of the scene's triangles about a point is the sum of their signed solid angles over
 * 4 pi: +-1 inside a closed mesh (the sign is its orientation), 0 outside, and it degrades smoothly near holes, self-intersections and
 * duplicated faces, where the parity vote of cgrt_signed_distance means nothing.  An exact all-triangles form (brute) and a hierarchical
 * form (tree) that replaces far clusters of triangles by one dipole.
 * Definition.  Everything is f32, every operation rounded on its own (nothing contracted), sums associated as the parentheses say.  For a
 * finite point p and a triangle record {v0, v1, v2} (the vertices in the caller's order):
 *   ra = v0 - p, rb = v1 - p, rc = v2 - p                      (componentwise)
 *   la = sqrtf((ra.x * ra.x + ra.y * ra.y) + ra.z * ra.z), lb and lc alike
 *   u  = rb x rc:  u.x = rb.y * rc.z - rb.z * rc.y,  u.y = rb.z * rc.x - rb.x * rc.z,  u.z = rb.x * rc.y - rb.y * rc.x
 *   num = (ra.x * u.x + ra.y * u.y) + ra.z * u.z
 *   ab = (ra.x * rb.x + ra.y * rb.y) + ra.z * rb.z,  bc = (rb.x * rc.x + ..) + ..,  ca = (rc.x * ra.x + ..) + ..
 *   den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb
 *   omega = 2.0f * atan2f(num, den)                             (van Oosterom and Strackee)
 * Brute form: acc = 0; acc = acc + omega_k for the records k = 0 .. ntris - 1 in RECORD ORDER (the order of the device's triangle array:
 * cgrt_debug_get_winding_tree reports it); w = acc * (1 / (4 pi)), the constant rounded to f32.
 * Tree form.  The records carry an implicit 8-ary cluster tree: level 0's cluster i covers records [8 i, min(8 i + 8, ntris)), level L's
 * cluster i the level-(L - 1) clusters 8 i .. 8 i + 7; level L has ceil(ntris / 8^(L+1)) clusters and the top level is the first with at
 * most 8 (at most 9 levels).  A cluster is 32 bytes {c.xyz, r2, n.xyz, 0}: c the area-weighted mean of its triangles' centroids (their
 * plain mean when the area sum is 0 or not finite), n the sum of their area vectors (v1 - v0) x (v2 - v0) / 2, both evaluated in double and
 * rounded once; r2 the largest ((dx * dx + dy * dy) + dz * dz), d = vertex - c, over the vertices of its records, evaluated in f32 in that
 * association (NaN if one of them is).  The walk is depth-first from the top level, clusters and children in index order, into the same
 * accumulator acc (0 at the start), with d = c - p and d2 = (d.x * d.x + d.y * d.y) + d.z * d.z:
 *   the cluster is FAR iff  d2 > beta2 * r2  is TRUE (beta2 = beta * beta, rounded once on the host; a NaN therefore opens the cluster)
 *   far:                acc = acc + ((n.x * d.x + n.y * d.y) + n.z * d.z) / (d2 * sqrtf(d2))      (the cluster's dipole; IEEE division)
 *   near, level 0:      acc = acc + omega_k for its records in record order
 *   near, level > 0:    its children are walked
 * and w = acc * (1 / (4 pi)) as above.  With beta = +inf no cluster is far (inf * 0 is a NaN) and the walk performs the brute form's
 * additions in the brute form's order: it returns the brute form's bytes.  inside = fabsf(w) > threshold, for every point.
 * A non-finite p gets w = 0 without a walk; in a scene without meshes every point gets 0.  Spheres are ignored.  A scene with non-finite
 * vertices may give NaN (inside = 0 then); no call faults or hangs over it.
 * Envelope.  num, the four terms of den and the dipole's d2 * sqrtf(d2) are products of THREE lengths: they grow as the third power of
 * the scene's size.  With M the largest and m the smallest |p - vertex| of the point, E the largest and e the smallest non-zero triangle
 * edge, a the sum of the triangle areas and D the diagonal of the scene's box:
 *   upper edge  8 * M^3 <= FLT_MAX         (every product and partial sum of num and den is at most 4 M^3; d2 * sqrtf(d2) <= M^3)
 *               2 * a * M <= FLT_MAX       (|n| <= a: the dipole's numerator)   and   2 * beta^2 * D^2 <= FLT_MAX   (beta2 * r2 finite)
 *               E^2 * M <= 2^-18 * FLT_MAX (|num| <= E^2 * M: atan2f, the one operation not pinned here, sees no argument pair it must screen)
 *   lower edge  m^3 >= FLT_MIN             ((la * lb) * lc, the one term of den nothing cancels, stays normal)
 *               e^3 >= 2^12 * FLT_MIN      (num is six tetrahedron volumes: one as small as the smallest edge in all its extents, and
 *                                           products down to 2^-12 of it, stay normal; a far cluster has d2 * sqrtf(d2) > e^3 / 8)
 * e.g. a unit-sized mesh with edges between 1/64 and 1/8 and points within a hundred extents: about 2^-32 .. 2^+35.  Inside the envelope multiplying
 * every position and every point (a grid's origin and spacing) by 2^k is an exact symmetry: the cluster tree is the power-of-two image
 * (c * 2^k; r2 and n * 2^2k), every far decision and so every work counter is the same, and w is the SAME float, bit for bit, where
 * atan2f(2^j y, 2^j x) == atan2f(y, x) -- which held for every point tested on the device and holds for numpy's float32 arctan2 within
 * the third upper line.  The first upper lines are a proof; the third and the second lower line are margins (a point in a triangle's
 * plane has num = 0 in the reals, and a product far below e^3 is then rounded as a subnormal).  The record order is the BVH builder's and
 * is not part of this envelope: on meshes of many small triangles it changes earlier (a 16 311-triangle mesh with slivers: below 2^-20
 * and above 2^33).  Outside the envelope the bytes are still the defined ones on every path -- the tree form at beta = +inf returns the
 * brute form's bytes, inf and NaN sums included, and the counters stay those of the definition -- but w loses its meaning silently:
 * below, num and den underflow and w tends to 0 (unit-sized meshes: errors of 4e-5 at 2^-40, 4e-3 at 2^-42; at 2^-70 every point inside
 * a unit cube reads 0); above, errors of 0.1 from 2^42 on, and NaN once the sums overflow (every point at 2^62; inside = 0 for a NaN).
 * DESIGN.md 5.25 has the table; tests/test_query_scale_cpu.py and _gpu.py hold both edges.
 * Parameters.  beta >= 1 (the opening ratio: a cluster is replaced by its dipole from beta cluster radii on; larger = more exact, more
 * work; +inf allowed), 0 = CGRT_WINDING_DEFAULT_BETA; NaN or anything else below 1 -> CGRT_E_ARG.  threshold: taken as given (a NaN
 * makes every inside 0).  params == NULL: {2.0f, 0.5f}.  The brute entry reads only the threshold.
 * Accuracy (DESIGN.md 5.25 has the table): against the float64 sum over every triangle the tree form's largest error at beta = 2 was
 * 1.8e-2 .. 3.2e-2 on the test meshes (6.3e-2 on an 800 000-triangle mesh), 2e-3 .. 1.3e-2 at beta = 4, and no verdict |w| > 0.5 differed
 * among the points with ||w| - 0.5| >= 0.05.
 * Outputs.  w (f32) and inside (u8, 0 or 1), n of each; either may be NULL, not both.  Nothing outside records 0..n-1 is written.
 * Grid.  CgrtGrid and the result order of cgrt_signed_distance_grid: point (ix, iy, iz) = origin + (float)i * spacing per component (the
 * product rounded, then the sum), result at (iz * ny + iy) * nx + ix; the value is what the list form returns for that point.
 * The tree is built on the host by the scene's first winding call (any entry below but the brute one), under the scene's lock, uploaded
 * once and freed with the scene; cgrt_device_bytes includes it from then on; cgrt_debug_layout_hash does not change (no existing array
 * is touched).  With cgrt_set_leaf_accel(0) the record order inside a leaf is the reference's scan order, the clusters get fat and the
 * walk does more work; the answers stay within the same bounds.
 * cgrt_debug_winding_work: a separate counting launch of the tree form; out3 = {clusters tested, dipoles taken, triangles evaluated},
 * summed over the n points.  The far decisions are f32 arithmetic in the order above, so the counters are reproducible on a CPU.
 * cgrt_debug_get_winding_tree (works on host-only scenes, building the tree if need be): *nlevels receives the number of levels;
 * level_offsets (NULL, or 10 entries are always enough) nlevels + 1 entries, level L's clusters are [level_offsets[L], level_offsets[L+1]);
 * clusters (NULL, or 8 floats per cluster) the array; record_prims (NULL, or one entry per triangle) the prim_id of every record in
 * record order.  Sizes first: call with NULL arrays, or compute them from the triangle count.
 * Streams.  The host forms (host pointers, synchronous) run on a call lane like cgrt_closest_points: any number of threads may query one
 * scene at once.  The device forms read no host array behind the call (the parameters travel in the kernel arguments) and only enqueue
 * on `stream` (NULL = default stream); the first of them on a scene uploads the tree before it enqueues.  They are concurrent on one
 * scene and neither read nor write the prediction record or the frame hints.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene; NULL points (or grid) with n > 0; both outputs NULL (out3
 * of the work entry); n > 0x7fffffff, or the grid limits of cgrt_signed_distance_grid; bad beta; (device forms) d_points or d_w not
 * 4-byte aligned.  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0 succeeds and touches nothing.  Device forms: then d_points (n * 12
 * bytes), d_w (n * 4) and d_inside (n) checked as device memory of the scene's device.
 * Not offered: the winding sign fused into the signed-distance kernel (whose registers must not move: Scene.signed_distance_winding_tensor
 * composes the two); higher-order expansions than the dipole; gradients; spheres; enqueued-ticket forms (the device forms never block);
 * the C++ host mirror; a Morton re-sort of the records. */
#define CGRT_WINDING_DEFAULT_BETA 2.0f
#define CGRT_WINDING_DEFAULT_THRESHOLD 0.5f
typedef struct CgrtWindingParams { /* NULL = all defaults */
    float beta;                    /* 0 = CGRT_WINDING_DEFAULT_BETA; otherwise >= 1 (+inf allowed); NaN or below 1 -> CGRT_E_ARG */
    float threshold;               /* inside = fabsf(w) > threshold                                                          */
} CgrtWindingParams;
int cgrt_winding_numbers(CgrtScene* scene, const float* points, uint64_t n, const CgrtWindingParams* params, float* w, uint8_t* inside);
int cgrt_winding_numbers_device(CgrtScene* scene, const float* d_points, uint64_t n, const CgrtWindingParams* params, float* d_w,
                                uint8_t* d_inside, void* stream);
int cgrt_winding_numbers_grid(CgrtScene* scene, const CgrtGrid* grid, const CgrtWindingParams* params, float* w, uint8_t* inside);
int cgrt_winding_numbers_grid_device(CgrtScene* scene, const CgrtGrid* grid, const CgrtWindingParams* params, float* d_w, uint8_t* d_inside,
                                     void* stream);
int cgrt_winding_numbers_brute(CgrtScene* scene, const float* points, uint64_t n, const CgrtWindingParams* params, float* w, uint8_t* inside);
int cgrt_debug_winding_work(CgrtScene* scene, const float* points, uint64_t n, const CgrtWindingParams* params, uint64_t* out3);
int cgrt_debug_get_winding_tree(CgrtScene* scene, float* clusters, uint32_t* level_offsets, uint32_t* nlevels, uint32_t* record_prims);

/* Surface sampling: points ON the scene's triangles, spread by area -- the producer the point queries above
 * lack ("sample A, cgrt_closest_points on B" is a mesh-to-mesh distance; "sample, make rays, cgrt_occluded" a hemisphere integral).
 * Sample j is a function of (scene, seed, j, strata) and nothing else, defined to the last bit, and everything that decides it is
 * integer arithmetic.  All integer arithmetic below is unsigned and wraps; all f32 arithmetic is IEEE, every operation rounded on its own.
 * Areas.  area_i = the reference's own area function (ray_tracing.cpp:13-21: the cross product of v1 - v0 and v2 - v0 in f32, its
 * magnitude with squares, sum and sqrt in double, narrowed to f32, divided by 2.0f) of triangle i, i in prim_id order.  An area that is
 * NaN, infinite or not > 0 counts as 0.  S_i is the running sum of the areas as doubles, added sequentially in prim_id order; A =
 * S_{ntris-1} is the total.
 * Thresholds.  T_i = min(floor((S_i / A) * 4294967296.0), 4294967295), evaluated in double, stored as u32.  L is the largest i with
 * area_i > 0; a scene without such a triangle (or without meshes) is EMPTY FOR SAMPLING.
 * Random words.  Philox4x32-10 with the Random123 constants (multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and
 * 0xBB67AE85); for the 64-bit sample index j the counter is {lo32(j), hi32(j), 0, 0} and the key {lo32(seed), hi32(seed)}; of the output
 * words w0..w3, w3 is unused.  (Known answer: counter 0,0,0,0 under key 0,0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.)
 * Position word.  strata == 0 (independent samples): x = w0.  strata = N > 0 (sample j lies in stratum j of N equal strata of the area
 * measure): x = floor((j * 2^32 + w0) / N) in 64-bit integers, which needs j < N <= 0xffffffff.
 * Triangle.  prim = #{ i < L : T_i <= x }: an upper bound over the first L thresholds; the last triangle with an area takes the rest.
 * Hence a triangle of area 0 is never chosen, wherever it sits, and a triangle smaller than 2^-32 of the total area may never be chosen.
 * Point.  a = w1 >> 8, b = w2 >> 8; if a + b > 2^24 then a = 2^24 - a and b = 2^24 - b; c = 2^24 - a - b.  bary = {c, a, b} * 2^-24 (exact
 * in f32), the weights of v0, v1, v2.  point.k = (bary0 * v0.k + bary1 * v1.k) + bary2 * v2.k, the order of cgrt_interpolate_hits.
 * Record.  CgrtSurfaceSample, 32 bytes; point, prim_id and bary sit at the offsets of CgrtClosest; mesh_id is the triangle's material
 * index (CgrtHit.material_id).  In a scene that is empty for sampling every record is {0,0,0, 0xffffffff, CGRT_NO_PRIM, 0,0,0}.
 * Per-vertex table (optional: attr and out_attr both, or neither).  attr is nverts x channels f32 (channels in 1..256), as
 * cgrt_interpolate_hits takes it; out_attr (n x channels) receives (bary0 * a0 + bary1 * a1) + bary2 * a2 over the triangle's three
 * vertex rows, zero rows for empty records.  With the vertex positions as the table the rows are the records' points, bit for bit.
 * Chunking.  A call with params->first = f writes samples f .. f + n - 1: any split of a range into calls, streams or devices gives the
 * same bytes.
 * Scale.  Multiplying every position by 2^k scales the areas exactly while none leaves the normal f32 range: thresholds, prim_id and
 * bary are then unchanged and the points are the old points times 2^k.  Beyond that range triangles drop out SILENTLY, since an area
 * that overflows to +inf or vanishes counts as 0: of the 32 triangles of a unit-sized Cornell box scaled by 2^64 the 10 largest are
 * never sampled again (L is unchanged), a unit cube scaled by 2^64 -- or any unit-sized scene scaled by 2^-75 -- is empty for
 * sampling, and at 2^-70 a 16 311-triangle mesh keeps 12 triangles, L moves to 11 and one threshold repeats 16 300 times.  The records
 * are the defined ones throughout (tests/test_surface_scale_gpu.py).
 * cgrt_triangle_areas: areas (NULL, or ntris floats: area_i, 0 where it counts as 0) and *total (NULL, or A).  cgrt_debug_get_sample_table:
 * thresholds (NULL, or ntris entries; all 0 in an empty scene) and *last (NULL, or L; CGRT_NO_PRIM in an empty scene).  Both are host
 * work and succeed on a host-only scene, as cgrt_debug_get_winding_tree does.
 * The table is built on the host by the scene's first sampling call (any of the four entries), under the scene's lock; the thresholds
 * are uploaded once and freed with the scene, and cgrt_device_bytes includes them (and the lookup table of cgrt_interpolate_hits) from
 * then on.
 * Streams.  The host form (host pointers, synchronous) runs on a call lane like cgrt_closest_points: any number of threads may sample
 * one scene at once.  The device form reads no host array behind the call and only enqueues on `stream` (NULL = default stream).
 * Neither reads or writes the prediction record, the frame hints or any frame state.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene; NULL out with n > 0; exactly one of attr and out_attr
 * given; n > 0x7fffffff; (with a table) channels outside 1..256, or n x channels x 4 above 2^40 bytes; strata > 0xffffffff; strata > 0
 * and first + n > strata; first + n overflows 64 bits; (device form) a pointer not 4-byte aligned.  Then a host-only scene:
 * CGRT_E_NO_DEVICE.  n == 0 succeeds and touches nothing.  Device form: then d_out (n * 32 bytes), d_attr (nverts * channels * 4) and
 * d_out_attr (n * channels * 4) checked as device memory of the scene's device.
 * Not offered: gradients through the samples; spheres; a restriction to some meshes or materials; weights other than area (blue-noise
 * sets: "Poisson-disk sets" below filters these samples); grid and enqueued-ticket forms (the device form never blocks); the C++ host
 * mirror. */
typedef struct CgrtSurfaceSample {
    float point[3];
    uint32_t mesh_id; /* 0xffffffff in an empty scene */
    uint32_t prim_id; /* CGRT_NO_PRIM in an empty scene */
    float bary[3];    /* the weights of tri[prim_id][0..2] */
} CgrtSurfaceSample;
typedef struct CgrtSampleParams { /* NULL = zeros */
    uint64_t seed;                /* the Philox key */
    uint64_t first;               /* the index of the call's first sample */
    uint64_t strata;              /* 0 = independent samples; N = sample j in stratum j of N (first + n <= N <= 0xffffffff) */
} CgrtSampleParams;
int cgrt_sample_surface(CgrtScene* scene, uint64_t n, const CgrtSampleParams* params, CgrtSurfaceSample* out, const float* attr,
                        uint32_t channels, float* out_attr);
int cgrt_sample_surface_device(CgrtScene* scene, uint64_t n, const CgrtSampleParams* params, CgrtSurfaceSample* d_out, const float* d_attr,
                               uint32_t channels, float* d_out_attr, void* stream);
int cgrt_triangle_areas(CgrtScene* scene, float* areas, double* total);
int cgrt_debug_get_sample_table(CgrtScene* scene, uint32_t* thresholds, uint32_t* last);

/* Poisson-disk sets: of n points, a subset in which no two are closer than a radius and to which none can be
 * added -- blue-noise samples when the points are cgrt_sample_surface's.  The result is defined to the last bit: a pure function of
 * (points, min_dist2, seed or priority), whatever the grid, the launch shape, the stream, the thread or the run.  The scene names the
 * device and lends its call lanes; its geometry is not read.  All f32 arithmetic is IEEE, every operation rounded on its own.
 * Inputs.  points: n x 3 f32.  params (CgrtPoissonParams, not NULL): min_dist2 (f32), seed (u64), priority (NULL, or n u32: host memory
 * in the host form, device memory in the device form).
 * Finite.  Point i is finite iff its three coordinates are.  A point that is not is never kept and conflicts with nobody.
 * Order.  P_i = priority[i] if a priority is given; else word w3 of Philox4x32-10 with the constants of "Surface sampling" above,
 * counter {lo32(i), hi32(i), 0, 0}, key {lo32(seed), hi32(seed)} -- the word the sampler leaves unused, so the order does not depend
 * on where a sample lies even under the sampler's own seed.  (Known answer: w3 = 9b00dbd8 for the zero counter and key.)  i comes
 * before j iff (P_i, i) < (P_j, j) lexicographically.
 * Conflict.  dx = fl(x_i - x_j), dy and dz likewise; d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), nothing contracted; the value is the
 * same for (i, j) and (j, i).  i and j conflict iff both are finite, i != j and d2 < min_dist2, strictly.  A d2 that overflows to +inf
 * is never a conflict.  min_dist2 NaN or <= 0: nothing conflicts, every finite point is kept.  min_dist2 == +inf: CGRT_E_ARG.
 * Envelope.  d2 is a sum of squares of differences: it grows as the SQUARE of the cloud's size.  Multiplying every point by 2^k and
 * min_dist2 by 2^2k changes no significand, so while, for every pair, the smallest non-zero |dx|, |dy|, |dz| still has a normal square,
 * d2 does not overflow, and min_dist2 * 2^2k is a normal float, every operation rounds as at scale 1 and the flags are those of scale 1
 * (tests/scale_ref.py in_point_envelope states the predicate).  Outside it the flags are still the defined ones on every path -- grid,
 * brute and restatement agree byte for byte -- they are only no longer the flags of scale 1: subnormal squares lose bits (a
 * subnormal min_dist2 of a few ulps keeps other points), a min_dist2 that underflows to 0 keeps every finite point, a d2 of +inf never
 * conflicts, and a cloud whose extent overflows f32 (x - lo = +inf) is binned into the last cell, 2^21 - 1, of that axis.
 * Result.  Going through the points in the order, i is kept iff it is finite and no point kept before it conflicts with it: the
 * lexicographically first maximal independent set of the conflict graph, which is unique.  No two kept points conflict, and every finite
 * point that is not kept conflicts with a kept point that comes before it.
 * Outputs.  keep: n bytes, each 1 or 0.  *kept (host memory in both forms; NULL: not wanted): the number of ones.
 * Both forms BLOCK.  The work is a few passes that build a hashed grid and then rounds whose number depends on the data: each round
 * decides every undecided point all of whose earlier conflicting points are decided.  With the Philox order the number of rounds
 * grows like log n; with a caller priority it can reach n (points on a line, priority = index).  The host form (host pointers) runs on a
 * call lane like cgrt_closest_points and allocates its own workspace: any number of threads may call at once.  The device form is
 * ordered on `stream` (NULL = default stream) behind what it held, reads one 64-byte header back from the device into pinned memory
 * per batch of rounds, and returns when keep[] is complete.  An enqueued form is not offered.
 * Workspace (device form).  cgrt_poisson_disk_workspace reports the bytes a call with n points needs (about 40 per point): caller-owned
 * device memory, 8-byte aligned, contents need no initialisation, not shared between calls in flight.
 * cgrt_poisson_disk_brute: the same bytes without a grid -- every pair is tested in every round; the yardstick.  Host form only.
 * cgrt_debug_poisson_work (host form, a counted run, no flags): out6 = {rounds that had undecided points, pair tests, buckets in use,
 * buckets, nanoseconds of the grid build, nanoseconds of the rounds (both on the host's clock around a wait for the stream)}.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene or params; NULL points or keep with n > 0; n > 0x7fffffff;
 * min_dist2 == +inf; (device form) d_points or priority not 4-byte aligned; (device form, n > 0) d_workspace NULL, not 8-byte aligned,
 * or workspace_bytes below cgrt_poisson_disk_workspace.  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0 succeeds, writes *kept = 0
 * and touches nothing else.  Device form: then d_points (n * 12 bytes), d_keep (n), priority (n * 4) and d_workspace checked as device
 * memory of the scene's device.  Neither form reads or writes the prediction record, the frame hints, the layout or any frame state.
 * Not offered: per-point radii; geodesic distance; weighted elimination beyond the caller priority; progressive or multi-class sets; an
 * enqueued form; the C++ host mirror. */
typedef struct CgrtPoissonParams {
    float min_dist2;          /* squared minimum distance; NaN or <= 0: nothing conflicts; +inf -> CGRT_E_ARG */
    uint64_t seed;            /* the Philox key of the order (ignored with a priority) */
    const uint32_t* priority; /* NULL, or n words: smaller goes first, ties by index */
} CgrtPoissonParams;
int cgrt_poisson_disk(CgrtScene* scene, const float* points, uint64_t n, const CgrtPoissonParams* params, uint8_t* keep, uint64_t* kept);
int cgrt_poisson_disk_device(CgrtScene* scene, const float* d_points, uint64_t n, const CgrtPoissonParams* params, uint8_t* d_keep,
                             uint64_t* kept, void* d_workspace, uint64_t workspace_bytes, void* stream);
int cgrt_poisson_disk_workspace(CgrtScene* scene, uint64_t n, uint64_t* bytes);
int cgrt_poisson_disk_brute(CgrtScene* scene, const float* points, uint64_t n, const CgrtPoissonParams* params, uint8_t* keep, uint64_t* kept);
int cgrt_debug_poisson_work(CgrtScene* scene, const float* points, uint64_t n, const CgrtPoissonParams* params, uint64_t* out6);

/* Point-set neighbours: "which points of this cloud lie within r of p -- all of them, nearest first?" and "which
 * are the k nearest?" for a list of query points -- normals and densities from the k nearest samples, kNN graphs and ball-query groups for
 * point-cloud networks, Chamfer distances between two clouds, outlier removal, smoothing over a radius.  Every other query relates a point
 * to the mesh; these relate points to points, over a hashed uniform grid that outlives the call that built it.  The scene names the
 * device and lends its call lanes, as for cgrt_poisson_disk; its geometry is not read.  All f32 arithmetic is IEEE, every operation rounded
 * on its own, nothing contracted.  The definition below IS the specification.
 * Data and queries.  data: m x 3 f32, 0 <= m <= 0x7fffffff.  points: n x 3 f32, the queries, n <= 0x7fffffff.  A data point with a
 * non-finite coordinate is nobody's neighbour; a non-finite query has no neighbours.
 * Distance.  For query q and data point j: dx = fl(q.x - d_j.x), dy and dz likewise; d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) -- the
 * conflict arithmetic of "Poisson-disk sets", a pure function of the two points.
 * Bound.  query (CgrtPointQuery, not NULL): r2 = radius2 ? radius2[i] : max_dist2, exactly as cgrt_count_neighbors defines and checks it:
 * a scalar max_dist2 that is NaN or negative is CGRT_E_ARG (also where radius2 is given), +inf is unbounded; a per-query radius2[i] for
 * which `radius2[i] >= 0` is false gives that query no neighbours, decided in the kernel, identically in all forms (radius2: n f32, host
 * memory in the host forms, device memory in the device forms; the host forms do not scan it).
 * Neighbour.  j is a neighbour of query i iff both are finite and `d2 <= r2` is true -- non-strictly, like the triangle neighbours and
 * unlike Poisson's `<` -- and the flag below does not exclude it.  A NaN d2 never qualifies.  A d2 that overflows to +inf qualifies under
 * r2 = +inf only.
 * Flag.  With CGRT_POINTS_SKIP_SAME_INDEX in query->flags, j == i is never a neighbour of query i (a cloud queried against itself).  Any
 * other bit: CGRT_E_ARG.
 * Order and slots.  A query's neighbours are ordered by d2 compared as floats, equal d2 going to the smaller index: a total order, so
 * every output byte is determined.  CgrtPointNeighbor = {dist2, index}, 8 bytes, CgrtNeighbor's layout.  The slot rule is word for word
 * that of "Crossing queries" and "Neighbour queries": the count calls write counts[i] = the number of neighbours of query i; in the list
 * calls query i owns the records [offsets[i], offsets[i + 1]) of out (offsets: n + 1 u64) or, with offsets == NULL, [i * k, (i + 1) * k):
 * exactly one of offsets and k > 0 must be given.  A slot of s records receives the first min(s, count) neighbours in order and
 * {+inf, CGRT_NO_PRIM} in its remaining entries; counts[i] (may be NULL in the list calls) is always the full count.  Every record of
 * every slot is written, nothing outside the slots.  The host forms check that offsets start at 0, do not decrease and end <= capacity;
 * the device form never reads the offsets on the host: the kernel treats a decreasing pair as an empty slot and clamps both ends to
 * capacity (slots that overlap are written by several queries, in no defined order).
 * Exact nearest.  With k > 0 and counts == NULL the call is "the k nearest within r2"; with r2 = +inf, the k nearest.
 * Determinism.  The result is a function of (data, points, bound, flags) alone: not of the cell size, the bucket count, the order inside
 * a bucket, the launch shape, the stream or the run.  cgrt_list_point_neighbors_brute -- every data point in turn, the same function, the
 * same slot rule, no grid -- returns the same bytes; it is the yardstick.
 * Accuracy.  While no intermediate is subnormal or overflows, d2 = exact * (1 + e) with |e| <= (1 + u)^5 - 1 < 5.0000006 u, u = 2^-24:
 * each difference carries one rounding (1 + a), |a| <= u, so its exact square carries (1 + a)^2; the product adds one rounding, the first
 * sum one (over non-negative terms, whose relative errors do not grow under addition), the second sum one: the x and y terms pass through
 * 2 + 1 + 1 + 1 = 5 factors, the z term through 4.  Membership can therefore differ from the float64 answer only for pairs whose exact
 * squared distance lies within that relative band of r2 (tests/test_point_neighbors_cpu.py).
 * Envelope.  d2 grows as the SQUARE of the cloud's size.  Multiplying data, queries (and the cell) by 2^k and every bound by 2^2k
 * changes no significand.  A query is inside the envelope at 2^k while (min |dx|)^2 * 2^2k >= FLT_MIN, min |dx| the smallest non-zero
 * coordinate difference between it and any finite data point; (max d2) * 2^2k <= FLT_MAX, over the finite data points; r2 * 2^2k is a
 * normal float; and the query and r2 are finite (tests/scale_ref.py point_measures, in_point_envelope).  Inside it every operation of
 * d2 rounds as at scale 1: counts and index order are unchanged, every dist2 is multiplied by 2^2k exactly, and the search visits the
 * images of the same cells (the work counters are equal).  Outside it the bytes are still the defined ones on every path -- grid form,
 * brute form and the definition agree -- only the relation to scale 1 is lost: subnormal d2 lose bits and tie; where r2 and every d2
 * underflow to 0 every finite data point is a neighbour of every finite query, in index order; a d2 of +inf qualifies under r2 = +inf
 * only and ties on index; a cloud whose x - lo overflows is binned into cell 2^21 - 1 of that axis; a subnormal cell or bound is taken
 * as it is (the reach R of a subnormal r2 is a normal float).
 * The grid.  cgrt_point_grid_workspace reports the bytes a grid over m points needs (24 per point and 8 per bucket, of which there are
 * about as many as points, at least 1024).  cgrt_point_grid_build_device enqueues the build on `stream` (NULL = default
 * stream) into caller-owned device memory (8-byte aligned, contents need no initialisation): it never blocks and reads nothing back.
 * The grid is self-contained -- its entries hold the coordinates -- so d_data may be freed or overwritten once the build has run.
 * cell (finite, > 0) is the wanted cell edge; the edge used is h = max(cell, half extent of the finite data * 2^-18), Poisson's rule.
 * A good cell is about the query radius; no result depends on it.  m == 0 or a cloud with no finite point builds an empty grid, in which
 * no query has a neighbour.  A grid may be queried any number of times, from several streams and threads at once; the caller orders
 * the queries behind the build, and a rebuild behind the queries.  The query entries read every grid parameter from the grid's header on
 * the device; a header that does not describe a grid within grid_bytes (memory that was never built) reads as an empty or a wrong grid,
 * never as an address outside [d_grid, d_grid + grid_bytes).  grid_bytes is what the memory holds, at least cgrt_point_grid_workspace(m).
 * Search.  One query per lane.  R_i: the root of the next float above r2, rounded up, plus an ulp.  d2 <= r2 implies |q.x - d_j.x| < R_i
 * exactly (monotone rounding, point_neighbor_kernels.hip), so per axis the lane visits the cells [cell(fl(x - R_i)), min(cell(fl(x + R_i)),
 * cell(hi))], hi the data's maximum: cell() is monotone, so the clamp loses nobody and a query far outside the cloud visits few cells.  A
 * bucket of the hash also holds points of other cells; every entry carries its own cell's 63-bit key and is accepted only in the visit of
 * that cell, so each data point is met exactly once per query.  A range with more cells than the grid has entries (r2 = +inf, radii far
 * above the cell edge) is not walked: the lane reads the entry array itself, once.  A slot is kept sorted by insertion: a full list of c
 * neighbours costs up to c^2 / 2 record moves.  While a slot is full and no count is asked for, entries beyond the largest d2 kept are
 * passed over (non-strictly: an equal-d2 smaller index still arrives).
 * Host forms (host pointers, synchronous) run on a call lane like cgrt_closest_points and allocate, build and free a grid of their own
 * per call: any number of threads may call at once.  cgrt_debug_point_neighbor_work (host form; a counted launch, never part of a timed
 * region; k = 0: the count search, k > 0: k records per query and no counts): out6 = {cells visited, entries read, entries passed over
 * because they belong to another cell, d2 evaluations, queries that took the linear walk, buckets in use}, summed over the n queries.
 * The device forms read no host array but *query and only enqueue on `stream`; they neither read nor write any frame state.
 * Checks, all CGRT_E_ARG, in this order and before any device work.  Query entries: NULL scene or query; with n > 0, NULL points, result
 * array (counts of the count calls, out of the list calls, out6), data with m > 0 (host forms) or d_grid (device forms); n > 0x7fffffff;
 * (host forms) m > 0x7fffffff; (host forms with a grid) cell not finite or <= 0; max_dist2 NaN or negative; an unknown flag; (list calls)
 * both or neither of offsets and k > 0; capacity above 2^37 records; with k, n * k > capacity; (host list calls, n > 0) offsets not
 * starting at 0, decreasing, or ending above capacity; (device forms) a pointer not aligned to its element (4 bytes; 8 for d_offsets and
 * d_grid); (device forms, n > 0) grid_bytes below cgrt_point_grid_workspace(0).  cgrt_point_grid_build_device: NULL scene; NULL d_data
 * with m > 0 or NULL d_grid; m > 0x7fffffff; cell; d_data not 4-byte or d_grid not 8-byte aligned; grid_bytes below
 * cgrt_point_grid_workspace(m).  cgrt_point_grid_workspace: NULL scene or bytes; m > 0x7fffffff.  Then a host-only scene:
 * CGRT_E_NO_DEVICE (not cgrt_point_grid_workspace, which only computes).  n == 0 succeeds and touches nothing.  Device forms: then
 * d_points (n * 12 bytes), radius2 (n * 4), d_offsets ((n + 1) * 8), d_out (capacity records with offsets, n * k with k), d_counts (n * 4)
 * and d_grid (grid_bytes; the build: d_data, m * 12, and the workspace of m) checked as device memory of the scene's device.
 * Not offered: per-record coordinates (they are data[index]); a per-query k (offsets give per-query slot sizes); periodic domains;
 * incremental insertion; enqueued-ticket forms (the device forms never block); the k nearest without a bound in one entry (r2 = +inf
 * walks every entry: compose growing radii, as the Python PointGrid.knn does); the C++ host mirror. */
#define CGRT_POINTS_SKIP_SAME_INDEX 1u
typedef struct CgrtPointNeighbor {
    float dist2;    /* d2 as defined above; +inf in an unused entry       */
    uint32_t index; /* the data point; CGRT_NO_PRIM in an unused entry    */
} CgrtPointNeighbor;
typedef struct CgrtPointQuery {
    const float* radius2; /* NULL, or n squared radii (NaN or negative: that query has no neighbours) */
    float max_dist2;      /* the bound of every query where radius2 == NULL; NaN or negative -> CGRT_E_ARG; +inf: unbounded */
    uint32_t flags;       /* 0, or CGRT_POINTS_SKIP_SAME_INDEX */
} CgrtPointQuery;
int cgrt_point_grid_workspace(CgrtScene* scene, uint64_t m, uint64_t* bytes);
int cgrt_point_grid_build_device(CgrtScene* scene, const float* d_data, uint64_t m, float cell, void* d_grid, uint64_t grid_bytes, void* stream);
int cgrt_count_point_neighbors_device(CgrtScene* scene, const void* d_grid, uint64_t grid_bytes, const float* d_points, uint64_t n,
                                      const CgrtPointQuery* query, uint32_t* d_counts, void* stream);
int cgrt_list_point_neighbors_device(CgrtScene* scene, const void* d_grid, uint64_t grid_bytes, const float* d_points, uint64_t n,
                                     const CgrtPointQuery* query, const uint64_t* d_offsets, uint32_t k, CgrtPointNeighbor* d_out,
                                     uint64_t capacity, uint32_t* d_counts, void* stream);
int cgrt_count_point_neighbors(CgrtScene* scene, const float* data, uint64_t m, float cell, const float* points, uint64_t n,
                               const CgrtPointQuery* query, uint32_t* counts);
int cgrt_list_point_neighbors(CgrtScene* scene, const float* data, uint64_t m, float cell, const float* points, uint64_t n,
                              const CgrtPointQuery* query, const uint64_t* offsets, uint32_t k, CgrtPointNeighbor* out, uint64_t capacity,
                              uint32_t* counts);
int cgrt_list_point_neighbors_brute(CgrtScene* scene, const float* data, uint64_t m, const float* points, uint64_t n,
                                    const CgrtPointQuery* query, const uint64_t* offsets, uint32_t k, CgrtPointNeighbor* out, uint64_t capacity,
                                    uint32_t* counts);
int cgrt_debug_point_neighbor_work(CgrtScene* scene, const float* data, uint64_t m, float cell, const float* points, uint64_t n,
                                   const CgrtPointQuery* query, uint32_t k, uint64_t* out6);

/* Point-set frames: the first use "Point-set neighbours" names -- a normal per point -- and what needs a local
 * frame: per query point the centroid, the three eigenvalues of the covariance and a right-handed frame of its k nearest data points
 * within a squared radius (local PCA).  normal is the direction of least variance; lambda0 / (lambda0 + lambda1 + lambda2) is the surface
 * variation; tangent_u and tangent_v span the tangent plane.  One kernel does the search and the solve; nothing is left to a library
 * routine.  The scene names the device and lends its call lanes; its geometry is not read.  All arithmetic is f32 and IEEE, every operation
 * rounded on its own, nothing contracted; the only operations are + - x / sqrt and comparisons.  The definition below IS the specification
 * (tests/point_frames_ref.py restates it in numpy and gives the same bytes).  For query i:
 * 1. Neighbourhood.  Exactly the slot cgrt_list_point_neighbors writes for this data, query, bound and flag with k records per query and
 *    no counts: the first min(k, count) neighbours in (d2, index) order, then {+inf, CGRT_NO_PRIM}.  used = the number of real records.
 *    used == 0 (also: a non-finite query, a NaN or negative radius2[i]) gives a record of 64 zero bytes.
 * 2. Centroid.  p_j = data[index_j], j = 0 .. used - 1 in slot order; ref = p_0.  Per axis s = sum_j fl(p_j - ref), added one by one
 *    from +0 in that order; c = fl(ref + fl(s / (float)used)).
 * 3. Covariance.  e_j = fl(p_j - c).  The six sums xx, xy, xz, yy, yz, zz of fl(e_a e_b), each added one by one from +0 in slot order,
 *    each then divided by (float)used: the symmetric matrix a.
 * 4. Eigen-solve.  Cyclic Jacobi on a, V = identity.  A sweep visits the pairs (p, q) = (0, 1), (0, 2), (1, 2), r the third index.  A
 *    pair with a_pq == 0 is skipped.  Otherwise theta = fl(fl(a_qq - a_pp) / fl(2 a_pq)); t = (theta < 0 ? -1 : 1) / fl(|theta| +
 *    sqrt(fl(fl(theta theta) + 1))); c = 1 / sqrt(fl(fl(t t) + 1)); s = fl(t c); h = fl(t a_pq); a_pp = fl(a_pp - h); a_qq = fl(a_qq + h);
 *    a_pq = 0; a_rp' = fl(fl(c a_rp) - fl(s a_rq)), a_rq' = fl(fl(s a_rp) + fl(c a_rq)); and in every row i of V, V_ip' = fl(fl(c V_ip) -
 *    fl(s V_iq)), V_iq' = fl(fl(s V_ip) + fl(c V_iq)).  After a sweep the loop ends if all three off-diagonals are == 0; it ends after 8
 *    sweeps in any case.
 * 5. Order.  The eigenvalues are the diagonal, sorted ascending together with their columns of V by three exchanges: (0, 1), (1, 2),
 *    (0, 1), each made iff `d_b < d_a` is true -- a stable sort: ties and NaNs keep column order.  normal, tangent_u, tangent_v are the
 *    columns of lambda0 <= lambda1 <= lambda2.  Nothing is renormalised.
 * 6. Signs.  normal and tangent_u are each negated iff their component of largest magnitude is < 0 (found by `|v_1| > |v_0|`, then
 *    `|v_2| > the larger`: on a tie the first counts, a NaN never does).  If orient is given, o = orient[i] has three finite components and
 *    fl(fl(fl(n.x o.x) + fl(n.y o.y)) + fl(n.z o.z)) < 0, normal is negated.  Then with w = (fl(fl(n.y u.z) - fl(n.z u.y)), fl(fl(n.z u.x) -
 *    fl(n.x u.z)), fl(fl(n.x u.y) - fl(n.y u.x))), tangent_v is negated iff fl(fl(fl(w.x v.x) + fl(w.y v.y)) + fl(w.z v.z)) < 0: a
 *    right-handed frame (normal x tangent_u = tangent_v) wherever that means something.
 * 7. Record.  CgrtPointFrame below, 64 bytes; every float that is a NaN is stored as 0x7fc00000 (the sign and payload of a NaN are the one
 *    thing IEEE arithmetic leaves open).  Every byte of every record is written.
 * 8. Degenerate input is returned as the arithmetic gives it.  used == 1: a zero matrix, the identity's columns, centroid = p_0.  used
 *    == 2 and collinear or coplanar neighbours: a rank-deficient matrix; the eigenvalues are right (0 up to rounding), the vectors of
 *    the null space deterministic but arbitrary.  Equal eigenvalues: any frame of the eigenspace.  Differences or squares that overflow
 *    give inf and then NaN, which propagate as defined above.
 * Determinism.  The record is a function of (data, points, bound, flag, k, orient) alone: not of the cell size, the bucket count, the
 * order inside a bucket, the launch shape, the stream or the run.  cgrt_point_frames_brute -- every data point in turn, the same function
 * -- returns the same bytes; it is the yardstick.  The neighbour array receives exactly the bytes of the list call.
 * Scale.  Multiplying data, queries (and the cell) by 2^s and every bound by 2^2s multiplies centroid by 2^s and the eigenvalues by 2^2s
 * exactly and leaves the vectors and used unchanged, while the query is inside the point-neighbour envelope at 2^s AND every product or
 * quotient of steps 2 to 4 that carries the scale -- s / used, e_a e_b, sum / used, t a_pq, c a_rp, s a_rq, s a_rp, c a_rq -- is zero or a
 * normal float at both scales (additions and subtractions are exact where they underflow; theta, t, c, s and V carry no scale).  This is
 * a sufficient condition and a narrow one: the late sweeps multiply off-diagonals that are already far below an ulp of the diagonal, down
 * to about 2^-140 of the trace T, so it asks T and T 2^2s to lie within about [2^14, 2^120].  Outside it the bytes are still the defined
 * ones on every path; the relation to scale 1 was observed to hold there too (the values that underflow meet nothing they could change)
 * but is not claimed.  tests/point_frames_ref.py reports the smallest and largest such value per query (in_frame_envelope).
 * Accuracy (measured through the restatement against numpy.linalg.eigh in float64 on the float64 covariance of the same neighbours,
 * tests/test_point_frames_cpu.py; the clouds are a sample of inputs, not a worst case, and the tests hold four times these figures).
 * With u = 2^-24, T the trace and P the largest coordinate magnitude of the neighbourhood, the largest values measured (k = 3, 8, 32):
 * |lambda - lambda64| <= 3.36 u T + 1.03 u^2 P^2 (the second term is the centroid's rounding, which enters every e_j; it dominates for a
 * cloud far from the origin relative to its spread: 8000 u T at offset 100 with spread 0.01 and k = 3); the squared length of every
 * vector is within 13.2 u of 1; the angle between normal and the float64 eigenvector, times the relative gap (lambda1 - lambda0) / T, is
 * at most 1.50 (u + u^2 P^2 / T) over the queries whose gap exceeds 1e-2.  Every off-diagonal was exactly zero after at most 5 sweeps.
 * The entries.  cgrt_point_frames_device enqueues on `stream` (NULL = default stream) and never blocks: d_grid, grid_bytes a built grid;
 * d_data, m the array it was built on, which the caller keeps alive and unchanged until the call has run -- unlike the list queries, the
 * frames read coordinates by index (an index that is not below m, which only a grid of other data holds, is never used as an address:
 * that query's record is 64 zero bytes); d_orient NULL or n x 3 f32; d_neighbors n * k records, a required output (the k nearest and the
 * frames come from one call); d_frames n records, 16-byte aligned.  cgrt_point_frames (host pointers, synchronous) builds and frees a grid
 * of its own on a call lane like cgrt_list_point_neighbors; its neighbors may be NULL.  cgrt_point_frames_brute: the host form over every
 * data point in turn.  One query per lane, 256 lanes per block; after its search the lane reads its own slot back, gathers data[index]
 * and stores its record as four 16-byte stores: no atomics, no LDS, no scratch.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene or query; with n > 0, NULL points, frames, d_neighbors
 * (device form), data with m > 0, d_grid (device form); n > 0x7fffffff; m > 0x7fffffff; (host form with a grid) cell not finite or <= 0;
 * max_dist2 NaN or negative; an unknown flag; k == 0; n * k above 2^37 records; (device form) a pointer not aligned to its element (4
 * bytes; 8 for d_grid), then d_frames not 16-byte aligned; (device form, n > 0) grid_bytes below cgrt_point_grid_workspace(0).  Then a
 * host-only scene: CGRT_E_NO_DEVICE.  n == 0 succeeds and touches nothing.  Device form: then d_points, radius2, d_orient, d_neighbors,
 * d_frames, d_grid and d_data checked as device memory of the scene's device.
 * Not offered: weighted neighbourhoods; globally consistent orientation (propagation over a graph: orient takes what the caller knows,
 * a view point or a coarse normal); a per-query k; curvature tensors and higher moments; the k nearest without a bound in one entry
 * (compose growing radii, as the Python PointGrid.knn_frames does); enqueued-ticket forms (the device form never blocks); the C++ host
 * mirror. */
typedef struct CgrtPointFrame {
    float centroid[3];
    uint32_t used; /* real neighbour records, 0 .. k; 0: the whole record is zero bytes */
    float normal[3];
    float lambda0; /* lambda0 <= lambda1 <= lambda2 */
    float tangent_u[3];
    float lambda1;
    float tangent_v[3];
    float lambda2;
} CgrtPointFrame;
int cgrt_point_frames_device(CgrtScene* scene, const void* d_grid, uint64_t grid_bytes, const float* d_data, uint64_t m, const float* d_points,
                             uint64_t n, const CgrtPointQuery* query, uint32_t k, const float* d_orient /* NULL or n x 3 */,
                             CgrtPointNeighbor* d_neighbors /* n * k */, CgrtPointFrame* d_frames /* n */, void* stream);
int cgrt_point_frames(CgrtScene* scene, const float* data, uint64_t m, float cell, const float* points, uint64_t n, const CgrtPointQuery* query,
                      uint32_t k, const float* orient, CgrtPointNeighbor* neighbors /* NULL or n * k */, CgrtPointFrame* frames);
int cgrt_point_frames_brute(CgrtScene* scene, const float* data, uint64_t m, const float* points, uint64_t n, const CgrtPointQuery* query,
                            uint32_t k, const float* orient, CgrtPointNeighbor* neighbors /* NULL or n * k */, CgrtPointFrame* frames);

/* Iso-surfaces: the way back from a volume to a surface -- the indexed triangle mesh of one level of a scalar
 * grid, by marching tetrahedra (six per cell around the main diagonal: no ambiguous case, closed by construction).  The values are the
 * caller's: what cgrt_signed_distance_grid or cgrt_winding_numbers_grid made (offset and shell surfaces, the 0.5 level of an open mesh's
 * winding field as its watertight stand-in), or anything else.  The output is defined to the last bit and to the last index: a pure
 * function of (grid, values, iso, flags), whatever the launch shape, the stream, the thread or the run.  The scene names the device and
 * lends its call lanes; its geometry is not read.  All f32 arithmetic is IEEE, every operation rounded on its own, nothing contracted.
 * Inputs.  grid: a CgrtGrid.  values: nx ny nz f32 in the result order of cgrt_signed_distance_grid, index (iz ny + iy) nx + ix.  params
 * (CgrtIsoParams, not NULL): iso (finite) and flags (0 or CGRT_ISO_INSIDE_ABOVE).
 * Limits.  Each dim in 1..2^24; nx ny nz <= 2^28 (7 vertices and 12 triangles per point stay below 2^32); origin and spacing finite.  A grid
 * with a dim of 1 has no cell and gives the empty mesh: no vertex, no triangle.
 * Classification.  A grid point is finite iff its value is.  It is inside iff value < iso, strictly; with CGRT_ISO_INSIDE_ABOVE iff
 * value > iso -- the definition applied to the negated values and the negated level: the positions are the same bits, the triangles face
 * the other way.  A value equal to iso is outside under either flag.
 * Edges.  Point q = (ix, iy, iz) owns up to seven edges, to q + (dx, dy, dz) with (dx, dy, dz) in {0,1}^3 without 0; the edge's type is
 * e = dx + 2 dy + 4 dz - 1, in 0..6.  An owned edge exists where its far end is in the grid.  It carries a vertex iff both ends are finite
 * and exactly one of them is inside.
 * Vertex.  A the owner, B the far end: t = fl(fl(iso - vA) / fl(vB - vA)); if !(t >= 0) then t = 0; if t > 1 then t = 1;
 * p.c = fl(pA.c + fl(t fl(pB.c - pA.c))) per component, with the grid positions origin.c + (float)i spacing.c of cgrt_signed_distance_grid.
 * Vertices are ordered by the owner's index (iz ny + iy) nx + ix, then by edge type.
 * Cells.  The cell of q (ix < nx - 1, iy < ny - 1, iz < nz - 1) has corners c = x + 2 y + 4 z.  Its six tetrahedra, in this order and
 * corner order, all positively oriented: (0,1,3,7) (0,5,1,7) (0,3,2,7) (0,2,6,7) (0,4,5,7) (0,6,4,7).  A tetrahedron with a non-finite
 * corner emits nothing.  Otherwise mask m has bit k set iff its k-th corner is inside, and it emits the triangles of row m below; a table
 * vertex names a tetrahedron edge by its two corner positions, and a triangle is listed in the order its indices are written:
 *    1: (01,02,03)             14: (01,03,02)
 *    2: (01,13,12)             13: (01,12,13)
 *    4: (02,12,23)             11: (02,23,12)
 *    8: (03,23,13)              7: (03,13,23)
 *    3: (02,03,13) (02,13,12)  12: (02,12,13) (02,13,03)
 *    5: (01,23,03) (01,12,23)  10: (01,23,12) (01,03,23)
 *    6: (01,13,23) (01,23,02)   9: (01,02,23) (01,23,13)
 *    0, 15: nothing
 * Normals by the right-hand rule point from inside to outside: for an SDF the mesh is outward-oriented and encloses positive signed
 * volume.  A triangle's index is its vertex's rank in the vertex order (the edge between cell corners lo < hi is owned by corner lo, type
 * hi - lo - 1).  Triangles are ordered by the cell's index, then tetrahedron, then table position.
 * Properties.  If every value is finite and no cell on the grid's boundary is crossed, every directed edge occurs exactly once and its
 * reverse exactly once.  A value equal to iso puts vertices on the grid point and gives zero-area triangles, which are kept.  Next to
 * non-finite values there may be unreferenced vertices and open borders.
 * Envelope.  Every intermediate is LINEAR in the values or in the positions, and the two never mix: t is a ratio of two value
 * differences, a coordinate is a position plus t times a position difference.  Per vertex-carrying edge, multiplying values and iso by
 * 2^kv changes nothing while every non-zero one of vA, vB, iso, fl(iso - vA), fl(vB - vA) times 2^kv stays a normal float; multiplying
 * origin and spacing by 2^kp multiplies the vertex by 2^kp exactly while every non-zero one of both ends' grid positions (and their
 * products (float)i spacing.c), fl(pB.c - pA.c), fl(t fl(pB.c - pA.c)) and the coordinate itself times 2^kp stays normal
 * (tests/scale_ref.py in_iso_envelope).  The triangles and both counts never depend on origin or spacing, and on the values only through
 * the classification, which a scale changes only where a value or iso underflows to 0 or overflows.  Outside the envelope the bytes are
 * still the defined ones on every path -- device, host and count forms agree with the definition -- only the relation to scale 1 is
 * lost: a subnormal vB - vA or position loses bits; a vB - vA of +-inf gives t = 0; where grid_coord overflows, pA.c - pA.c on an axis
 * the edge does not move along is inf - inf and the coordinate a NaN (of either sign bit: compare NaNs as NaNs, not by bytes).
 * Outputs.  verts: 3 f32 per vertex.  tris: 3 u32 per triangle.  counts2 = {vertices, triangles}, always the full counts (device forms:
 * device memory, 8-byte aligned; host form: host memory).  Vertex j is written iff j < vert_capacity, triangle j iff j < tri_capacity, its
 * indices as they are even where >= vert_capacity; nothing else in or outside the arrays is touched (the slot rule of the crossing lists).
 * cgrt_isosurface_device is self-contained: it redoes the count inside its workspace, so a caller who over-allocates needs one call.
 * Both device forms only enqueue on `stream` (NULL = default stream) and read nothing back.  The host form (host pointers) runs on a call
 * lane like cgrt_closest_points and blocks: any number of threads may call at once.
 * Workspace (device forms).  cgrt_isosurface_workspace reports the bytes a call on `grid` needs (6 per grid point, 1/16 per point for the
 * block totals, under 20 KB of padding): caller-owned device memory, 8-byte aligned, contents need no initialisation, not shared between
 * calls in flight.
 * cgrt_debug_isosurface_work (host form, a counted run): out4 = {cells that emit a triangle, tetrahedra that emit one, vertices, triangles}.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene, grid or params; the grid's limits; iso not finite, or an
 * unknown flag; NULL values; NULL counts2 (out4); NULL verts or tris with a non-zero capacity; (device forms) d_values, d_verts or d_tris
 * not 4-byte aligned, d_counts2 not 8-byte aligned; (device forms) d_workspace NULL, not 8-byte aligned, or workspace_bytes below
 * cgrt_isosurface_workspace.  Then a host-only scene: CGRT_E_NO_DEVICE (not cgrt_isosurface_workspace, which only computes: NULL argument,
 * then the grid's limits).  Device forms: then d_values (4 bytes per point), d_verts (12 bytes per vertex of min(vert_capacity, 7 per point)),
 * d_tris (likewise, 12 per point), d_counts2 (16 bytes) and d_workspace checked as device memory of the scene's device.  No form reads or
 * writes the prediction record, the frame hints, the layout or any frame state.
 * Not offered: marching cubes, dual contouring or sharp features; vertex normals or gradients as outputs; removal of zero-area triangles
 * and unreferenced vertices; a narrow-band mode that skips empty bricks; batched grids; the C++ host mirror. */
#define CGRT_ISO_INSIDE_ABOVE 1u
typedef struct CgrtIsoParams {
    float iso;      /* the level; not finite -> CGRT_E_ARG */
    uint32_t flags; /* 0, or CGRT_ISO_INSIDE_ABOVE */
} CgrtIsoParams;
int cgrt_isosurface_workspace(CgrtScene* scene, const CgrtGrid* grid, uint64_t* bytes);
int cgrt_isosurface_count_device(CgrtScene* scene, const CgrtGrid* grid, const float* d_values, const CgrtIsoParams* params,
                                 uint64_t* d_counts2, void* d_workspace, uint64_t workspace_bytes, void* stream);
int cgrt_isosurface_device(CgrtScene* scene, const CgrtGrid* grid, const float* d_values, const CgrtIsoParams* params, float* d_verts,
                           uint64_t vert_capacity, uint32_t* d_tris, uint64_t tri_capacity, uint64_t* d_counts2, void* d_workspace,
                           uint64_t workspace_bytes, void* stream);
int cgrt_isosurface(CgrtScene* scene, const CgrtGrid* grid, const float* values, const CgrtIsoParams* params, float* verts,
                    uint64_t vert_capacity, uint32_t* tris, uint64_t tri_capacity, uint64_t* counts2);
int cgrt_debug_isosurface_work(CgrtScene* scene, const CgrtGrid* grid, const float* values, const CgrtIsoParams* params, uint64_t* out4);

/* Grid fields: the two questions a volume is asked -- "what is the field, and its gradient, at this point?" and
 * "where does this ray first reach the level?" -- for the grids cgrt_signed_distance_grid and cgrt_winding_numbers_grid make and
 * cgrt_isosurface reads, or anyone's.  Both answers are defined to the last bit: pure functions of (grid, values, points or rays,
 * params), whatever the launch shape, the stream, the thread or the run.  The scene names the device and lends its call lanes; its
 * geometry is not read.  All f32 arithmetic is IEEE, every operation rounded on its own, nothing contracted; division and sqrt are
 * correctly rounded; every NaN the library computes is stored as 0x7fc00000.  Below, min(a, b) is a < b ? a : b and max(a, b) is
 * a > b ? a : b (a NaN first operand yields the second).
 * Grid and values.  grid: a CgrtGrid.  values: nx ny nz f32 in the result order of cgrt_signed_distance_grid, index (iz ny + iy) nx + ix.
 * Limits.  Each dim in 2..2^24; nx ny nz <= 0x7fffffff; origin and spacing finite; every spacing non-zero (a negative one is allowed: the
 * axis runs backwards).  Anything else: CGRT_E_ARG.
 * Sample of a point p.  params: CgrtFieldParams {outside, flags}, flags 0 or CGRT_FIELD_CLAMP; NULL means {NaN, 0}.
 *   Per axis c: u_c = fl(fl(p.c - origin.c) / spacing.c), top_c = (float)(n_c - 1).  With CGRT_FIELD_CLAMP u_c is first replaced by
 *   u_c < 0 ? 0 : (u_c > top_c ? top_c : u_c), which leaves a NaN a NaN.  p is inside iff 0 <= u_c && u_c <= top_c on all three axes
 *   (false for a NaN): under CGRT_FIELD_CLAMP only a point with a NaN u_c is outside.
 *   Outside: value = params.outside (its bits as given, a NaN's payload included), gradient = 0, inside = 0.
 *   Inside: i_c = min((int)floor(u_c), n_c - 2), f_c = fl(u_c - (float)i_c), which is exact and lies in [0, 1] (1 only on the last plane).
 *   The corners are v_xyz = values at (i_x + x, i_y + y, i_z + z).  lerp(a, b, f) = fl(a + fl(f fl(b - a))), the form of the iso-surface's
 *   vertex.  Along x: d_yz = fl(v_1yz - v_0yz), a_yz = fl(v_0yz + fl(f_x d_yz)).  Along y: e_z = fl(a_1z - a_0z), b_z = fl(a_0z + fl(f_y e_z)).
 *   Along z: w = fl(b_1 - b_0), value = fl(b_0 + fl(f_z w)).  The gradient is the derivative of that polynomial from the same differences:
 *   g_z = fl(w / spacing.z); g_y = fl(lerp(e_0, e_1, f_z) / spacing.y); g_x = fl(lerp(lerp(d_00, d_10, f_y), lerp(d_01, d_11, f_y), f_z)
 *   / spacing.x).  inside = 1.  A cell with a non-finite corner gives whatever IEEE gives (with the NaNs canonical).
 * Properties.  (a) Where f = 0 on all axes, value is the stored grid value's bits for finite corners: every product is a zero and every
 *   sum a + (+-0) (the one exception: a stored -0 may come back as +0; differences that overflow are not finite corners' business either).  On the last plane of an axis f = 1 and the
 *   value along it is fl(a + fl(b - a)), which need NOT be b: the difference rounds.  (b) A field that is affine in the position, with
 *   exactly representable data (every difference, product and sum above exact), is reproduced exactly, value and gradient alike.
 *   (c) Against float64 trilinear interpolation T64 at the same (i, f): |value - T64| <= 16 * 2^-24 * M, M the largest |corner|, for finite
 *   corners whose differences do not overflow.  Derivation, u = 2^-24: one lerp of inputs bounded by m rounds three times -- the
 *   difference (|b - a| <= 2m, error <= 2mu, times f <= 1), the product (<= 2mu), the sum (its exact value is a convex combination, so
 *   <= mu): 5mu to first order.  A lerp passes errors of its inputs on without growth (convex weights), its output stays within
 *   m (1 + 5u), and the three stages add: 15 M u + O(u^2); the second-order terms are below M u.  Hence C = 16.  (d) Both power-of-two
 *   scale symmetries hold.  Every intermediate is LINEAR in the values, and u, f depend on positions alone: multiplying the values by 2^k
 *   multiplies value and gradient by 2^k exactly while every non-zero one of the corners, d, f d, a, e, f e, b, w, f w, the value, the
 *   gradient's lerps and quotients times 2^k stays a normal float; multiplying origin, spacing and the points by 2^k leaves u, i, f and the
 *   value alone and multiplies the gradient by 2^-k exactly while every non-zero one of p.c, origin.c, p.c - origin.c, spacing.c and the
 *   gradient's quotients stays normal under the scale.  Outside the envelope the bytes are still the defined ones; only the relation to
 *   scale 1 is lost.
 * March of a ray.  A ray is the 7-float record {o, d, t_ray} (CgrtRay); d is taken as given and may be unnormalised.  params:
 *   CgrtMarchParams, 28 bytes, not NULL: iso finite; relax finite and >= 0; min_step finite and > 0; hit_eps finite and >= 0; max_steps in
 *   1..65536; refine in 0..32; flags 0 or CGRT_ISO_INSIDE_ABOVE.  A ray takes at most max_steps + refine samples by construction, which is
 *   what the caps are for: there is no unbounded mode.
 *   1. len = fl(sqrt(fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)))).  A ray is rejected -- a MISS with steps 0 -- if a component of o or d
 *      is not finite, if t_ray is a NaN, if !(len > 0), or if len is infinite.
 *   2. Box.  far_c = fl(origin.c + fl(top_c spacing.c)); lo_c = min(origin.c, far_c), hi_c = max(origin.c, far_c).  t0 = 0, t1 = t_ray.
 *      Per axis in x, y, z order: if d.c == 0 the ray is a MISS (steps 0) unless lo_c <= o.c && o.c <= hi_c; otherwise
 *      ta = fl(fl(lo_c - o.c) / d.c), tb = fl(fl(hi_c - o.c) / d.c), t0 = max(t0, min(ta, tb)), t1 = min(t1, max(ta, tb)).  MISS (steps 0)
 *      if !(t0 <= t1).
 *   3. t = t0, k = 0, no previous t.
 *   4. Sample: p.c = fl(o.c + fl(t d.c)); v = the sample at p under CGRT_FIELD_CLAMP with outside = NaN; g = fl(v - iso), with
 *      CGRT_ISO_INSIDE_ABOVE g = fl(iso - v).
 *   5. g a NaN: NONFINITE at t, steps = k.   6. g <= hit_eps: HIT (below).   7. Else t >= t1: MISS, steps = k.
 *   8. Else k + 1 == max_steps: EXHAUSTED at t, steps = max_steps.
 *   9. Else dt = max(fl(fl(relax g) / len), min_step); t_prev = t; t = min(fl(t + dt), t1); k += 1; back to 4.
 *   Hit.  ta = t_prev, tb = t.  Without a previous t (the first sample hit) no refinement runs.  Otherwise, `refine` times:
 *   tm = fl(ta + fl(0.5 fl(tb - ta))); gm as in 4 at tm; gm <= hit_eps sets tb = tm, anything else (a NaN too) ta = tm.  The record is
 *   t = tb, the field value v at tb, the sampler's gradient at p(tb) -- the field's own, not negated under CGRT_ISO_INSIDE_ABOVE --
 *   and steps = k.
 *   relax = 1 is sphere tracing of a signed distance field; relax = 0 a fixed-step march of any field (the 0.5 level of a winding grid
 *   with CGRT_ISO_INSIDE_ABOVE); refine makes either precise.
 * Record.  CgrtGridHit, 32 bytes {t, value, steps, status, gradient[3], reserved = 0}.  MISS: t = +inf, value 0, gradient 0.  EXHAUSTED: the
 *   last t and its v, gradient 0.  NONFINITE: t, value NaN, gradient 0.
 * Entries.  Sampling: value (n f32), gradient (3n f32), inside (n u8); any of the three may be NULL, not all.  Marching: hits, n records.
 * cgrt_debug_march_work (host form, a counting launch of its own, no record written): out3 = {rays that entered the box (passed step 2),
 * main-loop samples (step 4), refinement samples}; the closing evaluation of a HIT's gradient is not counted; n == 0 gives zeros.
 * The host forms (host pointers) run on a call lane like cgrt_isosurface and block: any number of threads may call at once.  The device
 * forms only enqueue on `stream` (NULL = default stream) and read nothing back.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene or grid; the grid's limits; bad params (sampling: an
 * unknown flag; marching: NULL, then its fields in the order above); NULL values; NULL points or rays with n > 0; every output NULL (hits;
 * out3); n > 0x7fffffff; (device forms) a pointer not 4-byte aligned (d_inside: any).  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0
 * succeeds and touches nothing.  Device forms: then d_values (4 bytes per grid point), d_points (12 n) or d_rays (28 n) and each output
 * given (4 n, 12 n, n; 32 n) checked as device memory of the scene's device.  Nothing outside the n records is written.  No form reads or
 * writes the prediction record, the frame hints, the layout or any frame state.
 * Not offered: tricubic or tetrahedral interpolation (the iso-surface's piecewise-linear field); gradients with respect to the values
 * from THESE entries (cgrt_sample_grid_grad below is the sampler's adjoint; the march's hit record has none); vector-valued or batched grids; wrap or reflect padding; a bricked or narrow-band value layout; empty-space skipping; frame,
 * AOV and enqueued-ticket forms; shading of marched hits through the render wavefront; the C++ host mirror. */
#define CGRT_FIELD_CLAMP 1u
#define CGRT_MARCH_MISS 0u
#define CGRT_MARCH_HIT 1u
#define CGRT_MARCH_EXHAUSTED 2u
#define CGRT_MARCH_NONFINITE 3u
typedef struct CgrtFieldParams {
    float outside;  /* the value of a point outside the grid, stored as given */
    uint32_t flags; /* 0, or CGRT_FIELD_CLAMP */
} CgrtFieldParams;
typedef struct CgrtMarchParams {
    float iso;          /* the level; finite */
    float relax;        /* step = relax * g / |d|; finite, >= 0 */
    float min_step;     /* the smallest step in t; finite, > 0 */
    float hit_eps;      /* a sample with g <= hit_eps hits; finite, >= 0 */
    uint32_t max_steps; /* main-loop samples per ray, 1..65536 */
    uint32_t refine;    /* bisection samples of a hit, 0..32 */
    uint32_t flags;     /* 0, or CGRT_ISO_INSIDE_ABOVE */
} CgrtMarchParams;
typedef struct CgrtGridHit {
    float t;
    float value;
    uint32_t steps;
    uint32_t status; /* CGRT_MARCH_* */
    float gradient[3];
    uint32_t reserved; /* 0 */
} CgrtGridHit;
int cgrt_sample_grid(CgrtScene* scene, const CgrtGrid* grid, const float* values, const float* points, uint64_t n, const CgrtFieldParams* params,
                     float* value, float* gradient, uint8_t* inside);
int cgrt_sample_grid_device(CgrtScene* scene, const CgrtGrid* grid, const float* d_values, const float* d_points, uint64_t n,
                            const CgrtFieldParams* params, float* d_value, float* d_gradient, uint8_t* d_inside, void* stream);
int cgrt_march_grid(CgrtScene* scene, const CgrtGrid* grid, const float* values, const CgrtRay* rays, uint64_t n, const CgrtMarchParams* params,
                    CgrtGridHit* hits);
int cgrt_march_grid_device(CgrtScene* scene, const CgrtGrid* grid, const float* d_values, const CgrtRay* d_rays, uint64_t n,
                           const CgrtMarchParams* params, CgrtGridHit* d_hits, void* stream);
int cgrt_debug_march_work(CgrtScene* scene, const CgrtGrid* grid, const float* values, const CgrtRay* rays, uint64_t n,
                          const CgrtMarchParams* params, uint64_t* out3);

/* Grid fields, the adjoint of the sampler.  Value and gradient of cgrt_sample_grid are linear in `values`; these
 * entries apply the transpose of that map, so that a volume can be fitted to samples of its value and of its gradient, and so that points
 * can be deposited into a volume (with grad_value alone the adjoint IS the trilinear splat of the weights grad_value).  Given grad_value
 * (n f32, may be NULL) and grad_gradient (3n f32, may be NULL; not both), the gradients of some scalar with respect to the forward's
 * value and gradient outputs, they ADD the gradient with respect to the values into grad_values (nx ny nz f32 in the values' order).
 * `values` is not an argument.  Grid, limits, params, arithmetic and the meaning of fl() are those of "Grid fields" above.
 * Validity and cell.  Exactly the forward's, with the same bits: u_c, its clamp under CGRT_FIELD_CLAMP, the inside rule, i_c and f_c.
 *   params->outside is ignored.  A point the forward calls outside contributes nothing: its grad_value and grad_gradient are not read
 *   (a NaN there stays out) and it indexes nothing.
 * Contributions of an inside point, gv = grad_value[i], gg = grad_gradient[i].  Per axis c: w_c[0] = fl(1 - f_c), w_c[1] = f_c;
 *   s[0] = -1, s[1] = +1; with grad_gradient given, q_c = fl(gg_c / spacing.c).  For each corner (x, y, z) in {0, 1}^3:
 *     T_v = fl(gv fl(fl(w_x[x] w_y[y]) w_z[z]))
 *     T_x = fl((s[x] q_x) fl(w_y[y] w_z[z]))     T_y = fl((s[y] q_y) fl(w_x[x] w_z[z]))     T_z = fl((s[z] q_z) fl(w_x[x] w_y[y]))
 *   (s q is a change of sign and exact).  The contribution c_xyz is the sum, left to right and each sum rounded, of those of
 *   T_v, T_x, T_y, T_z whose input array was given: fl(fl(fl(T_v + T_x) + T_y) + T_z) with both, T_v alone with grad_value only,
 *   fl(fl(T_x + T_y) + T_z) with grad_gradient only.  The terms of a NULL input are left out of the sum, not added as zeros.
 *   c_xyz is added to grad_values at (i_x + x, i_y + y, i_z + z) UNLESS c_xyz == 0: a zero of either sign is not added, a NaN is not
 *   equal to 0 and is added.  An element that receives only zero contributions keeps its bits, a stored -0 included; a point on a grid
 *   point (f = 0 on all axes) with grad_value alone touches one element.  Each contribution is thus a defined f32 bit pattern, a pure
 *   function of (grid, point, gv, gg, flags).
 * Order and bound.  The order of the additions into one element is unspecified: the value is the sum, in f32, of the element's previous
 *   content and its contributions in SOME order (contributions of neighbouring points may be summed with each other first), and its last
 *   bits may differ from run to run.  For an element with m contributions c and previous content a, every such order obeys
 *     |got - exact| <= gamma(m + 1) * S + (m + 1) * 2^-126,   gamma(k) = k*u / (1 - k*u),  u = 2^-24,  S = |a| + sum |c|
 *   (exact: the sum of a and the f32 contributions, in real arithmetic); this is the bound the tests use.  The hardware add keeps
 *   subnormals on gfx950 (see the surface gradients above), so the absolute term is slack there; it stays in the bound.
 * Against real arithmetic.  With W = w_x w_y w_z and W_x = w_y w_z, W_y = w_x w_z, W_z = w_x w_y the REAL products of the real weights
 *   (1 - f_c, f_c) of the corner, the real adjoint coefficient is C = gv W + sum_c s_c (gg_c / spacing.c) W_c, and
 *     |c_xyz - C| <= K u (|gv| W + sum_c |gg_c / spacing.c| W_c),   K = 10,
 *   while no intermediate is subnormal.  Derivation: T_v carries six roundings (up to three of 1 - f, two weight products, the product
 *   with gv), a T_c five (the division, up to two of 1 - f, one weight product, the product with q_c); the three sums put at most three
 *   more on each term.  So every term is its real value times a product of at most nine factors (1 + d), |d| <= u, and
 *   |c_xyz - C| <= gamma(9) B with B the bracket above; gamma(9) = 9u / (1 - 9u) < 10 u.  (First order: 9; the count "1 - f, division,
 *   two products, the product with g, three sums" gives 8 when a single 1 - f is counted.)
 * Scale symmetries, as property (d) above.  Multiplying grad_value and grad_gradient by 2^k multiplies every contribution by 2^k
 *   exactly while every non-zero one of q_c, T_v, T_x, T_y, T_z and the partial sums, times 2^k, stays a normal float (the weights do not
 *   move).  Multiplying origin, spacing and the points by 2^k leaves u, i, f, the weights and T_v alone and multiplies q_c, hence T_x,
 *   T_y, T_z, by 2^-k exactly while every non-zero one of p.c, origin.c, p.c - origin.c, spacing.c, q_c, T_x, T_y, T_z times the scale
 *   stays normal; the contribution of a call with grad_value only does not move, that of a call with grad_gradient only is multiplied
 *   by 2^-k exactly (its partial sums inside the same envelope), and with both the sum mixes the two and only the terms obey it.
 *   Outside the envelope the bytes are still the defined ones; only the relation to scale 1 is lost.
 * Forms.  cgrt_sample_grid_grad takes host pointers, runs on a call lane like cgrt_sample_grid and blocks; any number of threads may
 *   call at once; grad_values goes up, is added into and comes back.  cgrt_sample_grid_grad_device only enqueues on `stream` (NULL =
 *   default stream) and reads nothing back.
 * Checks, all CGRT_E_ARG, in this order and before any device work: NULL scene or grid; the grid's limits (the forward's); an unknown
 *   flag in params (NULL params means flags 0); NULL points with n > 0; both grads NULL; NULL grad_values; n > 0x7fffffff; (device form) a
 *   pointer not 4-byte aligned.  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0 succeeds and touches nothing.  Device form: then
 *   d_points (12 n), each grad given (4 n, 12 n) and d_grad_values (4 bytes per grid point) checked as device memory of the scene's device.
 *   Nothing outside the nx ny nz elements is written.  No form reads or writes the prediction record, the frame hints, the layout or any
 *   frame state.  Overlap of grad_values with an input is the caller's error and is not checked.
 * Not offered: reproducible bits from THESE entries (the cgrt_sample_grid_grad_repro* entries below are the bitwise-reproducible form);
 *   gradients of the march's hit record (re-sample the hit point: README); second derivatives with respect to the points;
 *   vector-valued or batched grids; f16 / bf16; the C++ host mirror. */
int cgrt_sample_grid_grad(CgrtScene* scene, const CgrtGrid* grid, const float* points, uint64_t n, const CgrtFieldParams* params,
                          const float* grad_value, const float* grad_gradient, float* grad_values);
int cgrt_sample_grid_grad_device(CgrtScene* scene, const CgrtGrid* grid, const float* d_points, uint64_t n, const CgrtFieldParams* params,
                                 const float* d_grad_value, const float* d_grad_gradient, float* d_grad_values, void* stream);

/* Grid fields, the bitwise-reproducible form of the sampler's adjoint.  An opt-in second form of the entries
 * above whose result is a pure function of the call's inputs, as the *_grad_repro* entries of the surface attributes are for the table
 * adjoint: one definition of "reproducible" for the library.  The entries above are unchanged.
 * Definition.  Validity, cell and contributions are those of cgrt_sample_grid_grad, bit for bit: u, its clamp, the inside rule, i and f
 * (field_cell), the eight c_xyz with the terms of a NULL input left out (field_adjoint); an outside point is neither read nor indexed.
 * A contribution that compares equal to zero is NOT a contribution, as in the float form (this is where the grid form departs from
 * the surface form, where +-0 counts): an element that receives only zeros is untouched.  Every dim is at least 2, so the eight corners
 * of a point are eight distinct elements: an element receives at most one contribution per point, m <= n.  For an element with previous
 * content a and contributions x_1..x_m (m >= 1), n the call's point count:
 *   S = min(24, 38 - bitlength(n))                        (n <= 0x7fffffff, so S >= 7)
 *   a finite x_j is +-M_j * 2^(e'_j - 150), e'_j = max(exponent field, 1), M_j the 24-bit significand (a subnormal: no implicit bit)
 *   E = max_j e'_j,  d_j = E - e'_j
 *   T_j = +-(M_j << (S - d_j)) if d_j <= S, else +-(M_j >> (d_j - S))   (the magnitude is truncated; 0 once the shift reaches 24)
 *   I = sum_j T_j in int64                                (no overflow: |I| < 2^(24 + S) * n <= 2^62)
 *   new value = fl32( fl64(a) + fl64(I) * 2^(E - 150 - S) )
 * fl64(I) is the round-to-nearest-even conversion, the scaling is exact, the sum is rounded to double and then once to float,
 * subnormals kept.  If any x_j is not finite the element becomes fl32(a + s), s = NaN if a NaN contribution is present or both +inf and
 * -inf are, else the infinity that is present.  Every NaN result is stored as the quiet NaN 0x7fc00000.  Elements without a contribution
 * are neither read nor written: a stored -0, a signalling-NaN payload and a sentinel byte pattern survive.  An element whose
 * contributions all truncate to T = 0 is still touched and becomes fl32(fl64(a) + 0).
 * Properties.
 *   (a) Order-freedom.  E is a maximum, the kinds an OR, I an integer sum: all three are associative and commutative, and the last step
 *       is a function of (a, E, kinds, I, S) alone.  So the result does not depend on the order of the additions, the mapping of lanes
 *       to points, a permutation of the points, the stream, the thread or the run.
 *   (b) A legal value of the float form.  Write sigma = 2^(E - 150 - S), X = sum x_j in real arithmetic, S_abs = |a| + sum |x_j|.
 *       x_j = T_j sigma exactly when d_j <= S; otherwise the truncation loses less than sigma, towards zero.  If E = 1 every d_j is 0
 *       and nothing is lost; else the largest contribution is normal, |x_max| >= 2^(23 + S) sigma, so sigma <= 2^(1 - S) u |x_max| and
 *       |I sigma - X| < (m - 1) sigma <= (m - 1) 2^(1 - S) u |x_max| <= (m - 1) u |x_max| / 64 (S >= 7).  fl64(I) is exact below 2^53
 *       and within 2^-53 relative above, the scaling is exact, the double sum adds 2^-53 relative and the rounding to float u relative,
 *       or at most 2^-150 absolute among subnormals.  Together
 *         |new - (a + X)| <= u S_abs (1 + (m - 1) / 64 + 2^-27) + 2^-150 <= gamma(m + 1) S_abs + (m + 1) 2^-126
 *       since gamma(m + 1) >= (m + 1) u and m >= 1: the bound of cgrt_sample_grid_grad holds for every element (the tests assert it
 *       with none excluded), so the result is one the float form may return.
 *   (c) Per call.  S depends on n, and E on the call's contributions: a gradient accumulated over several calls is reproducible because
 *       each call is, and equals no single larger call.
 *   (d) Scale.  With a = 0, multiplying grad_value and grad_gradient by 2^k multiplies every contribution by 2^k exactly (the scale
 *       symmetry of the entries above, inside its envelope), hence every e'_j and E by +k, every d_j, T_j and I not at all, and the
 *       result by 2^k exactly while it stays a normal float.
 *   (e) Exact data.  Where every sum is exact in f32 in every order (no d_j exceeds S, I 2^(E - 150 - S) = X exactly and a + X is a
 *       float), the result is the float form's.
 * Workspace.  cgrt_sample_grid_grad_repro_workspace reports the bytes a call on `grid` needs: 12 per grid element, 12 nx ny nz (a 64-bit
 * accumulator and a 32-bit exponent / kind word each); it applies the grid's limit checks (NULL scene, grid or bytes: CGRT_E_ARG).
 * The device form takes it as d_workspace / workspace_bytes: device memory of the scene's device, 8-byte aligned, contents need no
 * initialisation (the launch clears it), owned by the caller, and not to be shared by calls in flight at the same time.
 * Forms.  cgrt_sample_grid_grad_repro_device only enqueues on `stream` (NULL = default stream) and reads nothing back: a clear of the
 * workspace, two passes over the points (integer atomic max / or into the word; 64-bit integer atomic add into the accumulator) and one
 * pass over the grid, which reads and writes the touched elements of d_grad_values alone.  cgrt_sample_grid_grad_repro takes host
 * pointers, runs on a call lane like cgrt_sample_grid_grad, blocks, and allocates the workspace itself.
 * Checks.  Those of the float twin, in its order (CGRT_E_ARG); then d_workspace NULL, not 8-byte aligned or workspace_bytes too small
 * (CGRT_E_ARG; a call with n == 0 skips these); then a host-only scene: CGRT_E_NO_DEVICE; n == 0 succeeds and touches nothing; then
 * the extents of the device buffers, the workspace included.  No form reads or writes the prediction record, the frame hints, the
 * layout or any frame state.
 * Not offered: a form reproducible across a split into several calls; merging the lanes of a wave that share a cell (DESIGN.md section
 * 9); f16 / bf16 grids; the C++ host mirror. */
int cgrt_sample_grid_grad_repro_workspace(CgrtScene* scene, const CgrtGrid* grid, uint64_t* bytes);
int cgrt_sample_grid_grad_repro(CgrtScene* scene, const CgrtGrid* grid, const float* points, uint64_t n, const CgrtFieldParams* params,
                                const float* grad_value, const float* grad_gradient, float* grad_values);
int cgrt_sample_grid_grad_repro_device(CgrtScene* scene, const CgrtGrid* grid, const float* d_points, uint64_t n,
                                       const CgrtFieldParams* params, const float* d_grad_value, const float* d_grad_gradient,
                                       float* d_grad_values, void* d_workspace, uint64_t workspace_bytes, void* stream);

/* Visibility queries: the reference's second question, "is this point visible?" (DESIGN.md section 5.12).  One byte (or one count) per
 * answer instead of a 16-byte hit; every answer equals the reference's own, whatever the walk (certified or exact) and the kernel shape.
 * The queries neither read nor write the scene's frame prediction or frame hints.  The host forms (host pointers, synchronous) run on a
 * call lane like cgrt_intersect_batch: any number of threads may query one scene at once.
 *
 * cgrt_occluded: hit[i] = the bool BoundingVolumeHierarchy::intersect(rays[i], hitInfo) returns (bvh.cpp:850-881) -- true iff a triangle
 * or a sphere is hit before rays[i].t.  The ray is taken as given, t included (the `t >= ray.t` rule): a segment query sets t to the
 * segment's length.  The meshes are searched with the any-hit walk (the first leaf that accepts a triangle ends it, as the soft-shadow
 * samples of cgrt_render_soft end); the spheres are tested only when no mesh accepted a triangle (bvh.cpp:875-880).  hit[i] is 0 or 1.
 * Kernel shape by the list's size, as cgrt_intersect_batch (cgrt_set_kernel_shape forces it).
 * Checks, all CGRT_E_ARG, in this order: NULL scene, or NULL rays or hit with n > 0; n > 0x7fffffff; (device form) d_rays not 4-byte
 * aligned.  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0 succeeds and touches nothing.  Device form: then d_rays (n * 28 bytes) and
 * d_hit (n bytes) not device memory of the scene's device (as cgrt_shade_rays_device checks them) -> CGRT_E_ARG, before any device work.
 * cgrt_occluded_device reads no host array: it only enqueues on `stream` (NULL = default stream), asynchronously, like
 * cgrt_intersect_batch_device. */
int cgrt_occluded(CgrtScene* scene, const CgrtRay* rays, uint64_t n, uint8_t* hit);
int cgrt_occluded_device(CgrtScene* scene, const CgrtRay* d_rays, uint64_t n, uint8_t* d_hit, void* stream);
/* cgrt_in_shadow: out[i * nlights + l] = pointInShadow(points[i], lights[l], bvh) (main.cpp:104-135) for every point and light: the ray
 * from point + 0.001f * dir towards the light, in shadow iff `hit && !(ray.t + 0.001f >= |fromPosToLight|)`.  points: n x 3 floats;
 * lights: nlights x 6 floats {position, colour} as the render entries take them (colour ignored), a HOST pointer in both forms.  The ray
 * is built by the frame's own expressions and walked as the frame's shadow lists are (bounded by the light's distance).
 * Kernel shape by n * nlights, as a ray list of that length.
 * Checks, all CGRT_E_ARG, in this order: NULL scene, NULL points or out with n > 0, or nlights > 0 with NULL lights; n > 0x7fffffff or
 * n * nlights > 0x7fffffff; (device form) d_points not 4-byte aligned.  Then a host-only scene: CGRT_E_NO_DEVICE.  n == 0 or nlights == 0
 * succeeds and touches nothing.  Device form: then d_points (n * 12 bytes) and d_out (n * nlights bytes) checked as device memory of the
 * scene's device -> CGRT_E_ARG.
 * cgrt_in_shadow_device: ordered like cgrt_shade_rays_device -- the work runs after everything enqueued on `stream` before the call, and
 * the call returns when the answers are in d_out (the light table goes up through the library's own staging).  The stream is not kept. */
int cgrt_in_shadow(CgrtScene* scene, const float* points, uint64_t n, const float* lights, uint32_t nlights, uint8_t* out);
int cgrt_in_shadow_device(CgrtScene* scene, const float* d_points, uint64_t n, const float* lights, uint32_t nlights, uint8_t* d_out,
                          void* stream);
/* cgrt_soft_lit: lit[i * nspherical + l] = the number of the `samples` soft-shadow rays of spherical light l that reach points[i]
 * (shading's loop, main.cpp:168-200: !intersect || ray.t > lightT).  Sample smp draws as cgrt_render_soft does with pixel = i and level 0
 * -- cgrt_shade_rays' convention for its rays -- so the counts of a ray's level-0 hit point are the counts its shading uses.
 * soft->closest_hit as in cgrt_render_soft (0: any-hit sample rays, 1: closest hit; the counts are equal).  soft == NULL: no lights.
 * Checks, all CGRT_E_ARG, in this order: NULL scene, or NULL points or lit with n > 0; n > 0x7fffffff or n * nspherical > 0x7fffffff;
 * bad soft (cgrt_shade_rays' rules); (device form) d_points or d_lit not 4-byte aligned.  Then a host-only scene: CGRT_E_NO_DEVICE.
 * n == 0 or nspherical == 0 succeeds and touches nothing.  Device form: then d_points (n * 12 bytes) and d_lit (n * nspherical * 4 bytes)
 * checked as device memory of the scene's device -> CGRT_E_ARG.
 * cgrt_soft_lit_device: d_lit is zeroed and counted behind everything enqueued on `stream` before the call; the call returns when the
 * counts are in place (soft's tables are host arrays, as in cgrt_shade_rays_device). */
int cgrt_soft_lit(CgrtScene* scene, const float* points, uint64_t n, const CgrtSoftShadows* soft, uint32_t* lit);
int cgrt_soft_lit_device(CgrtScene* scene, const float* d_points, uint64_t n, const CgrtSoftShadows* soft, uint32_t* d_lit, void* stream);

/* Work counters of the same traversal (separate instrumented launch; not part of any timed region). */
int cgrt_count_primary(CgrtScene* scene, const CgrtCamera* cam, int W, int H, int x0, int y0, int x1, int y1,
                       int rank, int nranks, CgrtCounters* out);
int cgrt_count_batch(CgrtScene* scene, const CgrtRay* rays, uint64_t n, CgrtCounters* out);
/* Diagnostic (not part of the reference surface): one stamped + instrumented full-frame launch; out holds 16 u64
 * per 8x8 tile (= wave): s_memtime start, end; s_memrealtime start, end; lane-summed inner/leaf/tri/sub steps;
 * wave-level iterations of the inner, sub-node and triangle bodies; per-lane maxima of inner/leaf/tri/sub; active
 * lanes.  One record per launched wave: cap_waves >= 4 * 16 * 8 * ceil(ceil(W/64)*ceil(H/64) / 8). */
int cgrt_debug_wave_times(CgrtScene* scene, const CgrtCamera* cam, int W, int H, uint64_t* out, uint64_t cap_waves);
/* Diagnostic: the frame's shadow-list launchers on the caller's point-light shadow rays (origin, direction and t as k_spawn
 * writes them, dist[i] = |fromPosToLight|).  hits[i] is what the frame's k_shade reads: the ray is in shadow iff
 * `hit && !(t + 0.001f >= dist[i])` (main.cpp:104-135); t and prim_id need not be the closest ones.  `how` picks the path:
 *   0  launch_trace_shadow, n known on the host;
 *   1  launch_trace_shadow with the length in a device word: the word holds n / dmul (n % dmul == 0), the list dmul x that, the
 *      grid covers `capacity` >= n rays; expected = the host's estimate that picks the kernel shape (0: chosen on the device);
 *   2  launch_trace_pair: the shadow list as in 1, beside a mirror list of nmirror closest-hit rays whose length is in a device word of
 *      its own (grid for mirror_capacity >= nmirror rays, mirror_expected as expected); CGRT_E_ARG when the scene or the forced
 *      kernel shape does not allow the paired launch.
 * Every result is filled with the byte 0xA5 before the launch: an entry the kernel did not write keeps it.  hits receives n
 * entries (how 0) or max(n, capacity); mirror_hits / mirror_normals (how 2) max(nmirror, mirror_capacity) entries. */
int cgrt_debug_trace_shadow(CgrtScene* scene, const CgrtRay* rays, const float* dist, uint64_t n, int how, uint32_t dmul, uint64_t capacity,
                            uint64_t expected, const CgrtRay* mirror_rays, uint64_t nmirror, uint64_t mirror_capacity, uint64_t mirror_expected,
                            CgrtHit* mirror_hits, float* mirror_normals, CgrtHit* hits);
/* Diagnostic: the frame's soft-shadow launcher (launch_soft_shadow, main.cpp:168-200) on caller items: item i is the ray
 * item_rays[i] with its hit item_hits[i] (pointOn = origin + direction * hit.t; items with hit == 0 count nothing), sampled as
 * pixel item_pixels[i] at recursion level `level` (soft->spherical, unit_vectors, samples, seed as cgrt_render_soft; closest_hit
 * is ignored).  anyhit: 1 = the first accepting leaf ends a sample ray (the frame's default), 0 = the full closest hit.
 * lit[i * nspherical + l] receives the number of samples of light l that reach item i. */
int cgrt_debug_soft_lit(CgrtScene* scene, const CgrtRay* item_rays, const CgrtHit* item_hits, const int32_t* item_pixels, uint64_t nitems,
                        const CgrtSoftShadows* soft, int level, int anyhit, uint32_t* lit);
/* Diagnostic: `repeats` launches of a kernel that reads nrecords scattered 64-byte records (one per lane, never twice)
 * from a zeroed table -- a known HBM byte count in the traversal kernels' access shape, for calibrating rocprofv3's
 * FETCH_SIZE on gfx950 (tools/calibrate_fetch_size.sh). */
int cgrt_debug_gather_calibration(int device, uint64_t nrecords, int repeats);
/* Diagnostic: the kernels' 4-operation exact division (trace_kernels.hip fdiv4) against IEEE a[i] / d[i] on the
 * device; mismatches receives the count, first_bad {a, d, got, expected} of the first one. */
int cgrt_debug_fastdiv_check(int device, const float* a, const float* d, uint64_t n, uint64_t* mismatches, float* first_bad);
/* Diagnostic: validates every reference of the scene's record arrays on the host (tree child references, leaf references
 * in both encodings, accelerator nodes and runs, each triangle reachable exactly once).  Works on host-only scenes. */
int cgrt_debug_check_layout(CgrtScene* scene);
/* Diagnostic: FNV-1a hash over every array the device reads (node packets, accelerator + fast-tree nodes, triangle records, leaf
 * table, vertex normals, certificate paths, leaf of every record, roots): two builds of the same scene must agree, whatever the
 * number of builder threads (cgrt_set_build_threads: 0 = hardware concurrency, at most 16 are used; process-wide, for scenes
 * created afterwards).  Works on host-only scenes. */
int cgrt_debug_layout_hash(const CgrtScene* scene, uint64_t* out);
/* Diagnostic: the 4-wide nodes of the in-leaf accelerators and of the fast tree as the device reads them (128 bytes
 * = 32 words each, transposed quarters).  cgrt_debug_node_pack writes four child boxes (boxes[6 * c ..] = lower.xyz, upper.xyz of
 * child c), four child references and an accelerator root's leaf index into the 32 words of one node through the builder's own
 * store helpers; cgrt_debug_node_unpack reads them back through the matching load helpers.  cgrt_debug_get_subnodes copies the
 * scene's node array (16 words per 64-byte half, cgrt_num_subnodes halves; `words` may be NULL), the record index of its first half,
 * the fast tree's root reference (0xffffffff: none) and, per reference leaf, the record index of its accelerator's root node
 * (0xffffffff: the leaf has none; `leaf_roots` may be NULL, else cgrt_num_nodes entries are enough).  Works on host-only scenes. */
void cgrt_debug_node_pack(const float* boxes, const uint32_t* refs, uint32_t leaf_index, uint32_t* words);
void cgrt_debug_node_unpack(const uint32_t* words, float* boxes, uint32_t* refs, uint32_t* leaf_index);
int cgrt_debug_get_subnodes(const CgrtScene* scene, uint32_t* words, uint32_t* sub_base, uint32_t* fast_root, uint32_t* leaf_roots, uint32_t* nleaves);
int cgrt_set_build_threads(int threads);
/* Bytes of one inner-node record / one triangle record / one in-leaf accelerator node / one result. */
void cgrt_record_sizes(uint32_t* node_bytes, uint32_t* tri_bytes, uint32_t* sub_bytes, uint32_t* hit_bytes);

/* Element-wise device versions of the free functions of src/ray_tracing.h:10-20 and startsInBox
 * (bvh.cpp:647-661); element i of every array belongs to call i.  Host pointers; synchronous.
 *   cgrt_ray_triangle_batch  intersectRayWithTriangle (ray_tracing.cpp:86-114)
 *       tri: n x 18 floats {v0 v1 v2 n1 n2 n3}; t_io: n floats in/out; hit: n bytes; normals n x 3 (written on hit)
 *   cgrt_ray_plane_batch     intersectRayWithPlane (ray_tracing.cpp:40-72); plane: n x 4 {D, normal}
 *   cgrt_ray_box_batch       intersectRayWithShape(AxisAlignedBox) (ray_tracing.cpp:162-200) and startsInBox;
 *       box: n x 6 {lower, upper}; inside: n bytes (optional)
 *   cgrt_ray_sphere_batch    intersectRayWithShape(Sphere) (ray_tracing.cpp:118-158); sphere: n x 4 {center, radius}
 *   cgrt_triangle_plane_batch trianglePlane (ray_tracing.cpp:74-82); tri: n x 9 -> plane n x 4 {D, normal}
 *   cgrt_point_in_triangle_batch pointInTriangle (ray_tracing.cpp:23-38); in: n x 15 {v0 v1 v2 n p} */
int cgrt_ray_triangle_batch(int device, const float* tri, const CgrtRay* rays, uint64_t n, float* t_out, uint8_t* hit,
                            float* normals);
int cgrt_ray_plane_batch(int device, const float* plane, const CgrtRay* rays, uint64_t n, float* t_out, uint8_t* hit);
int cgrt_ray_box_batch(int device, const float* box, const CgrtRay* rays, uint64_t n, float* t_out, uint8_t* hit,
                       uint8_t* inside);
int cgrt_ray_sphere_batch(int device, const float* sphere, const CgrtRay* rays, uint64_t n, float* t_out, uint8_t* hit,
                          float* normals);
int cgrt_triangle_plane_batch(int device, const float* tri, uint64_t n, float* plane);
int cgrt_point_in_triangle_batch(int device, const float* in, uint64_t n, uint8_t* out);

int cgrt_device_count(void);
const char* cgrt_last_error(void);
const char* cgrt_version(void);
/* First 16 hex digits of the sha256 over the library's sources (every .hip, .cpp and .h file of csrc + this header, in name order) at build time:
 * ties a committed profile to the kernels it was measured on (bench.py nulls roofline.traffic / roofline.measured when it differs). */
const char* cgrt_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* CGRT_H */
