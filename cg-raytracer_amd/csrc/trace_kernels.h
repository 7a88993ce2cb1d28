// trace_kernels.h -- host-callable launchers of the gfx950 kernels in trace_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgrt_layout.h"
#include "spawn_rays.h"

namespace cgrt {

static const unsigned CGRT_QUEUE_BLOCK_WORDS = 32 * 9;

// Device mirror of CgrtHit (include/cgrt.h), 16 B.
struct CgrtHitDev {
    float t;
    uint32_t prim_id;
    int32_t material_id;
    uint32_t hit;
};

// Soft-shadow sampling of spherical lights (main.cpp:168-218) for one recursion level.
struct SoftDev {
    const float* lights;  // nlights x 7 {position, radius, color} (SphericalLight, scene.h:47-51)
    const float* units;   // nunits x 3 unit vectors: the randomUnitVector() draws (main.cpp:46-59)
    uint32_t nlights, samples, nunits, seed, level;
    uint32_t view_pixels;  // 0, or W * H of a multi-view frame: samples are drawn with item_pixels[item] % view_pixels (k_soft_shadow)
    // light sets (k_soft_shadow_sets): lights are the batch's distinct (position, radius, in-set index) keys, and key l draws as light
    // set_index[l] -- its index within its own set, as that set's single frame draws it.  NULL otherwise.  With view_pixels as well (a
    // multi-view batch of light sets, k_soft_shadow_views_sets / k_soft_shadow_sets_strided) both rules hold.
    const uint32_t* set_index;
};

// A batch of light sets on the device (capi_frames.h LightSetSrc; cgrt_render_light_sets*): set b holds the point lights point_off[b] ..
// point_off[b + 1] - 1 and the spherical lights sph_off[b] .. sph_off[b + 1] - 1, in the caller's order.  Light k is two float4s
// {position, slot}, {colour, 0}; slot (the bits of .w) is its distinct entry: the light index k_spawn traced its shadow ray with, or
// the soft-shadow key whose samples k_soft_shadow_sets counted.
struct SetsDev {
    const uint32_t* point_off;
    const uint32_t* sph_off;
    const float4* point;
    const float4* sph;
    uint32_t nsets;
};

// How a launch covers its list of n entries.  GRID_FULL: one thread per entry; with dcount (optional: the device word with the list's
// length) n is the capacity the grid covers and the kernel stops at *dcount.  GRID_STRIDED (enqueued frames):
// dcount is required, and at most strided_waves() waves stride over the *dcount entries present, in the shape the full grid has (a forced
// quad shape: the full grid itself), with the full grid's results.  A combination without a kernel is hipErrorInvalidValue.
enum ListGrid { GRID_FULL, GRID_STRIDED };
unsigned strided_waves();
unsigned strided_blocks(unsigned full, unsigned block);  // workgroups of a GRID_STRIDED launch whose full grid has `full` of `block` threads
// A ray list: n rays (the capacity the grid covers), *dcount (optional) of them present; expected (with dcount): the host's estimate of
// *dcount picks the kernel shape.  A shadow list holds pointInShadow's rays (main.cpp:104-135), *dcount x dmul of them: hits[i] decides
// `hit && !(t + 0.001f >= dist[i])` like the reference's closest hit does.
struct RayList {
    const float* rays;
    unsigned long long n;
    CgrtHitDev* hits;
    float* normals;
    const uint32_t* dcount;
    unsigned long long expected;
};
struct ShadowList {
    const float *rays, *dist;
    unsigned long long n;
    CgrtHitDev* hits;
    const uint32_t* dcount;
    unsigned dmul;  // (0: 1)
    unsigned long long expected;
};
// threads per workgroup the ray-list kernels (batch, soft shadow) are launched with for this scene; frames carry theirs in FrameDev::block
int trace_block(const SceneDev& S);
// kernel shape per launch (walk_quad.h): mode -1 = by size (launches of at most max_rays rays take the quad shape), 0 = never, 1 = always;
// max_rays 0 keeps the current threshold.  Results do not depend on the shape.
void set_quad_shape(int mode, unsigned long long max_rays);
void get_quad_shape(int* mode, unsigned long long* max_rays);
bool quad_shape_for(const SceneDev& S, unsigned long long rays);
// counters (optional): 5 x u64 device words {rays, inner_visits, leaf_visits, tri_tests, sub_visits}, accumulated.
hipError_t launch_trace_primary(const SceneDev& S, const CameraDev& C, const FrameDev& F, CgrtHitDev* hits, float* normals,
                                unsigned long long* counters, hipStream_t stream);
// Frame order (FrameDev::order).  A profile frame: the plain frame of a launch for which can_profile_frame holds, whose
// waves leave their longest wall time per super-tile in ticks[(nst_rank + 7) / 8 * 8] (u32, 10 ns; zeroed on the stream in front of
// the launch); the builder turns ticks into a table of as many u16 entries (live: the builder's threshold, CGRT_ORDER_LIVE_TICKS).
bool can_profile_frame(const SceneDev& S, const FrameDev& F);
hipError_t launch_trace_primary_profile(const SceneDev& S, const CameraDev& C, const FrameDev& F, CgrtHitDev* hits, float* normals,
                                        uint32_t* ticks, hipStream_t stream);
hipError_t launch_build_frame_order(const uint32_t* ticks, uint32_t nst, uint32_t live, uint16_t* out, hipStream_t stream);
// persistent variant: queue = CGRT_QUEUE_BLOCK_WORDS zeroed u32 (8 heads + exit counter, one 128-B line each) owned by this launch; blocks = persistent grid size
hipError_t launch_trace_primary_persistent(const SceneDev& S, const CameraDev& C, const FrameDev& F, CgrtHitDev* hits, float* normals,
                                           unsigned long long* counters, unsigned int* queue, unsigned blocks, hipStream_t stream);
// diagnostic: stamps = 4 x ntiles_rank u64 {memtime start, end, memrealtime start, end} per wave
hipError_t launch_trace_primary_stamped(const SceneDev& S, const CameraDev& C, const FrameDev& F, CgrtHitDev* hits,
                                        unsigned long long* stamps, hipStream_t stream);
hipError_t launch_trace_batch(const SceneDev& S, const RayList& R, unsigned long long* counters, hipStream_t stream, ListGrid grid = GRID_FULL);
// every triangle, no tree (ray_tracing.cpp:202-213); mesh < 0: all meshes + spheres
hipError_t launch_brute_batch(const SceneDev& S, const float* rays, unsigned long long n, int mesh, CgrtHitDev* hits, float* normals, hipStream_t s);
hipError_t launch_trace_shadow(const SceneDev& S, const ShadowList& A, unsigned long long* counters, hipStream_t stream, ListGrid grid = GRID_FULL);
// a level's two lists in ONE launch, workgroups dealt alternately; can_trace_pair: a fast tree and no forced quad shape
bool can_trace_pair(const SceneDev& S);
hipError_t launch_trace_pair(const SceneDev& S, const ShadowList& A, const RayList& B, hipStream_t stream, ListGrid grid = GRID_FULL);
// *flag = value (system scope) once everything queued on the stream before it has finished
hipError_t launch_signal(uint32_t* flag, uint32_t value, hipStream_t stream);
hipError_t launch_generate_rays(const CameraDev& C, int W, int H, int x0, int y0, int x1, int y1, float* rays, hipStream_t stream);
// the rays of a ray camera's whole W x H frame, row-major (cgrt_generate_rays_raycam)
hipError_t launch_generate_rays_raycam(const RayCameraDev& C, int W, int H, float* rays, hipStream_t stream);
// lit[item * nlights + l] += samples of spherical light l that reach item's hit point (zeroed by the caller); GRID_STRIDED light sets: views only
hipError_t launch_soft_shadow(const SceneDev& S, const SoftDev& Q, const float* rays, const CgrtHitDev* hits, const int* item_pixels,
                              unsigned long long nitems, uint32_t* lit, int anyhit, hipStream_t stream, const uint32_t* dcount = nullptr,
                              ListGrid grid = GRID_FULL);
// the same count from the caller's points (npoints x 3 floats), point i sampled as pixel i at level Q.level (cgrt_soft_lit*)
hipError_t launch_soft_points(const SceneDev& S, const SoftDev& Q, const float* points, unsigned long long npoints, uint32_t* lit, int anyhit,
                              hipStream_t stream);
// visibility queries (k_visibility), one byte per answer, laid out by the list's shape: out[i] = BoundingVolumeHierarchy::intersect's bool
// for rays[i] (cgrt_occluded*); out[i * nlights + l] = pointInShadow(points[i], light l) with lights nlights x 6 floats (cgrt_in_shadow*)
hipError_t launch_occluded(const SceneDev& S, const float* rays, unsigned long long n, uint8_t* out, hipStream_t stream);
hipError_t launch_in_shadow(const SceneDev& S, const float* points, unsigned long long npoints, const float* lights, unsigned nlights, uint8_t* out,
                            hipStream_t stream);

// primary frame for the shading wavefront: only the hits, appended to a compact list; count = one zeroed device word
hipError_t launch_trace_primary_compact(const SceneDev& S, const CameraDev& C, const FrameDev& F, float* rays, CgrtHitDev* hits, float* normals,
                                        int* pixels, uint32_t* count, hipStream_t stream, unsigned long long* counters = nullptr,
                                        float* rgb = nullptr, const SpawnDev* spawn = nullptr);  // spawn (device memory): level 0's k_spawn fused in (spawn_rays.h)  // rgb (optional): the rank's pixels are cleared by the same kernel
// multi-view frames (F.views set, F.nst_rank = nviews x F.view_st: capi.cpp make_views_frame): the VIEWS instantiations of the two
// primary kernels, pixel = view * W * H + y * W + x.  No counters, no hints, no fused spawn; the kernel shape as for a frame.
// raycams: the table is F.raycams (ray cameras, cgrt_*_raycams*: the RAYCAM instantiations) instead of F.views.
hipError_t launch_trace_primary_views(const SceneDev& S, const FrameDev& F, CgrtHitDev* hits, float* normals, hipStream_t stream, bool raycams = false);
hipError_t launch_trace_primary_views_compact(const SceneDev& S, const FrameDev& F, float* rays, CgrtHitDev* hits, float* normals, int* pixels,
                                              uint32_t* count, float* rgb, hipStream_t stream, bool raycams = false);
// level 0 of the shading wavefront from a caller's list of n rays (cgrt_shade_rays, k_trace_list_compact): rgb[3i..3i+2] := 0 for every
// i, the rays that hit appended to the compact list {rays, hits, normals, pixels = i}; count = one zeroed device word.  Laid out by the
// list's shape (list_shape), as launch_trace_batch.
hipError_t launch_trace_list_compact(const SceneDev& S, const float* in_rays, unsigned long long n, float* rays, CgrtHitDev* hits, float* normals,
                                     int* pixels, uint32_t* count, float* rgb, hipStream_t stream, unsigned long long* counters = nullptr);
hipError_t launch_clear_owned(const FrameDev& F, float* rgb, hipStream_t stream);
// shading wavefront (shade_kernels.hip); every level is a compact list of live paths
// One level of it, as the launchers below take it: typed device pointers into the frame's workspace (capi_frames.cpp Wavefront::level -- the
// only place that knows which buffer set a level lives in).  A plain value, built on the stack per launch group.
struct LevelDev {
    float* rays;  // the level's list: a ray, a hit, a normal and a pixel per entry
    CgrtHitDev* hits;
    float* normals;
    int* pixels;
    float *srays, *sdist;  // its shadow list (k_spawn appends, the shadow traversal fills shits)
    int* sslot;
    CgrtHitDev* shits;
    float* lvl;          // its level record: lvl[2i] = {direct light, flags} (k_shade), lvl[2i+1] = {ks, child} (k_spawn)
    uint32_t* counters;  // its counter block: 3 device words {shadow rays appended, mirror rays appended, hits}, zeroed by the caller
    float* sets;         // light sets: set b's colour of entry i at sets + 4 * (b * stride + i) = {colour, flags}; NULL otherwise
    int spawn;           // the level spawns mirror rays (level + 1 < max_level) ...
    float* next_rays;    // ... into the next level's list
    CgrtHitDev* next_hits;
    float* next_normals;
    int* next_pixels;
    const float *child_lvl, *child_sets;  // the next level's record and per-set colours (NULL: there is no next level)
    unsigned long long stride;            // entries the lists are sized for
    unsigned nsets;                       // 1 without light sets
    // its shadow list and its mirror list (the next level's), of capacity n
    ShadowList shadow_list(unsigned long long n, const uint32_t* dc, unsigned dmul = 1, unsigned long long expected = 0) const {
        return {srays, sdist, n, shits, dc, dmul, expected};
    }
    RayList mirror_list(unsigned long long n, const uint32_t* dc, unsigned long long expected = 0) const { return {next_rays, n, next_hits, next_normals, dc, expected}; }
};
// What does not change over a frame.  lights: the point lights k_spawn traces shadow rays to (light sets: the batch's distinct positions,
// sslot's row); slights: the spherical lights whose samples `lit` counts (light sets: the distinct keys, lit's row).
struct FrameConst {
    const float *materials, *lights;
    unsigned nlights;
    const float* slights;
    unsigned nslights;
    const uint32_t* lit;
    unsigned samples;
    float* rgb;                       // the frame the colours are scattered into
    unsigned long long frame_pixels;  // pixels of one frame in it (light sets, views: W * H)
};
// k_spawn: shadow rays of every hit -> the level's shadow list; mirror rays -> the next level's list; lvl[2i+1] = {ks, child}
hipError_t launch_spawn(const LevelDev& V, const FrameConst& K, unsigned long long n, hipStream_t s, const uint32_t* dcount = nullptr,
                        ListGrid grid = GRID_FULL);
// k_shade: lvl[2i] = {direct light, flags}
hipError_t launch_shade(const LevelDev& V, const FrameConst& K, unsigned long long n, hipStream_t s, const uint32_t* dcount = nullptr,
                        ListGrid grid = GRID_FULL);
// colour of the level's entries += colour of their child (the next level) * ks  (main.cpp:262)
hipError_t launch_fold(const LevelDev& V, unsigned long long n, hipStream_t s, const uint32_t* dcount = nullptr, ListGrid grid = GRID_FULL);
// level 0's colours to K.rgb; with_child: level 0 is folded with level 1 on the fly (colour + childColour * ks, main.cpp:262) instead of
// by launch_fold
hipError_t launch_write_rgb(const LevelDev& V0, const FrameConst& K, bool with_child, unsigned long long n, hipStream_t s,
                            const uint32_t* dcount = nullptr, ListGrid grid = GRID_FULL);
// light sets (cgrt_render_light_sets*): set b's direct colour of entry i -> V.sets (k_shade_sets); K.nlights / K.nslights: the batch's
// distinct point positions and spherical keys
hipError_t launch_shade_sets(const LevelDev& V, const FrameConst& K, const SetsDev& T, unsigned long long n, hipStream_t s,
                             const uint32_t* dcount = nullptr, ListGrid grid = GRID_FULL);
// launch_fold / launch_write_rgb per set (n entries, V.nsets sets of colours V.stride entries apart); set b's frame starts at
// K.rgb + 3 * b * K.frame_pixels.  views (multi-view light sets, cgrt_render_views_light_sets*: k_write_rgb_views_sets): the pixels are
// a multi-view frame's (view * frame_pixels + in-view pixel), and set s's colour of a pixel of view v goes to frame v * nsets + s.
// GRID_STRIDED (one capped grid for every set): the scatter only with views
hipError_t launch_fold_sets(const LevelDev& V, unsigned long long n, hipStream_t s, const uint32_t* dcount = nullptr, ListGrid grid = GRID_FULL);
hipError_t launch_write_rgb_sets(const LevelDev& V0, const FrameConst& K, bool views, bool with_child, unsigned long long n, hipStream_t s,
                                 const uint32_t* dcount = nullptr, ListGrid grid = GRID_FULL);
// the anti-aliased frame (main.cpp:663-687) from the 2W x 2H sub-sample frame `sub` of F: see k_resolve_aa (shade_kernels.hip).
// out: F.nst_rank * 1024 * 3 floats (packed) or (F.W / 2) * (F.H / 2) * 3 floats
hipError_t launch_resolve_aa(const FrameDev& F, const float* sub, float* out, int packed, hipStream_t s);
// cgrt_render_device's export (k_export_frame, shade_kernels.hip): the W x H float frame `src` into the caller's buffer in one of the
// CGRT_FRAME_* formats of include/cgrt.h.  tile = 0: every pixel is written; otherwise only pixels whose tile x tile block index
// (row-major, tiles_x per row) % nranks == rank.  packed (tile 32 only): src holds this rank's blocks back to back, as k_resolve_aa
// writes them with packed = 1 (block slot k / nranks, 1024 pixels each).  dst is 4-byte aligned, pitch a multiple of 4.
// views > 1 (multi-view frames, tile = 0): src holds `views` W x H frames back to back, view v goes to dst + v * view_bytes -- one launch
// (an instantiation of its own; the single frame's kernel is the one it was).
struct ExportDev {
    const float* src;
    unsigned char* dst;
    unsigned long long pitch;  // bytes from one row of dst to the next (CHW: plane stride pitch * H)
    int W, H, format;
    int tile, tiles_x, rank, nranks, packed;
    int views;                      // 0 or 1: one frame
    unsigned long long view_bytes;  // dst bytes from one view to the next
};
hipError_t launch_export_frame(const ExportDev& E, hipStream_t s);
// Geometry buffers of a frame (cgrt_render_aov_device, include/cgrt.h CgrtAovOut): what the frame's primary rays
// saw, from level 0 of its own wavefront.  Every plane is packed and row-major, pixel p of view v at v * W * H + p (3-channel planes: 3
// floats there, or with chw plane c of view v at (3 v + c) * W * H); a NULL plane is not wanted and costs no traffic.
struct AovDev {
    float* depth;
    float* normal;
    float* position;
    float* albedo;
    uint32_t* prim_id;
    int32_t* material_id;
    uint8_t* mask;
    int chw;
    int W, H, views;                   // the traced frame (aa: the sub-sample frame); views >= 1
    int tiles_x, rank, nranks;         // nranks > 1: only pixels whose 64 x 64 super-tile (row-major, tiles_x per row) % nranks == rank
};
// launch_aov_fill (k_aov_fill): the miss values into every owned pixel of every requested plane, in row order.  launch_aov_scatter
// (k_aov_scatter), behind it on the same stream: entry i < n of level 0 {rays, hits, normals, item_pixels} and its material's kd to pixel
// item_pixels[i]; position = origin + direction * t in cgrt_math.h's arithmetic.
hipError_t launch_aov_fill(const AovDev& A, hipStream_t s);
hipError_t launch_aov_scatter(const AovDev& A, const LevelDev& V0, const float* materials, unsigned long long n, hipStream_t s,
                              const uint32_t* dcount = nullptr, ListGrid grid = GRID_FULL);
hipError_t launch_gather_calib(const void* table, unsigned long long nrecords, unsigned long long mult, unsigned long long add, float* sink,
                               hipStream_t s);
hipError_t launch_fastdiv_check(const float* a, const float* d, unsigned long long n, unsigned long long* mismatches, float* first_bad,
                                hipStream_t s);
hipError_t launch_ray_triangle(const float* tri, const float* rays, unsigned long long n, float* t_out, uint8_t* hit, float* normals,
                               hipStream_t s);
hipError_t launch_ray_plane(const float* plane, const float* rays, unsigned long long n, float* t_out, uint8_t* hit, hipStream_t s);
hipError_t launch_ray_box(const float* box, const float* rays, unsigned long long n, float* t_out, uint8_t* hit, uint8_t* inside,
                          hipStream_t s);
hipError_t launch_ray_sphere(const float* sph, const float* rays, unsigned long long n, float* t_out, uint8_t* hit, float* normals,
                             hipStream_t s);
hipError_t launch_triangle_plane(const float* tri, unsigned long long n, float* plane, hipStream_t s);
hipError_t launch_point_in_triangle(const float* in, unsigned long long n, uint8_t* out, hipStream_t s);

}  // namespace cgrt
