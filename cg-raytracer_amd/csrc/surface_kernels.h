// surface_kernels.h -- host-callable launcher of the surface-attribute kernels in surface_kernels.hip (include/cgrt.h
// cgrt_hit_barycentrics*, cgrt_interpolate_hits*, cgrt_surface_*_device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgrt_layout.h"
#include "trace_kernels.h"

namespace cgrt {

// Per prim_id < ntris: where the triangle's TriRecord lives and which rows of a per-vertex table belong to its three vertices.  Built by
// capi_queries.cpp on the first surface call of a scene (16 bytes per triangle), never by a scene that makes none.
struct SurfaceLookup {
    uint32_t record;  // index into SceneDev::tris (the global record array)
    uint32_t v[3];    // tri[prim_id][0..2] as given to cgrt_scene_create
};
static_assert(sizeof(SurfaceLookup) == 16, "SurfaceLookup must be one 16-byte load");

enum SurfaceSource { SURFACE_LIST = 0, SURFACE_TRACKBALL = 1, SURFACE_RAYCAM = 2 };

// One launch: n items, item i either entry i of a ray list {rays, hits} or pixel i of `views` W x H frames (view = i / (W * H), the ray
// regenerated from cams[view], t = depth[i], prim_id = prim[i]).
struct SurfaceDev {
    const TriRecord* tris;        // SceneDev::tris
    const SurfaceLookup* lookup;  // ntris entries
    uint32_t ntris;
    uint32_t n;                   // items (<= 0x7fffffff)
    // ray list
    const float* rays;            // n x 7
    const CgrtHitDev* hits;       // n
    // frames
    const void* cams;             // CameraDev or RayCameraDev per view (device memory)
    const float* depth;
    const uint32_t* prim;
    int W, H;
    uint32_t plane;               // W * H
    // outputs
    const float* attr;            // nverts x channels, or NULL
    uint32_t channels;
    float* bary;                  // n x 3 (frames with chw: (views, 3, H, W)), or NULL
    float* out;                   // n x channels (frames with chw: (views, channels, H, W)), or NULL
    int chw;
    int vec4;                     // channels % 4 == 0 and attr, out 16-byte aligned: channel groups move as 16-byte loads and stores
};
hipError_t launch_surface(const SurfaceDev& A, int source, hipStream_t stream);

// One launch of the adjoint: the same n items, grad_out in the layout of SurfaceDev::out, every valid item's
// three weighted copies of its grad_out row added into grad_attr.
struct SurfaceGradDev {
    const TriRecord* tris;
    const SurfaceLookup* lookup;
    uint32_t ntris;
    uint32_t n;
    // ray list
    const float* rays;
    const CgrtHitDev* hits;
    // frames
    const void* cams;
    const float* depth;
    const uint32_t* prim;
    int W, H;
    uint32_t plane;
    // the gradient
    const float* grad_out;        // n x channels (frames with chw: (views, channels, H, W))
    uint32_t channels;
    float* grad_attr;             // nverts x channels, accumulated into
    int chw;
    int by_item;                  // each lane walks the channels of its own item (always with chw); else lanes walk the wave's 64 x C run
    int combine;                  // by_item: sum consecutive lanes of one prim_id inside the wave, one lane of each run adds
};
// The mapping the library ships for (channels, chw): see surface_grad_policy in surface_kernels.hip and DESIGN.md section 5.23.
void surface_grad_policy(uint32_t channels, int chw, int* by_item, int* combine);
hipError_t launch_surface_grad(const SurfaceGradDev& A, int source, hipStream_t stream);

}  // namespace cgrt
