// winding_kernels.h -- host-callable launcher of the winding-number kernel in winding_kernels.hip (include/cgrt.h
// cgrt_winding_numbers*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "winding_builder.h"

namespace cgrt {

// How a lane finds its point.
enum WindingPoints {
    WINDING_LIST = 0,        // point i of `points`
    WINDING_GRID_BRICK = 1,  // grid point of a 4 x 4 x 4 brick per wave, two bricks next to each other in x per block (as sdf_kernels.hip)
};

// One call, passed to the kernel by value: no host array is read behind the launch.  points: n x 3 f32 (WINDING_LIST), or the grid (n =
// nx * ny * nz); all pointers device memory, n <= 0x7fffffff.  recs: the scene's TriRecords in record order (SceneDev::tris + tri_base),
// ntris <= 2^26 of them; clusters: the tree of winding_builder.h over them (nlevels levels, the top one starting at cluster top_base;
// unused by the brute form, nullptr with ntris == 0).  beta2 = beta * beta, rounded once on the host.  w and inside (either may be
// nullptr) are what is stored.
struct WindingArgs {
    const float* points;
    uint32_t n;
    float origin[3], spacing[3];
    uint32_t dims[3];  // nx, ny, nz
    const TriRecord* recs;
    uint32_t ntris;
    const WindingCluster* clusters;
    uint32_t nlevels, top_base;
    float beta2, threshold;
    float* w;
    uint8_t* inside;
};

// brute: every record in record order, no cluster is read.  counters (optional, WINDING_LIST and the tree form only: three u64 {clusters
// tested, dipoles taken, triangles evaluated}, zeroed by the caller) selects the counting instantiation.
hipError_t launch_winding(const WindingArgs& A, WindingPoints how, bool brute, unsigned long long* counters, hipStream_t stream);

}  // namespace cgrt
