// point_frame_kernels.h -- host-callable launcher of the point-set frame kernel in point_frame_kernels.hip (include/cgrt.h
// cgrt_point_frames*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "point_neighbor_kernels.h"

namespace cgrt {

// include/cgrt.h CgrtPointFrame, as the device writes it: four 16-byte rows
struct CgrtPointFrameDev {
    float4 row[4];  // {centroid, used bits} {normal, lambda0} {tangent_u, lambda1} {tangent_v, lambda2}
};
static_assert(sizeof(CgrtPointFrameDev) == 64, "CgrtPointFrameDev must be 64 B");

// One call's buffers, all device memory.  points: n x 3 f32 (n <= 0x7fffffff); query i is bounded by radius2[i], or by max_dist2 where
// radius2 == nullptr.  data: the m x 3 f32 the grid was built on (the frames read coordinates by index; an index >= m, which only a
// grid of other data can hold, gives a record of zero bytes).  grid, grid_bytes as PointNeighborArgs; brute: only data and m.
// neighbors: n * k records, frames: n records (16-byte aligned); orient: nullptr or n x 3 f32.
struct PointFrameArgs {
    const void* grid;
    uint64_t grid_bytes;
    const float* data;
    uint64_t m;
    const float* points;
    const float* radius2;
    float max_dist2;
    uint32_t flags;
    uint64_t n;
    uint32_t k;
    const float* orient;
    CgrtPointNeighborDev* neighbors;
    CgrtPointFrameDev* frames;
};
hipError_t launch_point_frames(const PointFrameArgs& A, bool brute, hipStream_t stream);

}  // namespace cgrt
