// sdf_kernels.h -- host-callable launcher of the signed-distance / occupancy kernel in sdf_kernels.hip (include/cgrt.h
// cgrt_signed_distance*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgrt_layout.h"

namespace cgrt {

// How a lane finds its point.
enum SdfPoints {
    SDF_LIST = 0,         // point i of `points`
    SDF_GRID_BRICK = 1,   // grid point of a 4 x 4 x 4 brick per wave, two bricks next to each other in x per block
    SDF_GRID_LINEAR = 2,  // grid point of result index block * 128 + lane
};

// One call, passed to the kernel by value: no host array is read behind the launch.  points: n x 3 f32 (SDF_LIST), or the grid (n =
// nx * ny * nz); all pointers device memory, n <= 0x7fffffff.  dirs[0 .. ndirs) (ndirs odd, 1..7) are the parity directions.  The
// closest-point search runs iff want_sdf; sdf and inside (either may be nullptr) are what is stored.
struct SdfArgs {
    const float* points;
    uint32_t n;
    float origin[3], spacing[3];
    uint32_t dims[3];  // nx, ny, nz
    float max_dist2;
    uint32_t ndirs;
    float dirs[7][3];
    uint32_t want_sdf;
    float* sdf;
    uint8_t* inside;
};

// brute_parity: the parity walks test every triangle (scenes where the conservative box argument does not hold).  counters (optional,
// SDF_LIST only: five u64 {closest node steps, closest triangles, crossing node steps, crossing triangles, direction walks}, zeroed by the
// caller) selects the counting instantiation.
hipError_t launch_sdf(const SceneDev& S, const SdfArgs& A, SdfPoints how, bool brute_parity, unsigned long long* counters, hipStream_t stream);

}  // namespace cgrt
