// closest_kernels.h -- host-callable launchers of the closest-point kernels in closest_kernels.hip (include/cgrt.h cgrt_closest_points*;
// DESIGN.md section 5.20).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgrt_layout.h"

namespace cgrt {

// include/cgrt.h CgrtClosest, as the device writes it
struct CgrtClosestDev {
    float point[3];
    float dist2;
    uint32_t prim_id;
    float bary[3];
};
static_assert(sizeof(CgrtClosestDev) == 32, "CgrtClosestDev must be 32 B");

// Deferred subtrees of one query: a NodePacket step defers at most one child, a step through a 4-wide accelerator node at most three.
static const int CLOSEST_STACK_ENTRIES = (MAX_LEVELS - 1) + (SUB_WIDTH - 1) * SUB_MAX_DEPTH;

// n queries (points: n x 3 f32, out: n records; device memory, n <= 0x7fffffff) on `stream`.
// launch_closest: the tree search; counters (optional, two u64 {node steps, triangles evaluated}, zeroed by the caller) selects the
// counting instantiation.  launch_closest_brute: every TriRecord in turn.
hipError_t launch_closest(const SceneDev& S, const float* points, uint64_t n, float max_dist2, CgrtClosestDev* out, unsigned long long* counters,
                          hipStream_t stream);
hipError_t launch_closest_brute(const SceneDev& S, const float* points, uint64_t n, float max_dist2, CgrtClosestDev* out, hipStream_t stream);

}  // namespace cgrt
