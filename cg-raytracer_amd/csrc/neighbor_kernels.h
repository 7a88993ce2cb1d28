// neighbor_kernels.h -- host-callable launcher of the neighbour kernels in neighbor_kernels.hip (include/cgrt.h cgrt_count_neighbors*,
// cgrt_list_neighbors*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgrt_layout.h"

namespace cgrt {

// include/cgrt.h CgrtNeighbor, as the device writes it (two dwords; the caller's buffer is only 4-byte aligned)
struct CgrtNeighborDev {
    float dist2;
    uint32_t prim_id;
};
static_assert(sizeof(CgrtNeighborDev) == 8, "CgrtNeighborDev must be 8 B");

// One call's buffers, all device memory.  points: n x 3 f32 (n <= 0x7fffffff).  Query i is bounded by radius2[i], or by max_dist2 where
// radius2 == nullptr.  out == nullptr: count mode, only counts is written.  Otherwise query i owns records [offsets[i], offsets[i + 1])
// of out (offsets != nullptr, n + 1 entries, read by the kernel alone: a decreasing pair is an empty slot and both ends are clamped to
// capacity) or [i * k, (i + 1) * k) (the caller has checked n * k <= capacity); counts may then be nullptr.
struct NeighborArgs {
    const float* points;
    const float* radius2;
    float max_dist2;
    uint64_t n;
    const unsigned long long* offsets;
    uint32_t k;
    CgrtNeighborDev* out;
    uint64_t capacity;
    uint32_t* counts;
};

// launch_neighbors: the tree search (brute: every TriRecord in turn for every query).  counters (optional, tree search only: two u64
// {node steps, triangles evaluated}, zeroed by the caller) selects the counting instantiation of the count search (out == nullptr) or
// of the list search.
hipError_t launch_neighbors(const SceneDev& S, const NeighborArgs& A, bool brute, unsigned long long* counters, hipStream_t stream);

}  // namespace cgrt
