// crossing_kernels.h -- host-callable launchers of the crossing kernels in crossing_kernels.hip (include/cgrt.h cgrt_count_crossings*,
// cgrt_list_crossings*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgrt_layout.h"

namespace cgrt {

// include/cgrt.h CgrtCrossing, as the device writes it (two dwords; the caller's buffer is only 4-byte aligned)
struct CgrtCrossingDev {
    float t;
    uint32_t prim_id;
};
static_assert(sizeof(CgrtCrossingDev) == 8, "CgrtCrossingDev must be 8 B");

// One call's buffers, all device memory.  rays: n x 7 f32 (n <= 0x7fffffff).  out == nullptr: count mode, only counts is written.
// Otherwise ray i owns records [offsets[i], offsets[i + 1]) of out (offsets != nullptr, n + 1 entries, read by the kernel alone: a
// decreasing pair is an empty slot and both ends are clamped to capacity) or [i * k, (i + 1) * k) (the caller has checked
// n * k <= capacity); counts may then be nullptr.
struct CrossingArgs {
    const float* rays;
    uint64_t n;
    const unsigned long long* offsets;
    uint32_t k;
    CgrtCrossingDev* out;
    uint64_t capacity;
    uint32_t* counts;
};

// launch_crossings: the tree search (brute: every TriRecord in turn for every ray).  counters (optional, count mode only: two u64 {node
// steps, triangles evaluated}, zeroed by the caller) selects the counting instantiation.
hipError_t launch_crossings(const SceneDev& S, const CrossingArgs& A, bool brute, unsigned long long* counters, hipStream_t stream);

}  // namespace cgrt
