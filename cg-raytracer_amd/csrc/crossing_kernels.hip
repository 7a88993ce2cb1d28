// crossing_kernels.hip -- crossing queries (include/cgrt.h cgrt_count_crossings*, cgrt_list_crossings*): for every
// ray ALL the triangles intersectRayWithTriangle (ray_tracing.cpp:86-114) accepts on a fresh copy of the ray, counted, or listed in
// (t, prim_id) order.  A crossing is a pure function of (ray, triangle) -- TriEval of walk_exact.h, unchanged -- so the search only has to
// reach every acceptable triangle, in any order:
//
// k_crossings: one ray per lane, crossing_device.h's cross_walk over the structure every scene has, as closest_walk visits it -- the
// reference tree's NodePackets, then the leaves' 4-wide accelerators down to runs of records, or plain LeafRec ranges where a leaf has
// no accelerator.  Boxes are tested with the conservative test alone (walk_exact.h make_raypre / slab_cons / sub_node_step: no box that holds a point the triangle arithmetic
// could accept is rejected), bounded by the ray's own t; while a slot is full the bound shrinks to the largest t kept, non-strictly, so
// an equal-t smaller prim_id still arrives.  A ray outside that test's envelope (RayPre::regular false) scans every record itself.
// The per-lane stack is lane-interleaved in LDS, one dword per entry.  A lane owns its slot of the output and keeps it sorted in global
// memory by insertion, dropping the largest when full: no atomics, no scratch (query_device.h QuerySlot).
// k_crossings<.., BRUTE>: every record in turn for every ray, same function, same slot rule (validation, and the whole call on scenes
// where the conservative argument does not hold: capi_queries.cpp crossing_brute_scene).
#include <hip/hip_runtime.h>

#include "crossing_device.h"

namespace cgrt {

namespace {

template <bool LIST, bool COUNT, bool BRUTE>
__global__ __launch_bounds__(CGRT_CROSS_BLOCK) void k_crossings(const SceneDev S, const float* __restrict__ rays, const uint32_t n,
                                                                const unsigned long long* __restrict__ offsets, const uint32_t k, uint32_t* out,
                                                                const unsigned long long capacity, uint32_t* __restrict__ counts,
                                                                unsigned long long* __restrict__ counters) {
    // entry e of lane l of wave w at w * (CLOSEST_STACK_ENTRIES * 64) + e * 64 + l
    __shared__ uint32_t s_stk[BRUTE ? 1 : CLOSEST_STACK_ENTRIES * CGRT_CROSS_BLOCK];
    const unsigned long long i = (unsigned long long)blockIdx.x * CGRT_CROSS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const F3 o = f3(rays[7 * i], rays[7 * i + 1], rays[7 * i + 2]), d = f3(rays[7 * i + 3], rays[7 * i + 4], rays[7 * i + 5]);
    uint32_t* const stk = s_stk + (threadIdx.x >> 6) * (CLOSEST_STACK_ENTRIES * 64) + (threadIdx.x & 63u);
    QuerySlot Q;
    const bool wanted = slot_open<LIST>(Q, rays[7 * i + 6], out, offsets, k, capacity, counts != nullptr, i);
    unsigned long long c_nodes = 0, c_tris = 0;
    if (S.root_ref != REF_NONE && wanted) {
        if (BRUTE) {  // cross_walk's own scan, written out: through the call these kernels take two more VGPRs and lose a wave per SIMD
            if (COUNT) c_tris += S.ntris;
            for (uint32_t r = 0; r < S.ntris; r += SUB_RUN_MAX)
                cross_records<LIST>(S, (unsigned long long)S.tri_base + r, min(SUB_RUN_MAX, S.ntris - r), o, d, Q);
        } else {
            cross_walk<LIST, COUNT, false>(S, o, d, stk, Q, c_nodes, c_tris);
        }
    }
    slot_close<LIST>(Q, counts, i);
    if (COUNT) {
        atomicAdd(counters, c_nodes);
        atomicAdd(counters + 1, c_tris);
    }
}

template <bool LIST, bool COUNT, bool BRUTE>
hipError_t launch_one(const SceneDev& S, const CrossingArgs& A, unsigned long long* counters, hipStream_t stream) {
    const dim3 grid((unsigned)((A.n + CGRT_CROSS_BLOCK - 1) / CGRT_CROSS_BLOCK)), block(CGRT_CROSS_BLOCK);
    hipLaunchKernelGGL((k_crossings<LIST, COUNT, BRUTE>), grid, block, 0, stream, S, A.rays, (uint32_t)A.n, A.offsets, A.k,
                       reinterpret_cast<uint32_t*>(A.out), (unsigned long long)A.capacity, A.counts, counters);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_crossings(const SceneDev& S, const CrossingArgs& A, bool brute, unsigned long long* counters, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    if (A.n > 0x7fffffffull || (!A.out && !A.counts) || (counters && A.out)) return hipErrorInvalidValue;
    if (counters) return brute ? launch_one<false, true, true>(S, A, counters, stream) : launch_one<false, true, false>(S, A, counters, stream);
    if (!A.out) return brute ? launch_one<false, false, true>(S, A, nullptr, stream) : launch_one<false, false, false>(S, A, nullptr, stream);
    return brute ? launch_one<true, false, true>(S, A, nullptr, stream) : launch_one<true, false, false>(S, A, nullptr, stream);
}

}  // namespace cgrt
