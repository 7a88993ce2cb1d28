// neighbor_kernels.hip -- neighbour queries (include/cgrt.h cgrt_count_neighbors*, cgrt_list_neighbors*): for
// every query point ALL the triangles within its squared radius, counted, or listed in (dist2, prim_id) order -- the point-side twin of
// the crossing queries.  dist2 is closest_device.h closest_eval, the very function k_closest takes its minimum over: a pure function of
// (p, triangle), so the search only has to reach every triangle that can qualify, in any order.
//
// k_neighbors: one query per lane, closest_device.h's closest_walk -- k_closest's walk, with its box lower bound, child ordering and LDS
// stack (two dwords per entry {ref, lb2}, lane-interleaved) -- with every run of records taken into the lane's slot (query_device.h
// QuerySlot, the slot of the crossing queries).  A subtree is skipped iff `lb2 > bound` is TRUE; bound = the query's r2, and while a slot
// is full and no count is asked for, the largest dist2 kept -- non-strictly, so an equal-dist2 smaller prim_id still arrives.
// lb2 <= dist2 holds in f32 with no slack for every triangle under a box (closest_kernels.hip), hence no neighbour that belongs in the
// slot is ever skipped.  A lane owns its slot of the output and keeps it sorted in global memory by insertion, dropping the largest
// when full: no atomics, no scratch.
// k_neighbors<.., BRUTE>: every record in turn for every query, same function, same slot rule (validation).
#include <hip/hip_runtime.h>

#include "closest_device.h"
#include "neighbor_kernels.h"

namespace cgrt {

namespace {

// include/cgrt.h "Neighbour queries": membership; a neighbour is taken into the slot under its dist2 (query_device.h slot_take)
template <bool LIST>
__device__ __forceinline__ void neighbor_apply(const float dist2, const uint32_t prim, QuerySlot& Q) {
    if (dist2 <= Q.limit) slot_take<LIST>(dist2, prim, Q);  // (a NaN never qualifies)
}

// records [first, first + cnt)
template <bool LIST>
__device__ __forceinline__ void neighbor_records(const SceneDev& S, const unsigned long long first, const uint32_t cnt, const float px,
                                                 const float py, const float pz, QuerySlot& Q) {
    const float4* q = reinterpret_cast<const float4*>(S.tris + first);
    for (unsigned long long r = 0; r < cnt; r++) {
        const TriClosest E = closest_eval(q[4 * r], q[4 * r + 1], q[4 * r + 2], q[4 * r + 3], px, py, pz);
        neighbor_apply<LIST>(E.dist2, E.prim, Q);
    }
}

template <bool LIST, bool COUNT, bool BRUTE>
__global__ __launch_bounds__(CGRT_CLOSEST_BLOCK) void k_neighbors(const SceneDev S, const float* __restrict__ points,
                                                                  const float* __restrict__ radius2, const float max_dist2, const uint32_t n,
                                                                  const unsigned long long* __restrict__ offsets, const uint32_t k,
                                                                  uint32_t* out, const unsigned long long capacity,
                                                                  uint32_t* __restrict__ counts, unsigned long long* __restrict__ counters) {
    // slot s of lane l of wave w at w * (2 * CLOSEST_STACK_ENTRIES * 64) + s * 64 + l; entry e = slots 2e {ref}, 2e + 1 {lb2}
    __shared__ uint32_t s_stk[BRUTE ? 1 : 2 * CLOSEST_STACK_ENTRIES * CGRT_CLOSEST_BLOCK];
    const unsigned long long i = (unsigned long long)blockIdx.x * CGRT_CLOSEST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    QuerySlot Q;
    const bool wanted = slot_open<LIST>(Q, radius2 ? radius2[i] : max_dist2, out, offsets, k, capacity, counts != nullptr, i);
    unsigned long long c_nodes = 0, c_tris = 0;
    // a radius that is NaN or below zero and a point that is not finite have no neighbours
    if (S.root_ref != REF_NONE && wanted && Q.limit >= 0.0f && finite3(px, py, pz)) {
        if (BRUTE) {
            if (COUNT) c_tris += S.ntris;
            neighbor_records<LIST>(S, S.tri_base, S.ntris, px, py, pz, Q);
        } else {
            uint32_t* const stk = s_stk + (threadIdx.x >> 6) * (2 * CLOSEST_STACK_ENTRIES * 64) + (threadIdx.x & 63u);
            closest_walk<COUNT>(
                S, px, py, pz, stk, [&](const uint32_t first, const uint32_t cnt) { neighbor_records<LIST>(S, first, cnt, px, py, pz, Q); },
                [&]() { return Q.bound; }, c_nodes, c_tris);
        }
    }
    slot_close<LIST>(Q, counts, i);
    if (COUNT) {
        atomicAdd(counters, c_nodes);
        atomicAdd(counters + 1, c_tris);
    }
}

template <bool LIST, bool COUNT, bool BRUTE>
hipError_t launch_one(const SceneDev& S, const NeighborArgs& A, unsigned long long* counters, hipStream_t stream) {
    const dim3 grid((unsigned)((A.n + CGRT_CLOSEST_BLOCK - 1) / CGRT_CLOSEST_BLOCK)), block(CGRT_CLOSEST_BLOCK);
    hipLaunchKernelGGL((k_neighbors<LIST, COUNT, BRUTE>), grid, block, 0, stream, S, A.points, A.radius2, A.max_dist2, (uint32_t)A.n, A.offsets,
                       A.k, reinterpret_cast<uint32_t*>(A.out), (unsigned long long)A.capacity, A.counts, counters);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_neighbors(const SceneDev& S, const NeighborArgs& A, bool brute, unsigned long long* counters, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    if (A.n > 0x7fffffffull || (!A.out && !A.counts) || (counters && brute)) return hipErrorInvalidValue;
    if (counters) return A.out ? launch_one<true, true, false>(S, A, counters, stream) : launch_one<false, true, false>(S, A, counters, stream);
    if (!A.out) return brute ? launch_one<false, false, true>(S, A, nullptr, stream) : launch_one<false, false, false>(S, A, nullptr, stream);
    return brute ? launch_one<true, false, true>(S, A, nullptr, stream) : launch_one<true, false, false>(S, A, nullptr, stream);
}

}  // namespace cgrt
