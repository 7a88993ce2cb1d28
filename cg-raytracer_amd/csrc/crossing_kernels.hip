// crossing_kernels.hip -- crossing queries (include/cgrt.h cgrt_count_crossings*, cgrt_list_crossings*): for every
// ray ALL the triangles intersectRayWithTriangle (ray_tracing.cpp:86-114) accepts on a fresh copy of the ray, counted, or listed in
// (t, prim_id) order.  A crossing is a pure function of (ray, triangle) -- TriEval of walk_exact.h, unchanged -- so the search only has to
// reach every acceptable triangle, in any order:
//
// k_crossings: one ray per lane over the structure every scene has, as k_closest walks it -- the reference tree's NodePackets, then the
// leaves' 4-wide accelerators down to runs of records, or plain LeafRec ranges where a leaf has no accelerator.  Boxes are tested with
// the conservative test alone (walk_exact.h make_raypre / slab_cons / sub_node_step: no box that holds a point the triangle arithmetic
// could accept is rejected), bounded by the ray's own t; while a slot is full the bound shrinks to the largest t kept, non-strictly, so
// an equal-t smaller prim_id still arrives.  A ray outside that test's envelope (RayPre::regular false) scans every record itself.
// The per-lane stack is lane-interleaved in LDS, one dword per entry.  A lane owns its slot of the output and keeps it sorted in global
// memory by insertion, dropping the largest when full: no atomics, no scratch.
// k_crossings<.., BRUTE>: every record in turn for every ray, same function, same slot rule (validation, and the whole call on scenes
// where the conservative argument does not hold: capi.cpp crossing_brute_scene).
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
    CrossSlot Q;
    Q.t_in = rays[7 * i + 6];
    Q.bound = Q.t_in;
    Q.kept = 0u;
    Q.count = 0u;
    Q.rec = out;
    Q.len = 0ull;
    Q.shrink = LIST && counts == nullptr;  // the full count needs every crossing, whatever the slot holds
    if (LIST) {
        unsigned long long b, e;
        if (offsets) {
            b = offsets[i];
            e = offsets[i + 1];
            if (e < b) e = b;  // a decreasing pair: an empty slot
        } else {
            b = i * k;
            e = b + k;
        }
        b = b < capacity ? b : capacity;
        e = e < capacity ? e : capacity;
        Q.rec = out + 2 * b;
        Q.len = e - b;
    }
    Q.room = Q.len < 0xffffffffull ? (uint32_t)Q.len : 0xffffffffu;
    LaneCounters cnt;
    unsigned long long c_nodes = 0, c_tris = 0;
    const bool wanted = !LIST || counts != nullptr || Q.room != 0u;  // (an empty slot without a count asks for nothing)
    if (S.root_ref != REF_NONE && wanted) {
        const RayPre P = make_raypre(S, o, d, Q.t_in);
        if (BRUTE || !P.regular) {
            if (COUNT) c_tris += S.ntris;
            for (uint32_t r = 0; r < S.ntris; r += SUB_RUN_MAX)
                cross_records<LIST>(S, (unsigned long long)S.tri_base + r, min(SUB_RUN_MAX, S.ntris - r), o, d, Q);
        } else {
            uint32_t* const stk = s_stk + (threadIdx.x >> 6) * (CLOSEST_STACK_ENTRIES * 64) + (threadIdx.x & 63u);
            uint32_t cur = cross_topo_ref(S.root_ref);
            int sp = 0;
            for (;;) {
                if (cur == REF_NONE) {
                    if (sp == 0) break;
                    sp--;
                    cur = stk[sp * CGRT_STRIDE];
                }
                if (cur & REF_LEAF) {  // a run of 1..32 records
                    if (COUNT) c_tris += run_count(cur);
                    cross_records<LIST>(S, run_first(cur), run_count(cur), o, d, Q);
                    cur = REF_NONE;
                } else if (cur & CR_LEAF) {  // a reference leaf scanned linearly
                    const LeafRec L = S.leaves[cur & ~CR_LEAF];
                    if (COUNT) c_tris += L.count;
                    for (uint32_t r = 0; r < L.count; r += SUB_RUN_MAX)
                        cross_records<LIST>(S, (unsigned long long)L.first + r, min(SUB_RUN_MAX, L.count - r), o, d, Q);
                    cur = REF_NONE;
                } else if (cur & CR_PACKET) {  // NodePacket: two child boxes {lo.xyz, hi.xyz}
                    if (COUNT) c_nodes++;
                    cross_packet_step(S, P, Q.bound, cur, sp, stk);
                } else {  // an accelerator node: the nearest hit child becomes cur, the others are deferred
                    sub_node_step<COUNT>(S, P, Q.bound, cur, sp, stk, cnt);
                }
            }
        }
    }
    if (LIST) {
        for (unsigned long long j = Q.kept; j < Q.len; j++) {  // the rest of the slot: {+inf, CGRT_NO_PRIM}
            Q.rec[2 * j] = 0x7f800000u;
            Q.rec[2 * j + 1] = 0xffffffffu;
        }
    }
    if (counts) counts[i] = Q.count;
    if (COUNT) {
        atomicAdd(counters, c_nodes + cnt.sub);
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
