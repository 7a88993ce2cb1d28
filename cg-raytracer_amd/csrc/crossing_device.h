// crossing_device.h -- the device functions of the crossing search (include/cgrt.h "Crossing queries"): the
// definition on a TriEval, the evaluation of a run of records, the search stack's encoding, the NodePacket step and the walk itself
// (cross_walk).  crossing_kernels.hip (k_crossings) and sdf_kernels.hip (the parity walks of k_sdf) call these very functions, so both
// accept the same triangles for a ray.
#pragma once
#include <hip/hip_runtime.h>

#include "closest_kernels.h"
#include "crossing_kernels.h"
#include "query_device.h"
#include "walk_exact.h"

namespace cgrt {

#define CGRT_CROSS_BLOCK 128

// The stack's own encoding of a deferred subtree (sub_node_step pushes the first two kinds as the accelerator stores them):
//   bit 31 set             a run of records: REF_LEAF | (count - 1) << 26 | first record
//   index                  an accelerator node (two consecutive SubNodes)
//   CR_PACKET | index      a NodePacket
//   CR_LEAF | index        a reference leaf without accelerator: LeafRec{first, count}
const uint32_t CR_PACKET = 0x40000000u;
const uint32_t CR_LEAF = 0x20000000u;
static_assert(SUB_MAX_RECORDS <= CR_LEAF, "record indices must stay below the kind bits");
// Accelerator nodes and runs only exist where every record index is below SUB_MAX_RECORDS (bvh_builder.cpp drops the accelerators beyond
// it); NodePackets and leaves are those of a reference tree of at most MAX_LEVELS levels: fewer than 2^MAX_LEVELS of each.
static_assert((1u << MAX_LEVELS) <= CR_LEAF, "NodePacket and leaf-table indices must stay below the kind bits");
static_assert(CGRT_STRIDE == 64, "sub_node_step addresses the lane-interleaved stack of one wave");
static_assert(CLOSEST_STACK_ENTRIES * CGRT_CROSS_BLOCK * 4 <= 65536, "the stacks of a workgroup must fit its LDS");

__device__ __forceinline__ uint32_t cross_topo_ref(const uint32_t r) {  // a child reference of a NodePacket (or the root), not REF_NONE
    if (!(r & REF_LEAF)) return CR_PACKET | r;
    return (r & REF_LEAF_ACCEL) ? (r & REF_INDEX26) : (CR_LEAF | (r & ~REF_LEAF));
}

// include/cgrt.h "Crossing queries": the definition on a TriEval; a crossing is taken into the slot under its t (query_device.h slot_take)
template <bool LIST>
__device__ __forceinline__ void cross_apply(const TriEval& E, const uint32_t prim, QuerySlot& Q) {
    const bool ok = E.inside && (E.onp || (E.den_ok && !(E.tt < 0) && !(E.tt >= Q.limit)));
    if (ok) slot_take<LIST>(E.tt, prim, Q);
}

// records [first, first + n): the first two on the packed pipe when that is the whole run, as the walks evaluate runs
template <bool LIST>
__device__ __forceinline__ void cross_records(const SceneDev& S, const unsigned long long first, const uint32_t n, const F3 o, const F3 d,
                                              QuerySlot& Q) {
    const float4* q = reinterpret_cast<const float4*>(S.tris + first);
    if (n <= 2u) {
        const uint32_t j = (n > 1u) ? 4u : 0u;
        const float4 a0 = q[0], b0 = q[1], c0 = q[2], e0 = q[3];
        const float4 a1 = q[j], b1 = q[j + 1], c1 = q[j + 2], e1 = q[j + 3];
        TriEval E0, E1;
        eval_pair(a0, b0, c0, e0, a1, b1, c1, e1, o, d, E0, E1);
        cross_apply<LIST>(E0, __float_as_uint(e0.y), Q);
        if (n > 1u) cross_apply<LIST>(E1, __float_as_uint(e1.y), Q);
    } else {
        for (unsigned long long i = 0; i < n; i++) {
            const float4 e = q[4 * i + 3];
            cross_apply<LIST>(eval_record(q[4 * i], q[4 * i + 1], q[4 * i + 2], e, o, d), __float_as_uint(e.y), Q);
        }
    }
}

// One step through a NodePacket (two child boxes {lo.xyz, hi.xyz}) under the conservative test, bounded by `bound`: the nearer hit child
// becomes cur (a full slot's bound shrinks sooner), the other hit child is deferred; REF_NONE when neither is hit.
__device__ __forceinline__ void cross_packet_step(const SceneDev& S, const RayPre& P, const float bound, uint32_t& cur, int& sp,
                                                  uint32_t* __restrict__ stk) {
    const float4* q = reinterpret_cast<const float4*>(S.packets + (cur & ~CR_PACKET));
    const float4 a = q[0], b = q[1], c = q[2];
    const uint4 m = *reinterpret_cast<const uint4*>(q + 3);
    float tn0, tf0, tn1, tf1;
    slab_cons(P, P.sx ? a.w : a.x, P.sx ? a.x : a.w, P.sy ? b.x : a.y, P.sy ? a.y : b.x, P.sz ? b.y : a.z, P.sz ? a.z : b.y, tn0, tf0);
    slab_cons(P, P.sx ? c.y : b.z, P.sx ? b.z : c.y, P.sy ? c.z : b.w, P.sy ? b.w : c.z, P.sz ? c.w : c.x, P.sz ? c.x : c.w, tn1, tf1);
    const float tc = fmaxf(bound, 0.0f);  // never below 0: an origin-on-plane acceptance ignores ray.t (sub_node_step)
    const bool h0 = m.x != REF_NONE && (tn0 <= tf0) && (tf0 >= 0.0f) && (tn0 <= tc);
    const bool h1 = m.y != REF_NONE && (tn1 <= tf1) && (tf1 >= 0.0f) && (tn1 <= tc);
    const uint32_t r0 = cross_topo_ref(m.x), r1 = cross_topo_ref(m.y);  // (only used where the child was hit)
    const bool second_first = h1 && (!h0 || tn1 < tn0);
    if (h0 && h1) {
        stk[sp * CGRT_STRIDE] = second_first ? r0 : r1;
        sp++;
    }
    cur = second_first ? r1 : (h0 ? r0 : REF_NONE);
}

// The search of one ray {o, d, Q.limit}, from the root (S.root_ref != REF_NONE): every triangle the definition can accept reaches
// cross_apply, in any order.  The structure is the one closest_walk visits; boxes are tested with the conservative test alone, bounded by
// Q.bound.  BRUTE, and a ray outside that test's envelope (RayPre::regular false), scan every record instead.  stk: the lane's column of
// a lane-interleaved LDS region, entry e at stk[e * 64], CLOSEST_STACK_ENTRIES entries (not touched under BRUTE).
template <bool LIST, bool COUNT, bool BRUTE>
__device__ __forceinline__ void cross_walk(const SceneDev& S, const F3 o, const F3 d, uint32_t* const stk, QuerySlot& Q,
                                           unsigned long long& c_nodes, unsigned long long& c_tris) {
    const RayPre P = make_raypre(S, o, d, Q.limit);
    if (BRUTE || !P.regular) {
        if (COUNT) c_tris += S.ntris;
        for (uint32_t r = 0; r < S.ntris; r += SUB_RUN_MAX)
            cross_records<LIST>(S, (unsigned long long)S.tri_base + r, min(SUB_RUN_MAX, S.ntris - r), o, d, Q);
        return;
    }
    LaneCounters cnt;
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
    if (COUNT) c_nodes += cnt.sub;
}

}  // namespace cgrt
