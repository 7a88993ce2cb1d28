// crossing_device.h -- the device functions of the crossing search (include/cgrt.h "Crossing queries"): the
// definition on a TriEval with the slot rule, the evaluation of a run of records, the search stack's encoding and the NodePacket step.
// crossing_kernels.hip (k_crossings) and sdf_kernels.hip (the parity walks of k_sdf) call these very functions, so both accept the same
// triangles for a ray.
#pragma once
#include <hip/hip_runtime.h>

#include "closest_kernels.h"
#include "crossing_kernels.h"
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

// A lane's slot and its running state.
struct CrossSlot {
    uint32_t* rec;           // the slot's first record, two dwords per record {t, prim_id}
    unsigned long long len;  // records the slot holds
    uint32_t room;           // min(len, 2^32 - 1): a ray has fewer crossings than that
    uint32_t kept;           // records rec[0 .. kept) are the smallest `kept` crossings so far, in order
    uint32_t count;          // all crossings so far
    float t_in;              // the ray's own t: what a crossing is tested against
    float bound;             // what boxes are tested against: t_in, or the largest t kept once the slot is full (shrink)
    bool shrink;
};

__device__ __forceinline__ bool cross_before(const float ta, const uint32_t pa, const float tb, const uint32_t pb) {
    return ta < tb || (ta == tb && pa < pb);
}

// include/cgrt.h "Crossing queries": the definition on a TriEval, then the slot rule
template <bool LIST>
__device__ __forceinline__ void cross_apply(const TriEval& E, const uint32_t prim, CrossSlot& Q) {
    const bool ok = E.inside && (E.onp || (E.den_ok && !(E.tt < 0) && !(E.tt >= Q.t_in)));
    if (!ok) return;
    Q.count++;
    if (!LIST || Q.room == 0u) return;
    size_t j = Q.kept;
    if (Q.kept == Q.room) {  // full: the largest one leaves, unless that is the new one
        if (!cross_before(E.tt, prim, __uint_as_float(Q.rec[2 * (j - 1)]), Q.rec[2 * (j - 1) + 1])) return;
        j--;
    } else {
        Q.kept++;
    }
    while (j > 0) {
        const uint32_t pt = Q.rec[2 * (j - 1)], pp = Q.rec[2 * (j - 1) + 1];
        if (!cross_before(E.tt, prim, __uint_as_float(pt), pp)) break;
        Q.rec[2 * j] = pt;
        Q.rec[2 * j + 1] = pp;
        j--;
    }
    Q.rec[2 * j] = __float_as_uint(E.tt);
    Q.rec[2 * j + 1] = prim;
    if (Q.shrink && Q.kept == Q.room) Q.bound = __uint_as_float(Q.rec[2 * (size_t)(Q.room - 1u)]);
}

// records [first, first + n): the first two on the packed pipe when that is the whole run, as the walks evaluate runs
template <bool LIST>
__device__ __forceinline__ void cross_records(const SceneDev& S, const unsigned long long first, const uint32_t n, const F3 o, const F3 d,
                                              CrossSlot& Q) {
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

}  // namespace cgrt
