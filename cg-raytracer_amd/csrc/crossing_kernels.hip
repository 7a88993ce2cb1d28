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

#include "closest_kernels.h"
#include "crossing_kernels.h"
#include "walk_exact.h"

namespace cgrt {

namespace {

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
                    const float4* q = reinterpret_cast<const float4*>(S.packets + (cur & ~CR_PACKET));
                    const float4 a = q[0], b = q[1], c = q[2];
                    const uint4 m = *reinterpret_cast<const uint4*>(q + 3);
                    float tn0, tf0, tn1, tf1;
                    slab_cons(P, P.sx ? a.w : a.x, P.sx ? a.x : a.w, P.sy ? b.x : a.y, P.sy ? a.y : b.x, P.sz ? b.y : a.z, P.sz ? a.z : b.y, tn0,
                              tf0);
                    slab_cons(P, P.sx ? c.y : b.z, P.sx ? b.z : c.y, P.sy ? c.z : b.w, P.sy ? b.w : c.z, P.sz ? c.w : c.x, P.sz ? c.x : c.w, tn1,
                              tf1);
                    const float tc = fmaxf(Q.bound, 0.0f);  // never below 0: an origin-on-plane acceptance ignores ray.t (sub_node_step)
                    const bool h0 = m.x != REF_NONE && (tn0 <= tf0) && (tf0 >= 0.0f) && (tn0 <= tc);
                    const bool h1 = m.y != REF_NONE && (tn1 <= tf1) && (tf1 >= 0.0f) && (tn1 <= tc);
                    const uint32_t r0 = cross_topo_ref(m.x), r1 = cross_topo_ref(m.y);  // (only used where the child was hit)
                    const bool second_first = h1 && (!h0 || tn1 < tn0);
                    if (h0 && h1) {  // the nearer child now: a full slot's bound shrinks sooner
                        stk[sp * CGRT_STRIDE] = second_first ? r0 : r1;
                        sp++;
                    }
                    cur = second_first ? r1 : (h0 ? r0 : REF_NONE);
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
