// neighbor_kernels.hip -- neighbour queries (include/cgrt.h cgrt_count_neighbors*, cgrt_list_neighbors*): for
// every query point ALL the triangles within its squared radius, counted, or listed in (dist2, prim_id) order -- the point-side twin of
// the crossing queries.  dist2 is closest_device.h closest_eval, the very function k_closest takes its minimum over: a pure function of
// (p, triangle), so the search only has to reach every triangle that can qualify, in any order.
//
// k_neighbors: one query per lane over the structure k_closest walks, with its box lower bound, child ordering and LDS stack (two
// dwords per entry {ref, lb2}, lane-interleaved).  A subtree is skipped iff `lb2 > bound` is TRUE; bound = the query's r2, and while
// a slot is full and no count is asked for, the largest dist2 kept -- non-strictly, so an equal-dist2 smaller prim_id still arrives.
// lb2 <= dist2 holds in f32 with no slack for every triangle under a box (closest_kernels.hip), hence no neighbour that belongs in the
// slot is ever skipped.  A lane owns its slot of the output and keeps it sorted in global memory by insertion, dropping the largest
// when full: no atomics, no scratch (crossing_device.h cross_apply's rule).
// k_neighbors<.., BRUTE>: every record in turn for every query, same function, same slot rule (validation).
#include <hip/hip_runtime.h>

#include "closest_device.h"
#include "neighbor_kernels.h"

namespace cgrt {

namespace {

// A lane's slot and its running state.
struct NeighborSlot {
    uint32_t* rec;           // the slot's first record, two dwords per record {dist2, prim_id}
    unsigned long long len;  // records the slot holds
    uint32_t room;           // min(len, 2^32 - 1): a query has fewer neighbours than that
    uint32_t kept;           // records rec[0 .. kept) are the smallest `kept` neighbours so far, in order
    uint32_t count;          // all neighbours so far
    float r2;                // the query's own bound: what a dist2 is tested against
    float bound;             // what boxes are tested against: r2, or the largest dist2 kept once the slot is full (shrink)
    bool shrink;
};

__device__ __forceinline__ bool neighbor_before(const float da, const uint32_t pa, const float db, const uint32_t pb) {
    return da < db || (da == db && pa < pb);
}

// include/cgrt.h "Neighbour queries": membership, then the slot rule
template <bool LIST>
__device__ __forceinline__ void neighbor_apply(const float dist2, const uint32_t prim, NeighborSlot& Q) {
    if (!(dist2 <= Q.r2)) return;  // (a NaN never qualifies)
    Q.count++;
    if (!LIST || Q.room == 0u) return;
    size_t j = Q.kept;
    if (Q.kept == Q.room) {  // full: the largest one leaves, unless that is the new one
        if (!neighbor_before(dist2, prim, __uint_as_float(Q.rec[2 * (j - 1)]), Q.rec[2 * (j - 1) + 1])) return;
        j--;
    } else {
        Q.kept++;
    }
    while (j > 0) {
        const uint32_t pd = Q.rec[2 * (j - 1)], pp = Q.rec[2 * (j - 1) + 1];
        if (!neighbor_before(dist2, prim, __uint_as_float(pd), pp)) break;
        Q.rec[2 * j] = pd;
        Q.rec[2 * j + 1] = pp;
        j--;
    }
    Q.rec[2 * j] = __float_as_uint(dist2);
    Q.rec[2 * j + 1] = prim;
    if (Q.shrink && Q.kept == Q.room) Q.bound = __uint_as_float(Q.rec[2 * (size_t)(Q.room - 1u)]);
}

// records [first, first + cnt)
template <bool LIST>
__device__ __forceinline__ void neighbor_records(const SceneDev& S, const unsigned long long first, const uint32_t cnt, const float px,
                                                 const float py, const float pz, NeighborSlot& Q) {
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
    NeighborSlot Q;
    Q.r2 = radius2 ? radius2[i] : max_dist2;
    Q.bound = Q.r2;
    Q.kept = 0u;
    Q.count = 0u;
    Q.rec = out;
    Q.len = 0ull;
    Q.shrink = LIST && counts == nullptr;  // the full count needs every neighbour, whatever the slot holds
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
    unsigned long long c_nodes = 0, c_tris = 0;
    const bool wanted = !LIST || counts != nullptr || Q.room != 0u;  // (an empty slot without a count asks for nothing)
    // a radius that is NaN or below zero and a point that is not finite have no neighbours
    if (S.root_ref != REF_NONE && wanted && Q.r2 >= 0.0f && finite3(px, py, pz)) {
        if (BRUTE) {
            if (COUNT) c_tris += S.ntris;
            neighbor_records<LIST>(S, S.tri_base, S.ntris, px, py, pz, Q);
        } else {
            uint32_t* const stk = s_stk + (threadIdx.x >> 6) * (2 * CLOSEST_STACK_ENTRIES * 64) + (threadIdx.x & 63u);
            uint32_t cur = topo_ref(S.root_ref);
            int sp = 0;
            for (;;) {
                bool pop = true;
                if (cur & REF_LEAF) {  // a run of 1..32 records
                    const uint32_t cnt = ((cur >> 26) & 31u) + 1u;
                    if (COUNT) c_tris += cnt;
                    neighbor_records<LIST>(S, cur & REF_INDEX26, cnt, px, py, pz, Q);
                } else if (cur & CL_LEAF) {  // a reference leaf scanned linearly
                    const LeafRec L = S.leaves[cur & ~CL_LEAF];
                    if (COUNT) c_tris += L.count;
                    neighbor_records<LIST>(S, L.first, L.count, px, py, pz, Q);
                } else {
                    if (COUNT) c_nodes++;
                    uint32_t k0, k1, k2 = 0xffffffffu, k3 = 0xffffffffu, f0, f1, f2 = REF_NONE, f3 = REF_NONE;
                    if (cur & CL_SUB) {  // a transposed node (cgrt_layout.h SubNode): lo.x, hi.x, lo.y, hi.y, lo.z, hi.z of the four children, then the references
                        const float4* q = reinterpret_cast<const float4*>(S.subnodes + (cur & ~CL_SUB));
                        const float4 lx = q[0], hx = q[1], ly = q[2], hy = q[3], lz = q[4], hz = q[5];
                        const uint4 m = *reinterpret_cast<const uint4*>(q + 6);
                        const float l0 = box_lb2(lx.x, hx.x, ly.x, hy.x, lz.x, hz.x, px, py, pz);
                        const float l1 = box_lb2(lx.y, hx.y, ly.y, hy.y, lz.y, hz.y, px, py, pz);
                        const float l2 = box_lb2(lx.z, hx.z, ly.z, hy.z, lz.z, hz.z, px, py, pz);
                        const float l3 = box_lb2(lx.w, hx.w, ly.w, hy.w, lz.w, hz.w, px, py, pz);
                        k0 = child_key(m.x, l0, Q.bound);
                        k1 = child_key(m.y, l1, Q.bound);
                        k2 = child_key(m.z, l2, Q.bound);
                        k3 = child_key(m.w, l3, Q.bound);
                        f0 = sub_ref(m.x), f1 = sub_ref(m.y), f2 = sub_ref(m.z), f3 = sub_ref(m.w);  // (only read where the key is not all ones)
                    } else {  // NodePacket: two child boxes {lo.xyz, hi.xyz}
                        const float4* q = reinterpret_cast<const float4*>(S.packets + cur);
                        const float4 a = q[0], b = q[1], c = q[2];
                        const uint4 m = *reinterpret_cast<const uint4*>(q + 3);
                        const float l0 = box_lb2(a.x, a.w, a.y, b.x, a.z, b.y, px, py, pz);
                        const float l1 = box_lb2(b.z, c.y, b.w, c.z, c.x, c.w, px, py, pz);
                        k0 = child_key(m.x, l0, Q.bound);
                        k1 = child_key(m.y, l1, Q.bound);
                        f0 = topo_ref(m.x), f1 = topo_ref(m.y);
                    }
                    // ascending by key: absent and culled children (all ones) last
                    order2(k0, f0, k1, f1);
                    order2(k2, f2, k3, f3);
                    order2(k0, f0, k2, f2);
                    order2(k1, f1, k3, f3);
                    order2(k1, f1, k2, f2);
                    // farthest first, so that the deferred children pop nearest first (a full slot's bound shrinks sooner)
                    if (k3 != 0xffffffffu) {
                        stk[(2 * sp) * 64] = f3, stk[(2 * sp + 1) * 64] = k3;
                        sp++;
                    }
                    if (k2 != 0xffffffffu) {
                        stk[(2 * sp) * 64] = f2, stk[(2 * sp + 1) * 64] = k2;
                        sp++;
                    }
                    if (k1 != 0xffffffffu) {
                        stk[(2 * sp) * 64] = f1, stk[(2 * sp + 1) * 64] = k1;
                        sp++;
                    }
                    if (k0 != 0xffffffffu) {
                        cur = f0;
                        pop = false;
                    }
                }
                if (pop) {
                    bool got = false;
                    while (sp > 0) {
                        sp--;
                        const uint32_t r = stk[(2 * sp) * 64];
                        const float lb = __uint_as_float(stk[(2 * sp + 1) * 64]);
                        if (!(lb > Q.bound)) {  // the bound may have fallen since the child was deferred
                            cur = r;
                            got = true;
                            break;
                        }
                    }
                    if (!got) break;
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
