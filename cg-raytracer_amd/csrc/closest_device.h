// closest_device.h -- the device functions of the closest-point search (include/cgrt.h "Closest-point queries"):
// the per-triangle function, the box lower bound, the child ordering, the search stack's encoding and the walk itself (closest_walk).
// closest_kernels.hip (k_closest, k_closest_brute), sdf_kernels.hip (phase 1 of k_sdf) and neighbor_kernels.hip (k_neighbors) call these
// very functions, so all compute the same dist2, bit for bit, and visit the tree under the same rule.
#pragma once
#include <hip/hip_runtime.h>

#include "closest_kernels.h"
#include "query_device.h"

namespace cgrt {

#define CGRT_CLOSEST_BLOCK 128

// A deferred subtree on the stack.  Topology references and accelerator references overlap (bit 30 is REF_LEAF_ACCEL in the first and a
// count bit of a run in the second), so the stack holds one encoding of its own:
//   bit 31 set             a run of records, exactly the accelerator's REF_LEAF | (count - 1) << 26 | first record
//   CL_SUB  | index        an accelerator node (two consecutive SubNodes)
//   CL_LEAF | index        a reference leaf without accelerator: LeafRec{first, count}
//   index                  a NodePacket
const uint32_t CL_SUB = 0x20000000u;
const uint32_t CL_LEAF = 0x40000000u;
static_assert(SUB_MAX_RECORDS <= CL_SUB, "record indices must stay below the kind bits");
static_assert(CLOSEST_STACK_ENTRIES == (MAX_LEVELS - 1) + (SUB_WIDTH - 1) * SUB_MAX_DEPTH,
              "the stack holds one deferred child per NodePacket level and three per accelerator level");
static_assert(2 * CLOSEST_STACK_ENTRIES * CGRT_CLOSEST_BLOCK * 4 <= 65536, "the stacks of a workgroup must fit its LDS");

__device__ __forceinline__ uint32_t topo_ref(const uint32_t r) {  // a child reference of a NodePacket (or the root), not REF_NONE
    if (!(r & REF_LEAF)) return r;
    return (r & REF_LEAF_ACCEL) ? (CL_SUB | (r & REF_INDEX26)) : (CL_LEAF | (r & ~REF_LEAF));
}
__device__ __forceinline__ uint32_t sub_ref(const uint32_t r) {  // a child reference of an accelerator node, not REF_NONE
    return (r & REF_LEAF) ? r : (CL_SUB | r);
}

struct Best {
    float d2;       // the bound: best dist2 so far, max_dist2 while prim == CGRT_NO_PRIM
    uint32_t prim;
    float qx, qy, qz, v, w;
};

__device__ __forceinline__ float dot3(const float x0, const float x1, const float x2, const float y0, const float y1, const float y2) {
    return (x0 * y0 + x1 * y1) + x2 * y2;
}
__device__ __forceinline__ float clamp1(const float q, const float a, const float b, const float c) {
    const float lo = fminf(a, fminf(b, c)), hi = fmaxf(a, fmaxf(b, c));  // (a NaN vertex coordinate makes dist2 NaN whatever these return)
    return q < lo ? lo : (q > hi ? hi : q);
}

// One triangle's answer for a query: the definition's q, v, w and dist2, and the record's prim_id.
struct TriClosest {
    float dist2;
    uint32_t prim;
    float qx, qy, qz, v, w;
};

// include/cgrt.h "Closest-point queries", the definition, operation for operation; r0..r3 = the record's four 16-byte quarters.
// A pure function of (p, triangle): closest_tri takes its result into a Best, the neighbour search (neighbor_kernels.hip) into a slot.
__device__ __forceinline__ TriClosest closest_eval(const float4 r0, const float4 r1, const float4 r2, const float4 r3, const float px,
                                                   const float py, const float pz) {
    const float ax = r0.x, ay = r0.y, az = r0.z, bx = r0.w, by = r1.x, bz = r1.y, cx = r1.z, cy = r1.w, cz = r2.x;
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
    const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e1 = d4 - d3, e2 = d5 - d6;
    const bool rA = d1 <= 0.0f && d2 <= 0.0f;
    const bool rB = d3 >= 0.0f && d4 <= d3;
    const bool rAB = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool rC = d6 >= 0.0f && d5 <= d6;
    const bool rAC = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool rBC = va <= 0.0f && e1 >= 0.0f && e2 >= 0.0f;
    // every non-vertex region divides once: one division, its operands selected in the regions' priority
    float num = 1.0f, den = (va + vb) + vc;
    if (rBC) num = e1, den = e1 + e2;
    if (rAC) num = d2, den = d2 - d6;
    if (rC) num = 0.0f, den = 1.0f;
    if (rAB) num = d1, den = d1 - d3;
    if (rA || rB) num = 0.0f, den = 1.0f;
    const float t = num / den;
    float v, w;
    if (rA) {
        v = 0.0f, w = 0.0f;
    } else if (rB) {
        v = 1.0f, w = 0.0f;
    } else if (rAB) {
        v = t, w = 0.0f;
    } else if (rC) {
        v = 0.0f, w = 1.0f;
    } else if (rAC) {
        v = 0.0f, w = t;
    } else if (rBC) {
        w = t, v = 1.0f - w;
    } else {
        v = vb * t, w = vc * t;
    }
    float qx = (ax + abx * v) + acx * w, qy = (ay + aby * v) + acy * w, qz = (az + abz * v) + acz * w;
    const bool atA = rA, atB = !rA && rB, atC = !rA && !rB && !rAB && rC;
    qx = atA ? ax : (atB ? bx : (atC ? cx : qx));
    qy = atA ? ay : (atB ? by : (atC ? cy : qy));
    qz = atA ? az : (atB ? bz : (atC ? cz : qz));
    qx = clamp1(qx, ax, bx, cx);
    qy = clamp1(qy, ay, by, cy);
    qz = clamp1(qz, az, bz, cz);
    const float rx = px - qx, ry = py - qy, rz = pz - qz;
    TriClosest E;
    E.dist2 = dot3(rx, ry, rz, rx, ry, rz);
    E.prim = __float_as_uint(r3.y);
    E.qx = qx, E.qy = qy, E.qz = qz, E.v = v, E.w = w;
    return E;
}

__device__ __forceinline__ void closest_tri(const float4 r0, const float4 r1, const float4 r2, const float4 r3, const float px, const float py,
                                            const float pz, Best& B) {
    const TriClosest E = closest_eval(r0, r1, r2, r3, px, py, pz);
    // dist2 <= max_dist2 qualifies (prim starts as CGRT_NO_PRIM, above every id); smaller dist2 wins, equal dist2 goes to the smaller id
    const bool take = E.dist2 < B.d2 || (E.dist2 == B.d2 && E.prim < B.prim);
    B.d2 = take ? E.dist2 : B.d2;
    B.prim = take ? E.prim : B.prim;
    B.qx = take ? E.qx : B.qx;
    B.qy = take ? E.qy : B.qy;
    B.qz = take ? E.qz : B.qz;
    B.v = take ? E.v : B.v;
    B.w = take ? E.w : B.w;
}

// squared distance from p to the box, in dist2's operations and association
__device__ __forceinline__ float box_lb2(const float lox, const float hix, const float loy, const float hiy, const float loz, const float hiz,
                                         const float px, const float py, const float pz) {
    const float dx = fmaxf(fmaxf(lox - px, px - hix), 0.0f);
    const float dy = fmaxf(fmaxf(loy - py, py - hiy), 0.0f);
    const float dz = fmaxf(fmaxf(loz - pz, pz - hiz), 0.0f);
    return (dx * dx + dy * dy) + dz * dz;
}

// Sort key of a child: the bits of its lb2 (non-negative floats order as integers; a NaN bound never culls and sorts first, as 0), all
// ones for a child that is absent or culled.
__device__ __forceinline__ uint32_t child_key(const uint32_t ref, const float lb, const float bound) {
    if (ref == REF_NONE || lb > bound) return 0xffffffffu;
    return lb != lb ? 0u : __float_as_uint(lb);
}
__device__ __forceinline__ void order2(uint32_t& ka, uint32_t& ra, uint32_t& kb, uint32_t& rb) {
    const bool s = ka > kb;
    const uint32_t k0 = s ? kb : ka, k1 = s ? ka : kb, q0 = s ? rb : ra, q1 = s ? ra : rb;
    ka = k0, kb = k1, ra = q0, rb = q1;
}

// The search of one query p, from the root (S.root_ref != REF_NONE) over the structure every scene has -- the reference tree's
// NodePackets (two child boxes), then the leaves' 4-wide accelerators (SubNode pairs) down to runs of 1..32 records, or plain LeafRec
// ranges where a leaf has no accelerator.  A subtree is skipped iff `lb2 > bound()` is TRUE; bound() is re-read at every use, because
// records(first, count) -- the caller's evaluation of records [first, first + count) -- may lower it.  The nearest child is entered, the
// others are deferred farthest-first with their lb2 and culled again on pop.  stk: the lane's column of a lane-interleaved LDS region,
// slot s at stk[s * 64]; entry e = slots 2e {ref}, 2e + 1 {lb2}, CLOSEST_STACK_ENTRIES entries.
template <bool COUNT, class Records, class Bound>
__device__ __forceinline__ void closest_walk(const SceneDev& S, const float px, const float py, const float pz, uint32_t* const stk,
                                             const Records& records, const Bound& bound, unsigned long long& c_nodes,
                                             unsigned long long& c_tris) {
    uint32_t cur = topo_ref(S.root_ref);
    int sp = 0;
    for (;;) {
        bool pop = true;
        if (cur & REF_LEAF) {  // a run of 1..32 records
            const uint32_t first = cur & REF_INDEX26, cnt = ((cur >> 26) & 31u) + 1u;
            if (COUNT) c_tris += cnt;
            records(first, cnt);
        } else if (cur & CL_LEAF) {  // a reference leaf scanned linearly
            const LeafRec L = S.leaves[cur & ~CL_LEAF];
            if (COUNT) c_tris += L.count;
            records(L.first, L.count);
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
                k0 = child_key(m.x, l0, bound());
                k1 = child_key(m.y, l1, bound());
                k2 = child_key(m.z, l2, bound());
                k3 = child_key(m.w, l3, bound());
                f0 = sub_ref(m.x), f1 = sub_ref(m.y), f2 = sub_ref(m.z), f3 = sub_ref(m.w);  // (only read where the key is not all ones)
            } else {  // NodePacket: two child boxes {lo.xyz, hi.xyz}
                const float4* q = reinterpret_cast<const float4*>(S.packets + cur);
                const float4 a = q[0], b = q[1], c = q[2];
                const uint4 m = *reinterpret_cast<const uint4*>(q + 3);
                const float l0 = box_lb2(a.x, a.w, a.y, b.x, a.z, b.y, px, py, pz);
                const float l1 = box_lb2(b.z, c.y, b.w, c.z, c.x, c.w, px, py, pz);
                k0 = child_key(m.x, l0, bound());
                k1 = child_key(m.y, l1, bound());
                f0 = topo_ref(m.x), f1 = topo_ref(m.y);
            }
            // ascending by key: absent and culled children (all ones) last
            order2(k0, f0, k1, f1);
            order2(k2, f2, k3, f3);
            order2(k0, f0, k2, f2);
            order2(k1, f1, k3, f3);
            order2(k1, f1, k2, f2);
            // farthest first, so that the deferred children pop nearest first (a falling bound falls sooner)
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
                if (!(lb > bound())) {  // the bound may have fallen since the child was deferred
                    cur = r;
                    got = true;
                    break;
                }
            }
            if (!got) break;
        }
    }
}

// The closest-point search proper: the walk with the minimum taken into B, whose d2 is the bound (k_closest, phase 1 of k_sdf).
template <bool COUNT>
__device__ __forceinline__ void closest_search(const SceneDev& S, const float px, const float py, const float pz, uint32_t* const stk, Best& B,
                                               unsigned long long& c_nodes, unsigned long long& c_tris) {
    closest_walk<COUNT>(
        S, px, py, pz, stk,
        [&](const uint32_t first, const uint32_t cnt) {
            const float4* q = reinterpret_cast<const float4*>(S.tris + first);
            for (uint32_t k = 0; k < cnt; k++) closest_tri(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3], px, py, pz, B);
        },
        [&]() { return B.d2; }, c_nodes, c_tris);
}

}  // namespace cgrt
