// closest_kernels.hip -- closest-point queries (include/cgrt.h cgrt_closest_points*): for every query point the
// nearest point of the scene's triangles, its squared distance, the triangle and the barycentrics.  Nothing is traced.
//
// The per-triangle function (closest_tri) is Ericson's region walk in f32 with every operation rounded, followed by ONE clamp of the point
// to the triangle's own bounding box.  The clamp is what makes the tree search exact: every box of the structures is the exact min / max
// of its triangles' vertices, so the clamped point lies in every ancestor box, and box_lb2 -- the squared distance from the query to a
// box, in the same operations and association as dist2 -- never exceeds the dist2 of a triangle under that box, in f32, with no slack
// (per axis |p - q| >= dx in the reals; rounding, squaring and same-order summing are monotone).  A subtree is skipped iff
// `lb2 > bound` is TRUE, bound = the best dist2 so far (max_dist2 while nothing has been accepted): under that rule the search returns
// the brute-force result whatever the visiting order.  Equal dist2 goes to the smaller prim_id.
//
// k_closest: one query per lane over the structure every scene has -- the reference tree's NodePackets (two child boxes), then the
// leaves' 4-wide accelerators (SubNode pairs) down to runs of 1..32 records, or plain LeafRec ranges where a leaf has no accelerator.
// The nearest child is entered, the others are deferred farthest-first with their lb2 and culled again on pop.  The per-lane stack is
// lane-interleaved in LDS, two dwords per entry.  k_closest_brute: every record in turn, same function, same rule (validation).
#include <hip/hip_runtime.h>

#include "closest_device.h"
#include "closest_kernels.h"

namespace cgrt {

namespace {

__device__ __forceinline__ void store_result(CgrtClosestDev* out, const unsigned long long i, const Best& B) {
    float* o = reinterpret_cast<float*>(out + i);  // (the caller's buffer is only 4-byte aligned)
    if (B.prim == REF_NONE) {
        o[0] = o[1] = o[2] = 0.0f;
        o[3] = __builtin_inff();
        o[4] = __uint_as_float(0xffffffffu);
        o[5] = o[6] = o[7] = 0.0f;
        return;
    }
    o[0] = B.qx;
    o[1] = B.qy;
    o[2] = B.qz;
    o[3] = B.d2;
    o[4] = __uint_as_float(B.prim);
    o[5] = (1.0f - B.v) - B.w;
    o[6] = B.v;
    o[7] = B.w;
}

template <bool COUNT>
__global__ __launch_bounds__(CGRT_CLOSEST_BLOCK) void k_closest(const SceneDev S, const float* __restrict__ points, const uint32_t n,
                                                                 const float max_dist2, CgrtClosestDev* __restrict__ out,
                                                                 unsigned long long* __restrict__ counters) {
    // slot s of lane l of wave w at w * (2 * CLOSEST_STACK_ENTRIES * 64) + s * 64 + l; entry e = slots 2e {ref}, 2e + 1 {lb2}
    __shared__ uint32_t s_stk[2 * CLOSEST_STACK_ENTRIES * CGRT_CLOSEST_BLOCK];
    const unsigned long long i = (unsigned long long)blockIdx.x * CGRT_CLOSEST_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t* const stk = s_stk + (threadIdx.x >> 6) * (2 * CLOSEST_STACK_ENTRIES * 64) + (threadIdx.x & 63u);
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    Best B;
    B.d2 = max_dist2;
    B.prim = REF_NONE;
    B.qx = B.qy = B.qz = B.v = B.w = 0.0f;
    unsigned long long c_nodes = 0, c_tris = 0;
    if (S.root_ref != REF_NONE && finite3(px, py, pz)) {
        uint32_t cur = topo_ref(S.root_ref);
        int sp = 0;
        for (;;) {
            bool pop = true;
            if (cur & REF_LEAF) {  // a run of 1..32 records
                const uint32_t first = cur & REF_INDEX26, cnt = ((cur >> 26) & 31u) + 1u;
                const float4* q = reinterpret_cast<const float4*>(S.tris + first);
                if (COUNT) c_tris += cnt;
                for (uint32_t k = 0; k < cnt; k++) closest_tri(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3], px, py, pz, B);
            } else if (cur & CL_LEAF) {  // a reference leaf scanned linearly
                const LeafRec L = S.leaves[cur & ~CL_LEAF];
                const float4* q = reinterpret_cast<const float4*>(S.tris + L.first);
                if (COUNT) c_tris += L.count;
                for (uint32_t k = 0; k < L.count; k++) closest_tri(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3], px, py, pz, B);
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
                    k0 = child_key(m.x, l0, B.d2);
                    k1 = child_key(m.y, l1, B.d2);
                    k2 = child_key(m.z, l2, B.d2);
                    k3 = child_key(m.w, l3, B.d2);
                    f0 = sub_ref(m.x), f1 = sub_ref(m.y), f2 = sub_ref(m.z), f3 = sub_ref(m.w);  // (only read where the key is not all ones)
                } else {  // NodePacket: two child boxes {lo.xyz, hi.xyz}
                    const float4* q = reinterpret_cast<const float4*>(S.packets + cur);
                    const float4 a = q[0], b = q[1], c = q[2];
                    const uint4 m = *reinterpret_cast<const uint4*>(q + 3);
                    const float l0 = box_lb2(a.x, a.w, a.y, b.x, a.z, b.y, px, py, pz);
                    const float l1 = box_lb2(b.z, c.y, b.w, c.z, c.x, c.w, px, py, pz);
                    k0 = child_key(m.x, l0, B.d2);
                    k1 = child_key(m.y, l1, B.d2);
                    f0 = topo_ref(m.x), f1 = topo_ref(m.y);
                }
                // ascending by key: absent and culled children (all ones) last
                order2(k0, f0, k1, f1);
                order2(k2, f2, k3, f3);
                order2(k0, f0, k2, f2);
                order2(k1, f1, k3, f3);
                order2(k1, f1, k2, f2);
                // farthest first, so that the deferred children pop nearest first
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
                    if (!(lb > B.d2)) {  // the bound may have fallen since the child was deferred
                        cur = r;
                        got = true;
                        break;
                    }
                }
                if (!got) break;
            }
        }
    }
    store_result(out, i, B);
    if (COUNT) {
        atomicAdd(counters, c_nodes);
        atomicAdd(counters + 1, c_tris);
    }
}

__global__ __launch_bounds__(256) void k_closest_brute(const SceneDev S, const float* __restrict__ points, const uint32_t n, const float max_dist2,
                                                       CgrtClosestDev* __restrict__ out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    Best B;
    B.d2 = max_dist2;
    B.prim = REF_NONE;
    B.qx = B.qy = B.qz = B.v = B.w = 0.0f;
    if (S.root_ref != REF_NONE && finite3(px, py, pz)) {
        const float4* q = reinterpret_cast<const float4*>(S.tris + S.tri_base);
        for (uint32_t k = 0; k < S.ntris; k++) closest_tri(q[4ull * k], q[4ull * k + 1], q[4ull * k + 2], q[4ull * k + 3], px, py, pz, B);
    }
    store_result(out, i, B);
}

}  // namespace

hipError_t launch_closest(const SceneDev& S, const float* points, uint64_t n, float max_dist2, CgrtClosestDev* out, unsigned long long* counters,
                          hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + CGRT_CLOSEST_BLOCK - 1) / CGRT_CLOSEST_BLOCK)), block(CGRT_CLOSEST_BLOCK);
    if (counters)
        hipLaunchKernelGGL(k_closest<true>, grid, block, 0, stream, S, points, (uint32_t)n, max_dist2, out, counters);
    else
        hipLaunchKernelGGL(k_closest<false>, grid, block, 0, stream, S, points, (uint32_t)n, max_dist2, out, counters);
    return hipGetLastError();
}

hipError_t launch_closest_brute(const SceneDev& S, const float* points, uint64_t n, float max_dist2, CgrtClosestDev* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + 255u) / 256u)), block(256);
    hipLaunchKernelGGL(k_closest_brute, grid, block, 0, stream, S, points, (uint32_t)n, max_dist2, out);
    return hipGetLastError();
}

}  // namespace cgrt
