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
// k_closest: one query per lane, closest_device.h's closest_search (closest_walk with the minimum taken into a Best) over the structure
// every scene has.  The per-lane stack is lane-interleaved in LDS, two dwords per entry.  k_closest_brute: every record in turn, same
// function, same rule (validation).
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
    if (S.root_ref != REF_NONE && finite3(px, py, pz)) closest_search<COUNT>(S, px, py, pz, stk, B, c_nodes, c_tris);
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
