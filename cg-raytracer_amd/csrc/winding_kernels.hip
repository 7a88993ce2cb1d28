// winding_kernels.hip -- generalised winding numbers (include/cgrt.h cgrt_winding_numbers*): for every point the
// sum of the signed solid angles of the scene's triangles over 4 pi, +-1 inside a closed mesh, 0 outside, and a smooth value in between
// near holes.  One kernel, one point per lane, one f32 accumulator per lane:
//
// brute  acc += omega(record k) for k = 0 .. ntris - 1, in record order.
// tree   a depth-first walk of the implicit 8-ary cluster tree of winding_builder.h from its top level, clusters and children in index
//        order.  A cluster that is FAR (d2 > beta2 * r2 is true) adds its dipole (n . d) / (d2 * sqrt(d2)); a near level-0 cluster adds
//        the omega of its records in record order; a near higher cluster is descended.  The walk is STACKLESS: its state is (level,
//        index) and the index of the level's first cluster; "next" is index arithmetic (up while the index is a multiple of 8 or has
//        reached its level's count, done at the top level's count), so it needs neither LDS nor a per-lane stack in scratch.  With no
//        cluster far (beta = +inf) it performs the brute form's additions in the brute form's order: the same bytes.
// The far branch and the exact branch diverge inside a wave: lanes that take the dipole wait for the lanes that evaluate triangles.  That
// is accepted: the additions are not reordered to mend it, the bytes depend on their order (DESIGN.md 5.25 has the work counters).
// Every sum's association is include/cgrt.h's; nothing is contracted (the Makefile's -ffp-contract=off).
// A cluster is one 32-byte load, a record the three 16-byte loads that hold its vertices (its last quarter is not read).
// GRID: the lane makes its point from its grid index (query_device.h brick_index and grid_coord, as k_sdf does: a wave = a 4 x 4 x 4
// brick, so that a wave's 64 walks open the same clusters).
#include <hip/hip_runtime.h>

#include "query_device.h"
#include "winding_kernels.h"

namespace cgrt {

namespace {

#define CGRT_WINDING_BLOCK 128

// 2 * atan2f(num, den) of the triangle {a, b, c} seen from p (van Oosterom and Strackee); q0 = {a.xyz, b.x}, q1 = {b.yz, c.xy}, q2.x = c.z
__device__ __forceinline__ float winding_omega(const float4 q0, const float4 q1, const float4 q2, const float px, const float py, const float pz) {
    const float ax = q0.x - px, ay = q0.y - py, az = q0.z - pz;
    const float bx = q0.w - px, by = q1.x - py, bz = q1.y - pz;
    const float cx = q1.z - px, cy = q1.w - py, cz = q2.x - pz;
    const float la = sqrtf((ax * ax + ay * ay) + az * az);
    const float lb = sqrtf((bx * bx + by * by) + bz * bz);
    const float lc = sqrtf((cx * cx + cy * cy) + cz * cz);
    const float ux = by * cz - bz * cy, uy = bz * cx - bx * cz, uz = bx * cy - by * cx;  // b x c
    const float num = (ax * ux + ay * uy) + az * uz;
    const float ab = (ax * bx + ay * by) + az * bz;
    const float bc = (bx * cx + by * cy) + bz * cz;
    const float ca = (cx * ax + cy * ay) + cz * az;
    const float den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb;
    return 2.0f * atan2f(num, den);
}

__device__ __forceinline__ uint32_t level_count(const uint32_t ntris, const uint32_t level) {  // winding_level_count (ntris <= 2^26: no wrap)
    const uint32_t sh = WINDING_FANOUT_LOG2 * (level + 1u);
    return (ntris + (1u << sh) - 1u) >> sh;
}

template <int GRID, bool COUNT, bool BRUTE>
__global__ __launch_bounds__(CGRT_WINDING_BLOCK) void k_winding(const WindingArgs A, unsigned long long* __restrict__ counters) {
    unsigned long long i;  // the result's index, below A.n
    float px, py, pz;
    if (GRID == WINDING_LIST) {
        i = (unsigned long long)blockIdx.x * CGRT_WINDING_BLOCK + threadIdx.x;
        if (i >= A.n) return;
        px = A.points[3 * i], py = A.points[3 * i + 1], pz = A.points[3 * i + 2];
    } else {
        const uint32_t nx = A.dims[0], ny = A.dims[1], nz = A.dims[2];
        uint32_t ix, iy, iz;
        if (!brick_index(nx, ny, nz, ix, iy, iz)) return;
        i = ((unsigned long long)iz * ny + iy) * nx + ix;
        px = grid_coord(A.origin[0], ix, A.spacing[0]);
        py = grid_coord(A.origin[1], iy, A.spacing[1]);
        pz = grid_coord(A.origin[2], iz, A.spacing[2]);
    }
    unsigned long long c_clusters = 0, c_dipoles = 0, c_tris = 0;
    float acc = 0.0f;
    const bool finite = finite3(px, py, pz);
    if (A.ntris != 0u && finite) {
        const float4* const recs = reinterpret_cast<const float4*>(A.recs);
        if (BRUTE) {
            if (COUNT) c_tris += A.ntris;
            for (uint32_t k = 0; k < A.ntris; k++) acc += winding_omega(recs[4ull * k], recs[4ull * k + 1], recs[4ull * k + 2], px, py, pz);
        } else {
            const uint32_t top = A.nlevels - 1u, top_count = level_count(A.ntris, top);
            uint32_t level = top, index = 0, base = A.top_base;  // base: the index of the level's first cluster
            for (;;) {
                const float4* const q = reinterpret_cast<const float4*>(A.clusters + (base + index));  // (base + index < the tree's clusters)
                const float4 c0 = q[0], c1 = q[1];                                                      // {c.xyz, r2}, {n.xyz, 0}
                const float dx = c0.x - px, dy = c0.y - py, dz = c0.z - pz;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (COUNT) c_clusters++;
                if (d2 > A.beta2 * c0.w) {  // far (false for a NaN: the cluster is opened)
                    acc += ((c1.x * dx + c1.y * dy) + c1.z * dz) / (d2 * sqrtf(d2));
                    if (COUNT) c_dipoles++;
                } else if (level == 0u) {
                    const uint32_t first = index << WINDING_FANOUT_LOG2, last = min(first + 8u, A.ntris);
                    if (COUNT) c_tris += last - first;
                    for (uint32_t k = first; k < last; k++) acc += winding_omega(recs[4ull * k], recs[4ull * k + 1], recs[4ull * k + 2], px, py, pz);
                } else {  // the first child
                    level--;
                    base -= level_count(A.ntris, level);
                    index <<= WINDING_FANOUT_LOG2;
                    continue;
                }
                index++;
                while (level < top && ((index & 7u) == 0u || index >= level_count(A.ntris, level))) {  // the parent's siblings are next
                    base += level_count(A.ntris, level);
                    index = ((index - 1u) >> WINDING_FANOUT_LOG2) + 1u;
                    level++;
                }
                if (level == top && index >= top_count) break;
            }
        }
    }
    const float w = acc * 0.07957747154594767f;  // 1 / (4 pi), rounded to f32
    if (A.w) A.w[i] = w;
    if (A.inside) A.inside[i] = fabsf(w) > A.threshold ? 1 : 0;
    if (COUNT) {
        atomicAdd(counters, c_clusters);
        atomicAdd(counters + 1, c_dipoles);
        atomicAdd(counters + 2, c_tris);
    }
}

template <int GRID, bool COUNT, bool BRUTE>
hipError_t launch_one(const WindingArgs& A, const unsigned blocks, unsigned long long* counters, hipStream_t stream) {
    hipLaunchKernelGGL((k_winding<GRID, COUNT, BRUTE>), dim3(blocks), dim3(CGRT_WINDING_BLOCK), 0, stream, A, counters);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_winding(const WindingArgs& A, WindingPoints how, bool brute, unsigned long long* counters, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    if (A.n > 0x7fffffffu || (!A.w && !A.inside && !counters) || (counters && (how != WINDING_LIST || brute))) return hipErrorInvalidValue;
    if (A.ntris > SUB_MAX_RECORDS || (A.ntris && !A.recs)) return hipErrorInvalidValue;
    if (A.ntris && !brute) {  // the tree must be the one winding_builder.h makes over ntris records
        if (!A.clusters || A.nlevels < 1 || A.nlevels > WINDING_MAX_LEVELS) return hipErrorInvalidValue;
        uint32_t off = 0;
        for (uint32_t L = 0; L + 1 < A.nlevels; L++) {
            if (winding_level_count(A.ntris, L) <= 8u) return hipErrorInvalidValue;
            off += winding_level_count(A.ntris, L);
        }
        if (off != A.top_base || winding_level_count(A.ntris, A.nlevels - 1) > 8u) return hipErrorInvalidValue;
    }
    if (how == WINDING_LIST) {
        if (!A.points) return hipErrorInvalidValue;
        const unsigned linear = (unsigned)(((uint64_t)A.n + CGRT_WINDING_BLOCK - 1) / CGRT_WINDING_BLOCK);
        if (counters) return launch_one<WINDING_LIST, true, false>(A, linear, counters, stream);
        return brute ? launch_one<WINDING_LIST, false, true>(A, linear, nullptr, stream) : launch_one<WINDING_LIST, false, false>(A, linear, nullptr, stream);
    }
    const uint64_t plane = (uint64_t)A.dims[0] * A.dims[1];  // (n fits 31 bits: no product below wraps)
    if (brute || plane == 0 || plane > A.n || plane * A.dims[2] != A.n) return hipErrorInvalidValue;
    // (at most as many bricks as grid points: the count fits the launch's 32-bit grid)
    const uint64_t bricks = (uint64_t)((A.dims[0] + 7u) >> 3) * ((A.dims[1] + 3u) >> 2) * ((A.dims[2] + 3u) >> 2);
    return launch_one<WINDING_GRID_BRICK, false, false>(A, (unsigned)bricks, nullptr, stream);
}

}  // namespace cgrt
