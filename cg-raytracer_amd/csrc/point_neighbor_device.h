// point_neighbor_device.h -- the query side of the point-set grid, the one copy that point_neighbor_kernels.hip (point-set neighbours;
// DESIGN.md section 5.30) and point_frame_kernels.hip (point-set frames) both include: what a query reads of a
// built grid, the distance, membership, the reach of a bound and the search of one lane.  The argument why the search meets every data
// point that can qualify exactly once stands at the head of point_neighbor_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "point_grid_device.h"
#include "point_neighbor_kernels.h"
#include "query_device.h"

namespace cgrt {

const uint32_t kSkipSameIndex = 1u;  // include/cgrt.h CGRT_POINTS_SKIP_SAME_INDEX

__device__ __forceinline__ unsigned long long cell_key(uint32_t cx, uint32_t cy, uint32_t cz) {
    return (unsigned long long)cx | ((unsigned long long)cy << 21) | ((unsigned long long)cz << 42);
}

// what a query reads of a built grid
struct PointGridView {
    const uint32_t* bstart;
    const float4* epos;
    const unsigned long long* ekey;
    uint32_t bmask, entries, used;
    Grid g;
    float hi[3];
};
// False: no entries, or a header that does not describe a grid inside grid_bytes (uniform over the launch).
__device__ __forceinline__ bool grid_view(const void* grid, const unsigned long long grid_bytes, PointGridView& V) {
    const char* const p0 = reinterpret_cast<const char*>(((uintptr_t)grid + 15u) & ~(uintptr_t)15u);
    const unsigned long long slack = (unsigned long long)(p0 - static_cast<const char*>(grid));
    V.used = 0u;
    if (grid_bytes < slack + 64ull) return false;
    const uint32_t* const hdr = reinterpret_cast<const uint32_t*>(p0);
    const uint32_t m = hdr[PG_M];
    V.bmask = hdr[PG_BMASK];
    if (m > 0x7fffffffu || V.bmask != poisson_buckets(m) - 1u) return false;
    const PointGridLayout L = point_grid_layout(m);
    if (slack + L.bytes > grid_bytes) return false;
    V.bstart = reinterpret_cast<const uint32_t*>(p0 + L.bstart);
    V.epos = reinterpret_cast<const float4*>(p0 + L.epos);
    V.ekey = reinterpret_cast<const unsigned long long*>(p0 + L.ekey);
    V.entries = min(V.bstart[V.bmask + 1u], m);
    V.used = hdr[PG_USED];
    if (V.entries == 0u) return false;
    V.g = load_grid(hdr, __uint_as_float(hdr[PG_CELL]));
#pragma unroll
    for (int a = 0; a < 3; a++) V.hi[a] = unordered(hdr[H_HI + a]);
    return true;
}

// include/cgrt.h "Point-set neighbours", Distance: every operation rounded on its own (-ffp-contract=off); Poisson's conflict() arithmetic
__device__ __forceinline__ float point_dist2(float qx, float qy, float qz, float x, float y, float z) {
    const float dx = qx - x, dy = qy - y, dz = qz - z;
    return (dx * dx + dy * dy) + dz * dz;
}
// membership; a neighbour is taken into the slot under its d2 (a NaN never qualifies).  Q.bound is the query's r2, or below it while a
// full slot shrinks it
template <bool LIST, bool COUNT>
__device__ __forceinline__ void point_apply(float qx, float qy, float qz, float x, float y, float z, uint32_t j, uint32_t skip, QuerySlot& Q,
                                            unsigned long long& c_d2) {
    if (j == skip) return;
    const float d2 = point_dist2(qx, qy, qz, x, y, z);
    if (COUNT) c_d2++;
    if (d2 <= Q.bound) slot_take<LIST>(d2, j, Q);
}
// R of the head comment for a bound in [0, FLT_MAX)
__device__ __forceinline__ float query_reach(float r2) {
    const float up = __uint_as_float(__float_as_uint(fabsf(r2)) + 1u);
    return __uint_as_float(__float_as_uint(sqrtf(up)) + 2u);
}

// The search of the lane whose query is (px, py, pz), finite, with a bound Q.limit >= 0: every data point that can qualify is offered to
// the slot exactly once.  BRUTE: the A.m points of A.data in turn (A: the kernel's argument record); otherwise the grid V (built:
// grid_view's answer), by cells, or by the entry array where the range has more cells than the grid has entries.  c_*: the work of a
// counted search (COUNT; otherwise untouched) -- cells visited, entries read, entries of another cell, d2 evaluations, linear walks.
template <bool LIST, bool COUNT, bool BRUTE, class Args>
__device__ __forceinline__ void point_search(const Args& A, const PointGridView& V, const bool built, const float px, const float py, const float pz,
                                             const uint32_t skip, QuerySlot& Q, unsigned long long& c_cells, unsigned long long& c_read,
                                             unsigned long long& c_foreign, unsigned long long& c_d2, unsigned long long& c_linear) {
    if (BRUTE) {
        for (uint32_t j = 0u; j < (uint32_t)A.m; j++) {
            const float x = A.data[3ull * j], y = A.data[3ull * j + 1], z = A.data[3ull * j + 2];
            if (finite3(x, y, z)) point_apply<LIST, COUNT>(px, py, pz, x, y, z, j, skip, Q, c_d2);
        }
    } else if (built) {
        unsigned long long ncells = ~0ull;
        uint32_t x0 = 0u, x1 = 0u, y0 = 0u, y1 = 0u, z0 = 0u, z1 = 0u;
        if (Q.limit < 3.402823466e+38f) {
            const float R = query_reach(Q.limit);
            const Grid& g = V.g;
            x0 = cell(px - R, g.lo[0], g.h), x1 = min(cell(px + R, g.lo[0], g.h), cell(V.hi[0], g.lo[0], g.h));
            y0 = cell(py - R, g.lo[1], g.h), y1 = min(cell(py + R, g.lo[1], g.h), cell(V.hi[1], g.lo[1], g.h));
            z0 = cell(pz - R, g.lo[2], g.h), z1 = min(cell(pz + R, g.lo[2], g.h), cell(V.hi[2], g.lo[2], g.h));
            const unsigned long long nx = x1 >= x0 ? x1 - x0 + 1u : 0u, ny = y1 >= y0 ? y1 - y0 + 1u : 0u, nz = z1 >= z0 ? z1 - z0 + 1u : 0u;
            ncells = nx * ny * nz;  // each factor at most 2^21
        }
        if (ncells > V.entries) {
            if (COUNT) c_linear++;
            for (uint32_t t = 0u; t < V.entries; t++) {
                const float4 q = V.epos[t];
                if (COUNT) c_read++;
                point_apply<LIST, COUNT>(px, py, pz, q.x, q.y, q.z, __float_as_uint(q.w), skip, Q, c_d2);
            }
        } else if (ncells != 0ull) {
            for (uint32_t cz = z0; cz <= z1; cz++)
                for (uint32_t cy = y0; cy <= y1; cy++)
                    for (uint32_t cx = x0; cx <= x1; cx++) {
                        const unsigned long long key = cell_key(cx, cy, cz);
                        const uint32_t b = bucket(cx, cy, cz, V.bmask);
                        const uint32_t end = min(V.bstart[b + 1u], V.entries);
                        if (COUNT) c_cells++;
                        for (uint32_t t = V.bstart[b]; t < end; t++) {
                            if (COUNT) c_read++;
                            if (V.ekey[t] != key) {  // a point of another cell: met in that cell's visit, if the range holds it
                                if (COUNT) c_foreign++;
                                continue;
                            }
                            const float4 q = V.epos[t];
                            point_apply<LIST, COUNT>(px, py, pz, q.x, q.y, q.z, __float_as_uint(q.w), skip, Q, c_d2);
                        }
                    }
        }
    }
}

}  // namespace cgrt
