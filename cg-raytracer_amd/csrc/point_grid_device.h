// point_grid_device.h -- the arithmetic of the hashed uniform grid over a point cloud, the one copy that poisson_kernels.hip (Poisson-disk
// sets) and point_neighbor_kernels.hip (point-set neighbours) both include: bounds by
// ordered-integer atomics, the cell of a coordinate, the bucket of a cell, the block scan of the bucket counts.  Nothing here reads a scene.
//
// The grid.  cell(x) = uint(clamp((x - lo) / h, 0, 2^21 - 1)) per axis: f32 subtraction of a constant, division by a positive constant, the
// clamp and the truncation are all monotone in x, so cell() is.  lo is the minimum of the finite points, h = max(R, half extent * 2^-18) (so
// the quotient stays below 2^20 and two floats next to each other are less than a cell apart), R the upward-rounded root of min_dist2 plus an
// ulp.  d2 < min_dist2 implies fl(dx dx) < min_dist2 (adding non-negative terms with round-to-nearest never decreases a value), hence
// dx^2 < min_dist2 exactly, |fl(x_i - x_j)| < R and -- rounding being monotone -- |x_i - x_j| < R exactly; then x_j <= fl(x_i + R) and
// x_j >= fl(x_i - R), again because rounding is monotone and x_j is a float.  So every conflicting j lies in a cell of
// [cell(x_i - R), cell(x_i + R)] per axis, and the round visits exactly that range (two to four cells per axis).  Cells are hashed into
// buckets; a bucket also holds points of other cells and two cells of a range may share a bucket: pairs are then tested that need not be,
// or twice, and a Boolean cannot change.  With a radius that covers the cloud everything lies in one cell: still right, every pair tested.
// (The point-neighbour queries count and list, so there a pair tested twice would show: point_neighbor_kernels.hip keeps each entry's cell
// and extends the argument to `<=`, to a radius per query and to a cell edge the caller chose.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cgrt {

// header words both grids keep in the same place: the bounds of the finite points as ordered integers (the minimum complemented)
enum : uint32_t { H_LO = 0, H_HI = 3 };
const float kCellMax = 2097151.0f;  // 2^21 - 1: three cell coordinates make one 63-bit word

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// floats as unsigned integers of the same order (finite values give words above 0x00800000 and their complements too: 0 is "none yet")
__device__ __forceinline__ uint32_t ordered(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

struct Grid {
    float lo[3], h;
};
// the same values in every thread of every pass: the header's bounds are complete before the first pass that calls this
__device__ __forceinline__ Grid load_grid(const uint32_t* hdr, float R) {
    Grid g;
    float e = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        g.lo[a] = unordered(~hdr[H_LO + a]);
        e = fmaxf(e, unordered(hdr[H_HI + a]) * 0.5f - g.lo[a] * 0.5f);
    }
    g.h = fmaxf(R, e * 3.814697265625e-6f);  // 2^-18 of the half extent: quotients below 2^20
    return g;
}
__device__ __forceinline__ uint32_t cell(float x, float lo, float h) { return (uint32_t)fminf(fmaxf((x - lo) / h, 0.0f), kCellMax); }
__device__ __forceinline__ uint32_t bucket(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t bmask) {
    unsigned long long k = (unsigned long long)cx | ((unsigned long long)cy << 21) | ((unsigned long long)cz << 42);
    k *= 0x9E3779B97F4A7C15ull;
    k ^= k >> 29;
    k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 32;
    return (uint32_t)k & bmask;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

// exclusive scan of one value per thread over the block's 256 threads; *total: the block's sum.  lds: 4 words
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= (uint32_t)d) incl += t;
    }
    if (lane == 63u) lds[w] = incl;
    __syncthreads();
    const uint32_t s0 = lds[0], s1 = lds[1], s2 = lds[2], s3 = lds[3];
    __syncthreads();
    *total = s0 + s1 + s2 + s3;
    return (w > 0u ? s0 : 0u) + (w > 1u ? s1 : 0u) + (w > 2u ? s2 : 0u) + incl - v;
}

}  // namespace cgrt
