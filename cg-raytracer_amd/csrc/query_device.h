// query_device.h -- what the one-query-per-lane kernels share beside their walks (closest_device.h closest_walk, crossing_device.h
// cross_walk): the finite test of a query point, the grid point of a lane (sdf_kernels.hip, winding_kernels.hip) and the lane's sorted
// output slot (crossing_kernels.hip, neighbor_kernels.hip; DESIGN.md sections 5.21 and 5.26).  Nothing here reads the scene.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cgrt {

__device__ __forceinline__ bool finite3(const float x, const float y, const float z) {
    return fabsf(x) <= 3.402823466e+38f && fabsf(y) <= 3.402823466e+38f && fabsf(z) <= 3.402823466e+38f;
}

// The grid point of a lane of a 128-lane block: a block is 8 x 4 x 4 grid points, wave w the 4 x 4 x 4 brick at x offset 4w (so that a
// wave's 64 walks open the same nodes), lane l at {l & 3, (l >> 2) & 3, l >> 4}.  False beyond the grid's edge.
__device__ __forceinline__ bool brick_index(const uint32_t nx, const uint32_t ny, const uint32_t nz, uint32_t& ix, uint32_t& iy, uint32_t& iz) {
    const uint32_t bx = (nx + 7u) >> 3, by = (ny + 3u) >> 2;
    const uint32_t b = blockIdx.x, bxi = b % bx, rest = b / bx, byi = rest % by, bzi = rest / by;
    ix = bxi * 8u + (threadIdx.x >> 6) * 4u + (threadIdx.x & 3u);
    iy = byi * 4u + ((threadIdx.x >> 2) & 3u);
    iz = bzi * 4u + ((threadIdx.x >> 4) & 3u);
    return ix < nx && iy < ny && iz < nz;
}
// origin + (float)index * spacing: the product rounded, then the sum (an index is below 2^24: exact as f32)
__device__ __forceinline__ float grid_coord(const float origin, const uint32_t index, const float spacing) {
    return __fadd_rn(origin, __fmul_rn((float)index, spacing));
}

// A lane's slot of a list call's output and its running state.  A record is two dwords {key, prim_id}; the key is the crossing's t or
// the neighbour's dist2.  The lane keeps its slot sorted in global memory by insertion, dropping the largest when full: no atomics, no
// scratch.
struct QuerySlot {
    uint32_t* rec;           // the slot's first record
    unsigned long long len;  // records the slot holds
    uint32_t room;           // min(len, 2^32 - 1): a query has fewer members than that
    uint32_t kept;           // records rec[0 .. kept) are the smallest `kept` members so far, in order
    uint32_t count;          // all members so far
    float limit;             // the query's own limit (the ray's t, the squared radius): what a key is tested against
    float bound;             // what boxes are tested against: limit, or the largest key kept once the slot is full (shrink)
    bool shrink;
};

__device__ __forceinline__ bool slot_before(const float ka, const uint32_t pa, const float kb, const uint32_t pb) {
    return ka < kb || (ka == kb && pa < pb);
}

// Query i's slot: records [offsets[i], offsets[i + 1]) of `out`, or [i * k, (i + 1) * k) without offsets, clamped to `capacity` records.
// Without LIST there is no slot.  counted: the call stores the full count, which needs every member whatever the slot holds, so the
// bound stays the limit.  False when the query asks for nothing (an empty slot without a count).
template <bool LIST>
__device__ __forceinline__ bool slot_open(QuerySlot& Q, const float limit, uint32_t* const out, const unsigned long long* const offsets,
                                          const uint32_t k, const unsigned long long capacity, const bool counted, const unsigned long long i) {
    Q.limit = limit;
    Q.bound = limit;
    Q.kept = 0u;
    Q.count = 0u;
    Q.rec = out;
    Q.len = 0ull;
    Q.shrink = LIST && !counted;
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
    return !LIST || counted || Q.room != 0u;
}

// A member {key, prim} of the query: counted, then inserted in (key, prim_id) order; a full slot's bound shrinks to the largest key
// kept, non-strictly, so an equal-key smaller prim_id still arrives.
template <bool LIST>
__device__ __forceinline__ void slot_take(const float key, const uint32_t prim, QuerySlot& Q) {
    Q.count++;
    if (!LIST || Q.room == 0u) return;
    size_t j = Q.kept;
    if (Q.kept == Q.room) {  // full: the largest one leaves, unless that is the new one
        if (!slot_before(key, prim, __uint_as_float(Q.rec[2 * (j - 1)]), Q.rec[2 * (j - 1) + 1])) return;
        j--;
    } else {
        Q.kept++;
    }
    while (j > 0) {
        const uint32_t pk = Q.rec[2 * (j - 1)], pp = Q.rec[2 * (j - 1) + 1];
        if (!slot_before(key, prim, __uint_as_float(pk), pp)) break;
        Q.rec[2 * j] = pk;
        Q.rec[2 * j + 1] = pp;
        j--;
    }
    Q.rec[2 * j] = __float_as_uint(key);
    Q.rec[2 * j + 1] = prim;
    if (Q.shrink && Q.kept == Q.room) Q.bound = __uint_as_float(Q.rec[2 * (size_t)(Q.room - 1u)]);
}

template <bool LIST>
__device__ __forceinline__ void slot_close(const QuerySlot& Q, uint32_t* const counts, const unsigned long long i) {
    if (LIST) {
        for (unsigned long long j = Q.kept; j < Q.len; j++) {  // the rest of the slot: {+inf, CGRT_NO_PRIM}
            Q.rec[2 * j] = 0x7f800000u;
            Q.rec[2 * j + 1] = 0xffffffffu;
        }
    }
    if (counts) counts[i] = Q.count;
}

}  // namespace cgrt
