// point_neighbor_kernels.hip -- point-set neighbours (include/cgrt.h cgrt_point_grid_*, cgrt_count_point_neighbors*,
// cgrt_list_point_neighbors*): for every query point ALL the points of a cloud within its squared radius, counted,
// or listed in (d2, index) order.  d2 is point_dist2 below, a pure function of the two points, so the search only has to reach every
// data point that can qualify, each exactly once, in any order.
//
// The build, all enqueued on the caller's stream (launch_point_grid_build; the grid of point_grid_device.h, which Poisson-disk sets share):
//   k_pgrid_bounds    per data point: finite?; the per-axis minimum and maximum of the finite points by ordered-integer atomics, one
//                     set per wave; thread 0 leaves the caller's cell edge, the bucket mask and m in the header
//   k_pgrid_count     per finite point: its cell, the cell's bucket, one atomic add on the bucket's count (the first one of a bucket
//                     counts the bucket as in use)
//   launch_bucket_scan  the exclusive scan of the bucket counts: poisson_kernels.hip's three scan kernels through its one helper
//   k_pgrid_scatter   per finite point: {x, y, z, index} and the 63-bit key of its cell into the bucket's range (the order inside a bucket
//                     is whatever the atomics gave, and no result depends on it)
// The cell edge is h = max(cell, half extent * 2^-18), computed by load_grid from the header in every pass and in every query alike.
// Nothing is read back: the bucket count follows from m on the host, everything else stays in the header.
//
// The query, k_point_neighbors: one query per lane.  r2 is the query's bound, up the next float above it, R = the root of `up` rounded
// to nearest and moved two floats up (so R >= the exact root of `up`).  A neighbour j has d2 <= r2 < up; adding non-negative terms with
// round-to-nearest never decreases a value, so fl(dx dx) <= d2 < up, and -- rounding being monotone and `up` a float -- dx^2 < up exactly:
// |fl(x_q - x_j)| < R and, again by monotone rounding, |x_q - x_j| < R exactly; then x_j <= fl(x_q + R) and x_j >= fl(x_q - R) because x_j
// is a float.  (With Poisson's strict `<` the bound itself serves as `up`; with `<=` a dx^2 just above r2 may round down to it, which is
// why the next float is taken: that also covers subnormal bounds, where half an ulp is no small relative step.)  cell() is monotone, so
// cell(x_j) lies in [cell(fl(x_q - R)), cell(fl(x_q + R))] per axis; and x_j <= hi, the data's maximum, so cell(x_j) <= cell(hi):
// clamping the upper end to cell(hi) loses nobody, and a query far outside the cloud does not walk up to 2^21 empty cells per axis.  The
// lower end needs no clamp, cell() is 0 = cell(lo) below lo.  An upper end below the lower end is an empty range.
// A bucket also holds points of other cells, and two cells of one range may share a bucket: a count or a list would then meet a point
// twice.  Every entry carries the key of its own cell and is accepted only in the visit of that cell: each data point of the range is met
// exactly once.  The cells of a range are counted in 64 bits; more cells than entries (r2 = +inf or FLT_MAX, radii far above h): the lane
// walks the entry array itself, [0, entries), where every finite data point stands exactly once and no key is needed.
// Members go to the lane's slot (query_device.h QuerySlot, the slot of the crossing and neighbour queries); while a slot is full and no
// count is asked for, an entry with `d2 > bound` is passed over (bound = the largest d2 kept, non-strictly: an equal-d2 smaller index
// still arrives).  No cell is ever skipped on the bound.
// The header is the device's: the kernel takes m and the bucket mask from it, checks them against each other and against grid_bytes, clamps
// the number of entries to m and every bucket's end to the number of entries -- a workspace that was never built reads as an empty or
// a wrong grid, never as an address outside it.
// k_point_neighbors<.., BRUTE>: every data point in turn for every query, same function, same slot rule (validation).
//
// Plain vector loads and stores only in the query (atomics in the build and in the counted instantiation); no scratch, no LDS.
#include <hip/hip_runtime.h>

#include "point_neighbor_device.h"

namespace cgrt {

namespace {

struct PointGridDev {
    const float* data;
    uint32_t m;
    float cell;
    uint32_t bmask;
    uint32_t* hdr;
    uint32_t* bcount;
    uint32_t* bstart;
    float4* epos;
    unsigned long long* ekey;
};

__global__ __launch_bounds__(256) void k_pgrid_bounds(const PointGridDev A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t klo[3] = {0u, 0u, 0u}, khi[3] = {0u, 0u, 0u};
    if (i == 0u) {
        A.hdr[PG_CELL] = __float_as_uint(A.cell);
        A.hdr[PG_BMASK] = A.bmask;
        A.hdr[PG_M] = A.m;
    }
    if (i < A.m) {
        const float x = A.data[3ull * i], y = A.data[3ull * i + 1], z = A.data[3ull * i + 2];
        if (finite3(x, y, z)) {
            khi[0] = ordered(x), khi[1] = ordered(y), khi[2] = ordered(z);
            klo[0] = ~khi[0], klo[1] = ~khi[1], klo[2] = ~khi[2];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const uint32_t l = wave_max(klo[a]), h = wave_max(khi[a]);
        if (lane_id() == 0u && h != 0u) {
            atomicMax(A.hdr + H_LO + a, l);
            atomicMax(A.hdr + H_HI + a, h);
        }
    }
}

__global__ __launch_bounds__(256) void k_pgrid_count(const PointGridDev A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.m) return;
    const float x = A.data[3ull * i], y = A.data[3ull * i + 1], z = A.data[3ull * i + 2];
    if (!finite3(x, y, z)) return;
    const Grid g = load_grid(A.hdr, A.cell);
    const uint32_t b = bucket(cell(x, g.lo[0], g.h), cell(y, g.lo[1], g.h), cell(z, g.lo[2], g.h), A.bmask);
    if (atomicAdd(A.bcount + b, 1u) == 0u) atomicAdd(A.hdr + PG_USED, 1u);
}

// (takes the counts back down to 0: slot = start + what is left of the count)
__global__ __launch_bounds__(256) void k_pgrid_scatter(const PointGridDev A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.m) return;
    const float x = A.data[3ull * i], y = A.data[3ull * i + 1], z = A.data[3ull * i + 2];
    if (!finite3(x, y, z)) return;
    const Grid g = load_grid(A.hdr, A.cell);
    const uint32_t cx = cell(x, g.lo[0], g.h), cy = cell(y, g.lo[1], g.h), cz = cell(z, g.lo[2], g.h);
    const uint32_t b = bucket(cx, cy, cz, A.bmask);
    const uint32_t slot = A.bstart[b] + atomicSub(A.bcount + b, 1u) - 1u;  // below bstart[B] <= m
    A.epos[slot] = make_float4(x, y, z, __uint_as_float(i));
    A.ekey[slot] = cell_key(cx, cy, cz);
}

template <bool LIST, bool COUNT, bool BRUTE>
__global__ __launch_bounds__(256) void k_point_neighbors(const PointNeighborArgs A, unsigned long long* __restrict__ counters) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const float px = A.points[3 * i], py = A.points[3 * i + 1], pz = A.points[3 * i + 2];
    QuerySlot Q;
    const bool wanted = slot_open<LIST>(Q, A.radius2 ? A.radius2[i] : A.max_dist2, reinterpret_cast<uint32_t*>(A.out), A.offsets, A.k,
                                        A.capacity, A.counts != nullptr, i);
    const uint32_t skip = (A.flags & kSkipSameIndex) ? (uint32_t)i : 0xffffffffu;  // (no data point has index 0xffffffff)
    unsigned long long c_cells = 0, c_read = 0, c_foreign = 0, c_d2 = 0, c_linear = 0;
    PointGridView V;
    const bool built = !BRUTE && grid_view(A.grid, A.grid_bytes, V);
    // a radius that is NaN or below zero and a point that is not finite have no neighbours
    if (wanted && Q.limit >= 0.0f && finite3(px, py, pz))
        point_search<LIST, COUNT, BRUTE>(A, V, built, px, py, pz, skip, Q, c_cells, c_read, c_foreign, c_d2, c_linear);  // (point_neighbor_device.h)
    slot_close<LIST>(Q, A.counts, i);
    if (COUNT) {
        if (c_cells) atomicAdd(counters, c_cells);
        if (c_read) atomicAdd(counters + 1, c_read);
        if (c_foreign) atomicAdd(counters + 2, c_foreign);
        if (c_d2) atomicAdd(counters + 3, c_d2);
        if (c_linear) atomicAdd(counters + 4, c_linear);
        if (i == 0ull && V.used) atomicAdd(counters + 5, (unsigned long long)V.used);
    }
}

template <bool LIST, bool COUNT, bool BRUTE>
hipError_t launch_one(const PointNeighborArgs& A, unsigned long long* counters, hipStream_t stream) {
    const dim3 grid((unsigned)((A.n + 255u) / 256u)), block(256);
    hipLaunchKernelGGL((k_point_neighbors<LIST, COUNT, BRUTE>), grid, block, 0, stream, A, counters);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_point_grid_build(const float* data, uint64_t m, float cell, void* grid, hipStream_t stream) {
    if (m > 0x7fffffffull || !grid || (m && !data) || !(cell > 0.0f) || !(cell <= 3.402823466e+38f)) return hipErrorInvalidValue;
    char* const p0 = reinterpret_cast<char*>(((uintptr_t)grid + 15u) & ~(uintptr_t)15u);
    const PointGridLayout L = point_grid_layout(m);
    const uint32_t B = poisson_buckets(m);
    PointGridDev A{};
    A.data = data;
    A.m = (uint32_t)m;
    A.cell = cell;
    A.bmask = B - 1u;
    A.hdr = reinterpret_cast<uint32_t*>(p0);
    A.bcount = reinterpret_cast<uint32_t*>(p0 + L.bcount);
    A.bstart = reinterpret_cast<uint32_t*>(p0 + L.bstart);
    A.epos = reinterpret_cast<float4*>(p0 + L.epos);
    A.ekey = reinterpret_cast<unsigned long long*>(p0 + L.ekey);
    const hipError_t e = hipMemsetAsync(p0, 0, 64ull + 4ull * B, stream);  // the header and the bucket counts
    if (e != hipSuccess) return e;
    const dim3 block(256), grid_dim((unsigned)(m ? (m + 255u) / 256u : 1u));  // (one block without points: thread 0 fills the header)
    hipLaunchKernelGGL(k_pgrid_bounds, grid_dim, block, 0, stream, A);
    if (m) hipLaunchKernelGGL(k_pgrid_count, grid_dim, block, 0, stream, A);
    launch_bucket_scan(A.bcount, reinterpret_cast<uint32_t*>(p0 + L.sums), A.bstart, B, stream);
    if (m) hipLaunchKernelGGL(k_pgrid_scatter, grid_dim, block, 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_point_neighbors(const PointNeighborArgs& A, bool brute, unsigned long long* counters, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    if (A.n > 0x7fffffffull || A.m > 0x7fffffffull || (!A.out && !A.counts && !counters) || (counters && brute) || (!brute && !A.grid) ||
        (brute && A.m && !A.data))
        return hipErrorInvalidValue;
    if (counters) return A.out ? launch_one<true, true, false>(A, counters, stream) : launch_one<false, true, false>(A, counters, stream);
    if (!A.out) return brute ? launch_one<false, false, true>(A, nullptr, stream) : launch_one<false, false, false>(A, nullptr, stream);
    return brute ? launch_one<true, false, true>(A, nullptr, stream) : launch_one<true, false, false>(A, nullptr, stream);
}

}  // namespace cgrt
