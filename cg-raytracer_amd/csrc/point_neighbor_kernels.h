// point_neighbor_kernels.h -- host-callable launchers of the point-set neighbour kernels in point_neighbor_kernels.hip (include/cgrt.h
// cgrt_point_grid_*, cgrt_count_point_neighbors*, cgrt_list_point_neighbors*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poisson_kernels.h"

namespace cgrt {

// include/cgrt.h CgrtPointNeighbor, as the device writes it (two dwords; the caller's buffer is only 4-byte aligned)
struct CgrtPointNeighborDev {
    float dist2;
    uint32_t index;
};
static_assert(sizeof(CgrtPointNeighborDev) == 8, "CgrtPointNeighborDev must be 8 B");

// The grid over m points, in caller-owned memory: carved in this order from its first 16-byte boundary (hence the 8 bytes of slack behind
// an 8-byte aligned pointer), B = poisson_buckets(m) buckets:
//   header 64 | bucket counts 4 B (the build's; all 0 again when it ends) | bucket starts 4 (B + 1) | tile sums 4 (B / 1024) (the build's)
//   | entries {x, y, z, index} 16 m | the entries' cell keys 8 m
// The build writes every part it or a query reads: the contents need no initialisation.  Header words: 0..2 and 3..5 the bounds of the
// finite points (point_grid_device.h H_LO, H_HI), then the words below; the number of entries (finite points) is bstart[B].
enum : uint32_t { PG_CELL = 6 /* the caller's cell edge, f32 bits */, PG_BMASK = 7 /* B - 1 */, PG_M = 8, PG_USED = 9 /* buckets in use */ };
struct PointGridLayout {
    uint64_t bcount, bstart, sums, epos, ekey, bytes;  // byte offsets from the 16-byte boundary; bytes: the end
};
__host__ __device__ inline PointGridLayout point_grid_layout(uint64_t m) {
    const uint64_t B = poisson_buckets(m);
    PointGridLayout L;
    L.bcount = 64ull;
    L.bstart = L.bcount + 4ull * B;
    L.sums = L.bstart + poisson_round16(4ull * (B + 1ull));
    L.epos = L.sums + poisson_round16(4ull * (B / 1024ull));
    L.ekey = L.epos + 16ull * m;
    L.bytes = L.ekey + 8ull * m;
    return L;
}
inline uint64_t point_grid_bytes(uint64_t m) { return 8ull + point_grid_layout(m).bytes; }

// Enqueues the build of the grid over data (m x 3 f32, device memory; m <= 0x7fffffff) into grid (point_grid_bytes(m) bytes, 8-byte
// aligned) on `stream`: bounds, count, scan, scatter.  Reads nothing back.  cell: finite and > 0.
hipError_t launch_point_grid_build(const float* data, uint64_t m, float cell, void* grid, hipStream_t stream);

// One query call's buffers, all device memory.  points: n x 3 f32 (n <= 0x7fffffff).  Query i is bounded by radius2[i], or by max_dist2
// where radius2 == nullptr.  out == nullptr: count mode, only counts is written.  Otherwise the slots are neighbor_kernels.h's.
// grid, grid_bytes: what the build filled -- the kernel reads every parameter from its header and takes a header that does not fit
// grid_bytes for an empty grid; or (brute) data, m: the cloud itself, every point tested in turn.
struct PointNeighborArgs {
    const void* grid;
    uint64_t grid_bytes;
    const float* data;
    uint64_t m;
    const float* points;
    const float* radius2;
    float max_dist2;
    uint32_t flags;
    uint64_t n;
    const unsigned long long* offsets;
    uint32_t k;
    CgrtPointNeighborDev* out;
    uint64_t capacity;
    uint32_t* counts;
};
// counters (optional, grid search only: six u64 {cells visited, entries read, entries of another cell skipped, d2 evaluations, queries
// that took the linear walk, buckets in use}, zeroed by the caller) selects the counting instantiation.
hipError_t launch_point_neighbors(const PointNeighborArgs& A, bool brute, unsigned long long* counters, hipStream_t stream);

}  // namespace cgrt
