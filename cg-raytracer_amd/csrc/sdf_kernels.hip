// sdf_kernels.hip -- signed distance and occupancy (include/cgrt.h cgrt_signed_distance*): for every point the
// square root of cgrt_closest_points' dist2, signed by a majority vote over the parities of cgrt_count_crossings along a few fixed
// directions.  One kernel, one point per lane, nothing in between:
//
// phase 1  the closest-point search of k_closest (closest_device.h closest_search: the same walk, the same arithmetic, the same
//          `lb2 > bound` rule).  Only the bound and the winner's id are read afterwards, so the point and the barycentrics of Best
//          are dead and cost no register; the equal-dist2 tie rule does not change the value.
// phase 2  per direction the count search of k_crossings<false, ..> (crossing_device.h cross_walk), keeping only the parity.  Once more
//          than ndirs / 2 walks agree the others are skipped: the vote is decided.  BRUTE_PARITY and a ray outside the conservative
//          test's envelope test every record, as the crossing entries do.
// Both phases use one lane-interleaved LDS region, sized for the closest stack (two dwords per entry) and reused by the parity walks (one
// dword per entry): a lane only ever touches its own column, so no barrier separates them.  One f32 and / or one byte is stored per point.
// GRID: the lane makes its point from its grid index (SdfPoints; query_device.h brick_index, grid_coord).
#include <hip/hip_runtime.h>

#include "closest_device.h"
#include "crossing_device.h"
#include "sdf_kernels.h"

namespace cgrt {

namespace {

#define CGRT_SDF_BLOCK 128
static_assert(CGRT_SDF_BLOCK == CGRT_CLOSEST_BLOCK && CGRT_SDF_BLOCK == CGRT_CROSS_BLOCK, "the stacks are laid out for 128 lanes");

// the parity of cgrt_count_crossings' count for the ray {o, d, +inf}: an uncounted query without a slot
template <bool COUNT, bool BRUTE_PARITY>
__device__ __forceinline__ uint32_t sdf_parity(const SceneDev& S, const F3 o, const F3 d, uint32_t* const stk, unsigned long long& c_nodes,
                                               unsigned long long& c_tris) {
    QuerySlot Q;
    slot_open<false>(Q, __builtin_inff(), nullptr, nullptr, 0u, 0ull, false, 0ull);
    cross_walk<false, COUNT, BRUTE_PARITY>(S, o, d, stk, Q, c_nodes, c_tris);
    return Q.count & 1u;
}

template <int GRID, bool COUNT, bool BRUTE_PARITY>
__global__ __launch_bounds__(CGRT_SDF_BLOCK) void k_sdf(const SceneDev S, const SdfArgs A, unsigned long long* __restrict__ counters) {
    // phase 1: slot s of lane l of wave w at w * (2 * CLOSEST_STACK_ENTRIES * 64) + s * 64 + l, entry e = slots 2e {ref}, 2e + 1 {lb2};
    // phase 2: entry e of the same lane in slot e
    __shared__ uint32_t s_stk[2 * CLOSEST_STACK_ENTRIES * CGRT_SDF_BLOCK];
    unsigned long long i;  // the result's index, below A.n
    float px, py, pz;
    if (GRID == SDF_LIST) {
        i = (unsigned long long)blockIdx.x * CGRT_SDF_BLOCK + threadIdx.x;
        if (i >= A.n) return;
        px = A.points[3 * i], py = A.points[3 * i + 1], pz = A.points[3 * i + 2];
    } else {
        const uint32_t nx = A.dims[0], ny = A.dims[1], nz = A.dims[2];
        uint32_t ix, iy, iz;
        if (GRID == SDF_GRID_BRICK) {
            if (!brick_index(nx, ny, nz, ix, iy, iz)) return;
        } else {
            const unsigned long long j = (unsigned long long)blockIdx.x * CGRT_SDF_BLOCK + threadIdx.x;
            if (j >= A.n) return;
            const uint32_t row = (uint32_t)(j / nx);
            ix = (uint32_t)(j % nx), iy = row % ny, iz = row / ny;
        }
        i = ((unsigned long long)iz * ny + iy) * nx + ix;
        px = grid_coord(A.origin[0], ix, A.spacing[0]);
        py = grid_coord(A.origin[1], iy, A.spacing[1]);
        pz = grid_coord(A.origin[2], iz, A.spacing[2]);
    }
    uint32_t* const stk = s_stk + (threadIdx.x >> 6) * (2 * CLOSEST_STACK_ENTRIES * 64) + (threadIdx.x & 63u);
    unsigned long long c_cl_nodes = 0, c_cl_tris = 0, c_cr_nodes = 0, c_cr_tris = 0, c_walks = 0;
    float s = __builtin_inff();
    bool inside = false;
    if (S.root_ref != REF_NONE && finite3(px, py, pz)) {
        if (A.want_sdf) {
            Best B;  // (only the bound and whether a triangle qualified are read: the compiler drops the point and the barycentrics)
            B.d2 = A.max_dist2;
            B.prim = REF_NONE;
            B.qx = B.qy = B.qz = B.v = B.w = 0.0f;
            closest_search<COUNT>(S, px, py, pz, stk, B, c_cl_nodes, c_cl_tris);
            if (B.prim != REF_NONE) s = sqrtf(B.d2);  // (IEEE: the Makefile's -fhip-fp32-correctly-rounded-divide-sqrt)
        }
        const uint32_t half = A.ndirs >> 1;
        uint32_t odd = 0u, even = 0u;
        for (uint32_t j = 0; j < A.ndirs && odd <= half && even <= half; j++) {
            const uint32_t par = sdf_parity<COUNT, BRUTE_PARITY>(S, f3(px, py, pz), f3(A.dirs[j][0], A.dirs[j][1], A.dirs[j][2]), stk, c_cr_nodes,
                                                                 c_cr_tris);
            odd += par;
            even += 1u - par;
            if (COUNT) c_walks++;
        }
        inside = odd > half;
    }
    if (A.sdf) A.sdf[i] = inside ? -s : s;
    if (A.inside) A.inside[i] = inside ? 1 : 0;
    if (COUNT) {
        atomicAdd(counters, c_cl_nodes);
        atomicAdd(counters + 1, c_cl_tris);
        atomicAdd(counters + 2, c_cr_nodes);
        atomicAdd(counters + 3, c_cr_tris);
        atomicAdd(counters + 4, c_walks);
    }
}

template <int GRID, bool COUNT>
hipError_t launch_one(const SceneDev& S, const SdfArgs& A, const unsigned blocks, bool brute_parity, unsigned long long* counters,
                      hipStream_t stream) {
    const dim3 grid(blocks), block(CGRT_SDF_BLOCK);
    if (brute_parity)
        hipLaunchKernelGGL((k_sdf<GRID, COUNT, true>), grid, block, 0, stream, S, A, counters);
    else
        hipLaunchKernelGGL((k_sdf<GRID, COUNT, false>), grid, block, 0, stream, S, A, counters);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sdf(const SceneDev& S, const SdfArgs& A, SdfPoints how, bool brute_parity, unsigned long long* counters, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    if (A.n > 0x7fffffffu || (!A.sdf && !A.inside && !counters) || A.ndirs < 1 || A.ndirs > 7 || !(A.ndirs & 1u) || (counters && how != SDF_LIST))
        return hipErrorInvalidValue;
    const unsigned linear = (unsigned)(((uint64_t)A.n + CGRT_SDF_BLOCK - 1) / CGRT_SDF_BLOCK);
    if (how == SDF_LIST) {
        if (!A.points) return hipErrorInvalidValue;
        return counters ? launch_one<SDF_LIST, true>(S, A, linear, brute_parity, counters, stream)
                        : launch_one<SDF_LIST, false>(S, A, linear, brute_parity, nullptr, stream);
    }
    const uint64_t plane = (uint64_t)A.dims[0] * A.dims[1];  // (n fits 31 bits: no product below wraps)
    if (plane == 0 || plane > A.n || plane * A.dims[2] != A.n) return hipErrorInvalidValue;
    if (how == SDF_GRID_LINEAR) return launch_one<SDF_GRID_LINEAR, false>(S, A, linear, brute_parity, nullptr, stream);
    // (at most as many bricks as grid points: the count fits the launch's 32-bit grid)
    const uint64_t bricks = (uint64_t)((A.dims[0] + 7u) >> 3) * ((A.dims[1] + 3u) >> 2) * ((A.dims[2] + 3u) >> 2);
    return launch_one<SDF_GRID_BRICK, false>(S, A, (unsigned)bricks, brute_parity, nullptr, stream);
}

}  // namespace cgrt
