// point_frame_kernels.hip -- point-set frames (include/cgrt.h cgrt_point_frames*): for every query point the
// centroid, the covariance's eigenvalues and a right-handed frame of its k nearest data points within a squared radius -- the local PCA
// behind normals, surface variation and tangent planes.  One kernel does the search and the solve, one query per lane:
//   search   k_point_neighbors<LIST, no counts> word for word (point_neighbor_device.h point_search, the shrinking bound included), into the
//            caller's neighbour array: its bytes are the list call's
//   solve    after slot_close the lane reads its own slot back (its own stores, in program order), gathers data[index] twice -- once for
//            the centroid, once for the covariance -- and runs sym3_eigen.h: at most 8 Jacobi sweeps, the order, the signs
//   store    four 16-byte rows; a query without neighbours stores 64 zero bytes
// The sums run in slot order, sequentially, so the record is a function of the slot and the data alone, and the slot is a function of
// (data, points, bound, flag, k): nothing depends on the grid's cell, the buckets or the launch.  An index that is not below m can only come
// from a grid built on other data; it is never used as an address: the query stores 64 zero bytes.
// No atomics, no LDS, no scratch, no loop whose length depends on data beyond the search's own and the two passes over `used <= k` records.
#include <hip/hip_runtime.h>

#include "point_frame_kernels.h"
#include "point_neighbor_device.h"
#include "sym3_eigen.h"

namespace cgrt {

namespace {

template <bool BRUTE>
__global__ __launch_bounds__(256) void k_point_frames(const PointFrameArgs A) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const float px = A.points[3 * i], py = A.points[3 * i + 1], pz = A.points[3 * i + 2];
    QuerySlot Q;
    const bool wanted = slot_open<true>(Q, A.radius2 ? A.radius2[i] : A.max_dist2, reinterpret_cast<uint32_t*>(A.neighbors), nullptr, A.k,
                                        A.n * A.k, false, i);
    const uint32_t skip = (A.flags & kSkipSameIndex) ? (uint32_t)i : 0xffffffffu;
    const uint32_t m = (uint32_t)A.m;
    unsigned long long w = 0;  // (the counters of a counted search, which this is not)
    PointGridView V;
    const bool built = !BRUTE && grid_view(A.grid, A.grid_bytes, V);
    if (wanted && Q.limit >= 0.0f && finite3(px, py, pz)) point_search<true, false, BRUTE>(A, V, built, px, py, pz, skip, Q, w, w, w, w, w);
    slot_close<true>(Q, nullptr, i);

    // steps 2 and 3 of the definition over the slot's `used` records, in slot order
    const uint32_t used = Q.kept;
    bool ok = used != 0u;
    float rx = 0.0f, ry = 0.0f, rz = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (uint32_t j = 0u; ok && j < used; j++) {
        const uint32_t idx = Q.rec[2 * (size_t)j + 1];
        if (idx >= m) {
            ok = false;
            break;
        }
        const float x = A.data[3ull * idx], y = A.data[3ull * idx + 1], z = A.data[3ull * idx + 2];
        if (j == 0u) rx = x, ry = y, rz = z;
        sx = sx + (x - rx), sy = sy + (y - ry), sz = sz + (z - rz);
    }
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0, r3 = r0;
    if (ok) {
        const float fu = (float)used;
        const float cx = rx + sx / fu, cy = ry + sy / fu, cz = rz + sz / fu;
        float xx = 0.0f, xy = 0.0f, xz = 0.0f, yy = 0.0f, yz = 0.0f, zz = 0.0f;
        for (uint32_t j = 0u; j < used; j++) {
            const uint32_t idx = Q.rec[2 * (size_t)j + 1];  // (below m: the first pass saw it)
            const float ex = A.data[3ull * idx] - cx, ey = A.data[3ull * idx + 1] - cy, ez = A.data[3ull * idx + 2] - cz;
            xx = xx + ex * ex, xy = xy + ex * ey, xz = xz + ex * ez;
            yy = yy + ey * ey, yz = yz + ey * ez, zz = zz + ez * ez;
        }
        const Sym3 S = {xx / fu, xy / fu, xz / fu, yy / fu, yz / fu, zz / fu};
        Sym3Frame F;
        sym3_eigen(S, F);
        float ox = 0.0f, oy = 0.0f, oz = 0.0f;
        if (A.orient) ox = A.orient[3 * i], oy = A.orient[3 * i + 1], oz = A.orient[3 * i + 2];
        sym3_signs(F, A.orient != nullptr, ox, oy, oz);
        r0 = make_float4(sym3_canonical(cx), sym3_canonical(cy), sym3_canonical(cz), __uint_as_float(used));
        r1 = make_float4(sym3_canonical(F.n[0]), sym3_canonical(F.n[1]), sym3_canonical(F.n[2]), sym3_canonical(F.lambda[0]));
        r2 = make_float4(sym3_canonical(F.u[0]), sym3_canonical(F.u[1]), sym3_canonical(F.u[2]), sym3_canonical(F.lambda[1]));
        r3 = make_float4(sym3_canonical(F.v[0]), sym3_canonical(F.v[1]), sym3_canonical(F.v[2]), sym3_canonical(F.lambda[2]));
    }
    CgrtPointFrameDev* const out = A.frames + i;
    out->row[0] = r0;
    out->row[1] = r1;
    out->row[2] = r2;
    out->row[3] = r3;
}

}  // namespace

hipError_t launch_point_frames(const PointFrameArgs& A, bool brute, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    if (A.n > 0x7fffffffull || A.m > 0x7fffffffull || A.k == 0u || !A.points || !A.neighbors || !A.frames || (uintptr_t)A.frames % 16 ||
        (A.m && !A.data) || (!brute && !A.grid))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((A.n + 255u) / 256u)), block(256);
    if (brute)
        hipLaunchKernelGGL(k_point_frames<true>, grid, block, 0, stream, A);
    else
        hipLaunchKernelGGL(k_point_frames<false>, grid, block, 0, stream, A);
    return hipGetLastError();
}

}  // namespace cgrt
