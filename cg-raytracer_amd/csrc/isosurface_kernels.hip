// isosurface_kernels.hip -- iso-surfaces by marching tetrahedra (include/cgrt.h cgrt_isosurface*): the indexed
// triangle mesh of the level `iso` of a scalar grid, vertices ordered by (owner point, edge type), triangles by (cell, tetrahedron, table
// position).  The order is the definition, so every index comes from a scan and nothing is ordered by an atomic.
//
// A block is 256 consecutive grid points in result order; a point owns its seven edges towards +x, +y, +z and the cell whose corner 0 it is.
//   k_iso_classify   per point: the 7-bit mask of owned edges that carry a vertex and the triangle count of its cell (a byte each); thread 0
//                    leaves the block's two totals; block 0 also writes the zero padding of both total arrays up to the scan's tile
//   launch_bucket_scan, twice: the exclusive scans of the block totals (poisson_kernels.hip's three scan kernels through its one helper)
//   k_iso_totals     the two grand totals to the caller's counts2 as u64
//   k_iso_vertices   per point: its first vertex index = the block's start + the in-block scan of the masks' popcounts, recomputed here and
//                    kept (4 bytes per point); its vertices' positions, each under the capacity
//   k_iso_triangles  per cell: its first triangle = the block's start + the in-block scan of the per-point triangle counts; a table vertex
//                    on the edge (lo, hi) of the cell's corners is owned by corner lo, with type hi - lo - 1 (every tetrahedron is a chain
//                    0 < a < b < 7 of corner bit sets, so lo's bits are a subset of hi's): its index is the owner's first index plus the
//                    rank of the type in the owner's mask
// The count form stops after k_iso_totals.  A grid with a dim of 1 has no cell: counts2 = {0, 0} and nothing else runs.
//
// Loads of `values` run along x in every pass (lane = point), so a wave's eight corner loads are eight contiguous runs.  Plain vector loads
// and stores only (atomics in the counted instantiation alone); no scratch; LDS: the four words of the block scan.
#include <hip/hip_runtime.h>

#include "isosurface_kernels.h"
#include "point_grid_device.h"
#include "query_device.h"

namespace cgrt {

namespace {

// a tetrahedron's four cell corners (c = x + 2 y + 4 z), three bits each, position 0 lowest
constexpr uint32_t tet(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 3) | (c << 6) | (d << 9); }
constexpr uint32_t kTets[6] = {tet(0, 1, 3, 7), tet(0, 5, 1, 7), tet(0, 3, 2, 7), tet(0, 2, 6, 7), tet(0, 4, 5, 7), tet(0, 6, 4, 7)};
// include/cgrt.h's table.  A table vertex is a tetrahedron edge: its two corner positions, two bits each; a triangle is three of them;
// a row is up to two triangles and, from bit 24, their number.
constexpr uint32_t E01 = 0u | (1u << 2), E02 = 0u | (2u << 2), E03 = 0u | (3u << 2), E12 = 1u | (2u << 2), E13 = 1u | (3u << 2),
                   E23 = 2u | (3u << 2);
constexpr uint32_t tri(uint32_t a, uint32_t b, uint32_t c) { return a | (b << 4) | (c << 8); }
constexpr uint32_t row1(uint32_t t0) { return t0 | (1u << 24); }
constexpr uint32_t row2(uint32_t t0, uint32_t t1) { return t0 | (t1 << 12) | (2u << 24); }
__constant__ uint32_t kIsoTable[16] = {
    0u,
    row1(tri(E01, E02, E03)),
    row1(tri(E01, E13, E12)),
    row2(tri(E02, E03, E13), tri(E02, E13, E12)),
    row1(tri(E02, E12, E23)),
    row2(tri(E01, E23, E03), tri(E01, E12, E23)),
    row2(tri(E01, E13, E23), tri(E01, E23, E02)),
    row1(tri(E03, E13, E23)),
    row1(tri(E03, E23, E13)),
    row2(tri(E01, E02, E23), tri(E01, E23, E13)),
    row2(tri(E01, E23, E12), tri(E01, E03, E23)),
    row1(tri(E02, E23, E12)),
    row2(tri(E02, E12, E13), tri(E02, E13, E03)),
    row1(tri(E01, E12, E13)),
    row1(tri(E01, E03, E02)),
    0u,
};

struct IsoDev {
    const float* values;
    float origin[3], spacing[3];
    uint32_t nx, ny, nz, nxy, N, K, B;
    float iso;
    uint32_t above;
    uint32_t *vcount, *tcount, *vstart, *tstart, *first;
    uint8_t *emask, *ptris;
    float* verts;
    unsigned long long vcap;
    uint32_t* tris;
    unsigned long long tcap;
    unsigned long long* counts2;
};

__device__ __forceinline__ bool is_finite(const float v) { return fabsf(v) <= 3.402823466e+38f; }
__device__ __forceinline__ bool is_inside(const float v, const float iso, const uint32_t above) { return above ? v > iso : v < iso; }

// the corners of point idx's cell: bit c of `fin` iff corner c is in the grid and finite, bit c of `in` iff it is also inside
__device__ __forceinline__ void corners(const IsoDev& A, const uint32_t idx, uint32_t& fin, uint32_t& in) {
    const uint32_t ix = idx % A.nx, r = idx / A.nx, iy = r % A.ny, iz = r / A.ny;
    const bool hx = ix + 1u < A.nx, hy = iy + 1u < A.ny, hz = iz + 1u < A.nz;
    fin = 0u;
    in = 0u;
#pragma unroll
    for (uint32_t c = 0u; c < 8u; c++) {
        const bool here = (!(c & 1u) || hx) && (!(c & 2u) || hy) && (!(c & 4u) || hz);
        if (!here) continue;
        const float v = A.values[idx + (c & 1u) + ((c >> 1) & 1u) * A.nx + (c >> 2) * A.nxy];
        if (!is_finite(v)) continue;
        fin |= 1u << c;
        if (is_inside(v, A.iso, A.above)) in |= 1u << c;
    }
}
// tetrahedron t of a cell: its table row (0: nothing, a non-finite corner included)
template <int T>
__device__ __forceinline__ uint32_t tet_row(const uint32_t fin, const uint32_t in) {
    constexpr uint32_t P = kTets[T], c0 = P & 7u, c1 = (P >> 3) & 7u, c2 = (P >> 6) & 7u, c3 = (P >> 9) & 7u;
    constexpr uint32_t all = (1u << c0) | (1u << c1) | (1u << c2) | (1u << c3);
    if ((fin & all) != all) return 0u;
    return kIsoTable[((in >> c0) & 1u) | (((in >> c1) & 1u) << 1) | (((in >> c2) & 1u) << 2) | (((in >> c3) & 1u) << 3)];
}

template <bool COUNTED>
__global__ __launch_bounds__(256) void k_iso_classify(const IsoDev A, unsigned long long* counters) {
    __shared__ uint32_t lds[4];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    uint32_t em = 0u, nt = 0u, tets = 0u;
    if (idx < A.N) {
        uint32_t fin, in;
        corners(A, idx, fin, in);
        if (fin & 1u) {
            const uint32_t d = (in & 1u) ? ~in : in;  // the corners on the other side than corner 0
            em = ((fin & d) >> 1) & 0x7fu;
        }
        if ((fin >> 7) & 1u) {
            const uint32_t r[6] = {tet_row<0>(fin, in), tet_row<1>(fin, in), tet_row<2>(fin, in),
                                   tet_row<3>(fin, in), tet_row<4>(fin, in), tet_row<5>(fin, in)};
#pragma unroll
            for (int t = 0; t < 6; t++) {
                nt += r[t] >> 24;
                tets += r[t] ? 1u : 0u;
            }
        }
        A.emask[idx] = (uint8_t)em;
        A.ptris[idx] = (uint8_t)nt;
    }
    // both sums in one word: a block has at most 7 * 256 vertices and 12 * 256 triangles
    uint32_t total;
    (void)block_scan((uint32_t)__popc(em) | (nt << 16), lds, &total);
    if (threadIdx.x == 0u) {
        A.vcount[blockIdx.x] = total & 0xffffu;
        A.tcount[blockIdx.x] = total >> 16;
    }
    if (blockIdx.x == 0u) {
        for (uint32_t k = A.K + threadIdx.x; k < A.B; k += 256u) {
            A.vcount[k] = 0u;
            A.tcount[k] = 0u;
        }
    }
    if (COUNTED) {
        unsigned long long cells = nt ? 1ull : 0ull, t = tets;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            cells += (unsigned long long)__shfl_xor((long long)cells, d);
            t += (unsigned long long)__shfl_xor((long long)t, d);
        }
        if (lane_id() == 0u && t) {
            atomicAdd(counters, cells);
            atomicAdd(counters + 1, t);
        }
    }
}

__global__ void k_iso_totals(const IsoDev A) {
    A.counts2[0] = A.vstart[A.B];
    A.counts2[1] = A.tstart[A.B];
}

__global__ __launch_bounds__(256) void k_iso_vertices(const IsoDev A) {
    __shared__ uint32_t lds[4];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    const uint32_t em = idx < A.N ? A.emask[idx] : 0u;
    uint32_t total;
    const uint32_t f = A.vstart[blockIdx.x] + block_scan((uint32_t)__popc(em), lds, &total);
    if (idx >= A.N) return;
    A.first[idx] = f;
    if (!em) return;
    const uint32_t ix = idx % A.nx, r = idx / A.nx, iy = r % A.ny, iz = r / A.ny;
    const float va = A.values[idx];
    const float ax = grid_coord(A.origin[0], ix, A.spacing[0]), ay = grid_coord(A.origin[1], iy, A.spacing[1]),
                az = grid_coord(A.origin[2], iz, A.spacing[2]);
    const float ex = __fsub_rn(grid_coord(A.origin[0], ix + 1u, A.spacing[0]), ax), ey = __fsub_rn(grid_coord(A.origin[1], iy + 1u, A.spacing[1]), ay),
                ez = __fsub_rn(grid_coord(A.origin[2], iz + 1u, A.spacing[2]), az);
    unsigned long long j = f;
#pragma unroll
    for (uint32_t c = 1u; c < 8u; c++) {
        if (!((em >> (c - 1u)) & 1u)) continue;
        if (j < A.vcap) {
            const float vb = A.values[idx + (c & 1u) + ((c >> 1) & 1u) * A.nx + (c >> 2) * A.nxy];
            float t = __fdiv_rn(__fsub_rn(A.iso, va), __fsub_rn(vb, va));
            if (!(t >= 0.0f)) t = 0.0f;
            if (t > 1.0f) t = 1.0f;
            // (an axis the edge does not move along: pB.c - pA.c is pA.c - pA.c, the definition's own arithmetic)
            float* const p = A.verts + 3ull * j;
            p[0] = __fadd_rn(ax, __fmul_rn(t, (c & 1u) ? ex : __fsub_rn(ax, ax)));
            p[1] = __fadd_rn(ay, __fmul_rn(t, (c & 2u) ? ey : __fsub_rn(ay, ay)));
            p[2] = __fadd_rn(az, __fmul_rn(t, (c & 4u) ? ez : __fsub_rn(az, az)));
        }
        j++;
    }
}

// the index of the vertex on the edge between positions pa and pb (the table's nibble) of tetrahedron P of point idx's cell
__device__ __forceinline__ uint32_t table_vertex(const IsoDev& A, const uint32_t idx, const uint32_t P, const uint32_t nib) {
    const uint32_t ca = (P >> (3u * (nib & 3u))) & 7u, cb = (P >> (3u * (nib >> 2))) & 7u;
    const uint32_t lo = min(ca, cb), hi = max(ca, cb);
    const uint32_t own = idx + (lo & 1u) + ((lo >> 1) & 1u) * A.nx + (lo >> 2) * A.nxy;
    return A.first[own] + (uint32_t)__popc((uint32_t)A.emask[own] & ((1u << (hi - lo - 1u)) - 1u));
}
template <int T>
__device__ __forceinline__ void emit(const IsoDev& A, const uint32_t idx, const uint32_t fin, const uint32_t in, unsigned long long& j) {
    const uint32_t row = tet_row<T>(fin, in);
    const uint32_t n = row >> 24;
    for (uint32_t k = 0u; k < n; k++) {
        if (j < A.tcap) {
            const uint32_t t = (row >> (12u * k)) & 0xfffu;
            uint32_t* const p = A.tris + 3ull * j;
            p[0] = table_vertex(A, idx, kTets[T], t & 15u);
            p[1] = table_vertex(A, idx, kTets[T], (t >> 4) & 15u);
            p[2] = table_vertex(A, idx, kTets[T], t >> 8);
        }
        j++;
    }
}

__global__ __launch_bounds__(256) void k_iso_triangles(const IsoDev A) {
    __shared__ uint32_t lds[4];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    const uint32_t nt = idx < A.N ? A.ptris[idx] : 0u;
    uint32_t total;
    unsigned long long j = A.tstart[blockIdx.x] + block_scan(nt, lds, &total);
    if (!nt || j >= A.tcap) return;
    uint32_t fin, in;
    corners(A, idx, fin, in);
    emit<0>(A, idx, fin, in, j);
    emit<1>(A, idx, fin, in, j);
    emit<2>(A, idx, fin, in, j);
    emit<3>(A, idx, fin, in, j);
    emit<4>(A, idx, fin, in, j);
    emit<5>(A, idx, fin, in, j);
}

}  // namespace

hipError_t launch_isosurface(const IsoCall& Q, unsigned long long* counters, hipStream_t stream) {
    if (!Q.counts2) return hipErrorInvalidValue;
    uint64_t N = 1;
    bool cells = true;
    for (int c = 0; c < 3; c++) {
        if (Q.dims[c] < 1u || Q.dims[c] > (1u << 24)) return hipErrorInvalidValue;
        N *= Q.dims[c];
        if (N > kIsoMaxPoints) return hipErrorInvalidValue;
        cells = cells && Q.dims[c] > 1u;
    }
    if (!cells) return hipMemsetAsync(Q.counts2, 0, 16, stream);
    if (!Q.values || !Q.workspace) return hipErrorInvalidValue;
    const IsoLayout L = iso_layout(N);
    char* const p0 = reinterpret_cast<char*>(((uintptr_t)Q.workspace + 15u) & ~(uintptr_t)15u);
    IsoDev A{};
    A.values = Q.values;
    for (int c = 0; c < 3; c++) {
        A.origin[c] = Q.origin[c];
        A.spacing[c] = Q.spacing[c];
    }
    A.nx = Q.dims[0];
    A.ny = Q.dims[1];
    A.nz = Q.dims[2];
    A.nxy = A.nx * A.ny;  // (below 2^28: the product of all three is)
    A.N = (uint32_t)N;
    A.K = (uint32_t)((N + 255ull) / 256ull);
    A.B = (uint32_t)L.B;
    A.iso = Q.iso;
    A.above = Q.above ? 1u : 0u;
    A.vcount = reinterpret_cast<uint32_t*>(p0 + L.vcount);
    A.tcount = reinterpret_cast<uint32_t*>(p0 + L.tcount);
    A.vstart = reinterpret_cast<uint32_t*>(p0 + L.vstart);
    A.tstart = reinterpret_cast<uint32_t*>(p0 + L.tstart);
    A.first = reinterpret_cast<uint32_t*>(p0 + L.first);
    A.emask = reinterpret_cast<uint8_t*>(p0 + L.emask);
    A.ptris = reinterpret_cast<uint8_t*>(p0 + L.ptris);
    A.verts = Q.verts;
    A.vcap = Q.list ? Q.vert_capacity : 0ull;
    A.tris = Q.tris;
    A.tcap = Q.list ? Q.tri_capacity : 0ull;
    A.counts2 = Q.counts2;
    uint32_t* const sums = reinterpret_cast<uint32_t*>(p0 + L.sums);
    const dim3 grid(A.K), block(256);
    if (counters)
        hipLaunchKernelGGL(k_iso_classify<true>, grid, block, 0, stream, A, counters);
    else
        hipLaunchKernelGGL(k_iso_classify<false>, grid, block, 0, stream, A, counters);
    launch_bucket_scan(A.vcount, sums, A.vstart, A.B, stream);
    launch_bucket_scan(A.tcount, sums, A.tstart, A.B, stream);
    hipLaunchKernelGGL(k_iso_totals, dim3(1), dim3(1), 0, stream, A);
    if (Q.list) {
        hipLaunchKernelGGL(k_iso_vertices, grid, block, 0, stream, A);
        if (A.tcap) hipLaunchKernelGGL(k_iso_triangles, grid, block, 0, stream, A);
    }
    return hipGetLastError();
}

}  // namespace cgrt
