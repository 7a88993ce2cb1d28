// isosurface_kernels.h -- host-callable launcher of the iso-surface kernels in isosurface_kernels.hip (include/cgrt.h cgrt_isosurface*;
// DESIGN.md section 5.31).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "poisson_kernels.h"

namespace cgrt {

const uint64_t kIsoMaxPoints = 1ull << 28;  // 7 vertices and 12 triangles per point stay below 2^32

// The workspace over N grid points, carved in this order from its first 16-byte boundary (hence the 8 bytes of slack behind an 8-byte
// aligned pointer); K = ceil(N / 256) blocks, B = K rounded up to the scan's 1024-entry tile:
//   block vertex counts 4 B | block triangle counts 4 B | block vertex starts 4 (B + 1) | block triangle starts 4 (B + 1) | tile sums
//   4 (B / 1024) | first vertex index per point 4 N | edge mask per point N | triangle count per point N
// Every part is written before it is read: the contents need no initialisation.
struct IsoLayout {
    uint64_t B, vcount, tcount, vstart, tstart, sums, first, emask, ptris, bytes;  // byte offsets from the 16-byte boundary; bytes: the end
};
inline IsoLayout iso_layout(uint64_t N) {
    IsoLayout L;
    const uint64_t K = (N + 255ull) / 256ull;
    L.B = (K + 1023ull) / 1024ull * 1024ull;
    L.vcount = 0;
    L.tcount = L.vcount + 4ull * L.B;
    L.vstart = L.tcount + 4ull * L.B;
    L.tstart = L.vstart + poisson_round16(4ull * (L.B + 1ull));
    L.sums = L.tstart + poisson_round16(4ull * (L.B + 1ull));
    L.first = L.sums + poisson_round16(4ull * (L.B / 1024ull));
    L.emask = L.first + poisson_round16(4ull * N);
    L.ptris = L.emask + poisson_round16(N);
    L.bytes = L.ptris + poisson_round16(N);
    return L;
}
inline uint64_t iso_workspace_bytes(uint64_t N) { return 8ull + iso_layout(N).bytes; }

// One call.  All pointers device memory.  list false: the count alone (verts, tris and the capacities are not looked at).
struct IsoCall {
    const float* values;  // nx ny nz, index (iz ny + iy) nx + ix
    float origin[3], spacing[3];
    uint32_t dims[3];  // each 1..2^24, product <= kIsoMaxPoints
    float iso;
    uint32_t above;  // CGRT_ISO_INSIDE_ABOVE
    bool list;
    float* verts;  // 3 f32 per vertex
    uint64_t vert_capacity;
    uint32_t* tris;  // 3 indices per triangle
    uint64_t tri_capacity;
    unsigned long long* counts2;  // {vertices, triangles}, 8-byte aligned
    void* workspace;              // iso_workspace_bytes(points) bytes, 8-byte aligned
};
// Enqueues the passes on `stream` and reads nothing back.  counters (optional: two u64 {cells that emit, tetrahedra that emit}, zeroed by
// the caller) selects the counting instantiation of the classify pass.
hipError_t launch_isosurface(const IsoCall& Q, unsigned long long* counters, hipStream_t stream);

}  // namespace cgrt
