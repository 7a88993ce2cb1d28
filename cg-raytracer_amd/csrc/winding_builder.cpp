// winding_builder.cpp -- builds the cluster tree of winding_builder.h: per-cluster sums in double bottom-up (a parent's sums are its
// children's), the centre and the area vector rounded once, then the radius in f32 over the vertices of the records a cluster covers.
#include "winding_builder.h"

#include <algorithm>
#include <cmath>

namespace cgrt {

namespace {
struct Sums {
    double area = 0, ac[3] = {0, 0, 0}, c[3] = {0, 0, 0}, n[3] = {0, 0, 0};
    uint64_t count = 0;
    void add(const Sums& o) {
        area += o.area;
        count += o.count;
        for (int a = 0; a < 3; a++) ac[a] += o.ac[a], c[a] += o.c[a], n[a] += o.n[a];
    }
};
Sums triangle_sums(const TriRecord& T) {
    Sums s;
    double e1[3], e2[3];
    for (int a = 0; a < 3; a++) e1[a] = (double)T.v1[a] - (double)T.v0[a], e2[a] = (double)T.v2[a] - (double)T.v0[a];
    s.n[0] = 0.5 * (e1[1] * e2[2] - e1[2] * e2[1]);
    s.n[1] = 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]);
    s.n[2] = 0.5 * (e1[0] * e2[1] - e1[1] * e2[0]);
    s.area = std::sqrt(s.n[0] * s.n[0] + s.n[1] * s.n[1] + s.n[2] * s.n[2]);
    for (int a = 0; a < 3; a++) {
        s.c[a] = ((double)T.v0[a] + (double)T.v1[a] + (double)T.v2[a]) / 3.0;
        s.ac[a] = s.area * s.c[a];
    }
    s.count = 1;
    return s;
}
// ((dx * dx + dy * dy) + dz * dz) in f32, d = v - c: the kernel's expression for a point at v (no contraction: the Makefile's flags)
inline float dist2_f32(const float* v, const float cx, const float cy, const float cz) {
    const float dx = v[0] - cx, dy = v[1] - cy, dz = v[2] - cz;
    return (dx * dx + dy * dy) + dz * dz;
}
}  // namespace

void build_winding_tree(const TriRecord* recs, uint32_t ntris, WindingTree& out) {
    out.clusters.clear();
    out.level_offsets.clear();
    if (ntris == 0) return;
    uint32_t nlevels = 1;
    while (winding_level_count(ntris, nlevels - 1) > 8u) nlevels++;
    out.level_offsets.resize(nlevels + 1);
    uint32_t total = 0;
    for (uint32_t L = 0; L < nlevels; L++) {
        out.level_offsets[L] = total;
        total += winding_level_count(ntris, L);
    }
    out.level_offsets[nlevels] = total;
    out.clusters.resize(total);
    std::vector<Sums> below, here;
    for (uint32_t L = 0; L < nlevels; L++) {
        const uint32_t count = winding_level_count(ntris, L);
        here.assign(count, Sums());
        for (uint32_t i = 0; i < count; i++) {
            if (L == 0) {
                for (uint32_t k = 8u * i; k < std::min(8u * i + 8u, ntris); k++) here[i].add(triangle_sums(recs[k]));
            } else {
                for (size_t k = 8ull * i; k < std::min<size_t>(8ull * i + 8u, below.size()); k++) here[i].add(below[k]);
            }
            const Sums& s = here[i];
            WindingCluster& C = out.clusters[out.level_offsets[L] + i];
            const bool weighted = s.area > 0.0 && std::isfinite(s.area);
            C.cx = (float)(weighted ? s.ac[0] / s.area : s.c[0] / (double)s.count);
            C.cy = (float)(weighted ? s.ac[1] / s.area : s.c[1] / (double)s.count);
            C.cz = (float)(weighted ? s.ac[2] / s.area : s.c[2] / (double)s.count);
            C.nx = (float)s.n[0];
            C.ny = (float)s.n[1];
            C.nz = (float)s.n[2];
            C.pad = 0.0f;
            // the records the cluster covers: [span * i, min(span * (i + 1), ntris))
            const uint64_t span = 1ull << (WINDING_FANOUT_LOG2 * (L + 1u));
            const uint64_t first = span * i, last = std::min<uint64_t>(span * (i + 1ull), ntris);
            float r2 = 0.0f;
            bool nan = false;
            for (uint64_t k = first; k < last; k++) {
                const TriRecord& T = recs[k];
                for (const float* v : {T.v0, T.v1, T.v2}) {
                    const float q = dist2_f32(v, C.cx, C.cy, C.cz);
                    if (q != q)
                        nan = true;
                    else if (q > r2)
                        r2 = q;
                }
            }
            C.r2 = nan ? NAN : r2;
        }
        below.swap(here);
    }
}

}  // namespace cgrt
