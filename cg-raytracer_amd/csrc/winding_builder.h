// winding_builder.h -- the cluster tree of the winding-number queries (include/cgrt.h cgrt_winding_numbers*):
// an implicit 8-ary tree over a scene's TriRecords IN RECORD ORDER, built on the host.
//   level 0   cluster i covers records [8 i, min(8 i + 8, ntris))
//   level L   cluster i covers the level-(L - 1) clusters 8 i .. 8 i + 7, i.e. records [8^(L+1) i, min(8^(L+1) (i + 1), ntris))
// so level L has ceil(ntris / 8^(L+1)) clusters; the top level is the first with at most 8 (at most 9 levels for the 2^26 records the
// layout allows; no level at all without triangles).  There are no child pointers: the levels lie one after another in one array,
// level 0 first, and level_offsets[L] is the index of level L's first cluster (level_offsets[nlevels] = the total).
// Record order is what the in-leaf accelerators produce (bvh_builder.cpp permutes a leaf's records into its accelerator's runs), so
// consecutive records are neighbours and a cluster is compact.  With cgrt_set_leaf_accel(0) the order inside a leaf is the reference's
// scan order and the clusters get fat: the answers stay within the same bounds, only the work of the walk grows.
#pragma once
#include <stdint.h>

#include <vector>

#include "cgrt_layout.h"

namespace cgrt {

// One cluster, 32 bytes, 32-byte aligned (two 16-byte loads).
//   c   the area-weighted mean of the centroids of its triangles (area = |(v1 - v0) x (v2 - v0)| / 2); the plain mean of the centroids
//       when the area sum is 0 or not finite.  Evaluated in double, rounded once.
//   n   the sum of its triangles' area vectors (v1 - v0) x (v2 - v0) / 2.  Evaluated in double, rounded once.
//   r2  the largest ((dx * dx + dy * dy) + dz * dz), evaluated in f32 in that association with d = vertex - c (each difference rounded),
//       over every vertex of its records: for every vertex that expression is <= r2, exactly.  NaN when one of them is NaN (such a
//       cluster is never far).
struct alignas(32) WindingCluster {
    float cx, cy, cz, r2;
    float nx, ny, nz, pad;
};
static_assert(sizeof(WindingCluster) == 32, "WindingCluster must be 32 B");

static const uint32_t WINDING_FANOUT_LOG2 = 3;  // 8 children
static const uint32_t WINDING_MAX_LEVELS = 9;   // ceil(26 / 3): 2^26 records

// clusters of level L over ntris records
inline uint32_t winding_level_count(uint32_t ntris, uint32_t level) {
    const uint32_t sh = WINDING_FANOUT_LOG2 * (level + 1u);
    return (uint32_t)(((uint64_t)ntris + (1ull << sh) - 1ull) >> sh);
}

struct WindingTree {
    std::vector<WindingCluster> clusters;
    std::vector<uint32_t> level_offsets;  // nlevels + 1 entries
    uint32_t nlevels() const { return level_offsets.empty() ? 0u : (uint32_t)level_offsets.size() - 1u; }
};

// recs[0 .. ntris) in record order.  May throw std::bad_alloc.
void build_winding_tree(const TriRecord* recs, uint32_t ntris, WindingTree& out);

}  // namespace cgrt
