// surface_sample_builder.h -- the host table of the surface sampler (include/cgrt.h cgrt_sample_surface*): the
// triangles' areas in prim_id order, their running sum and the 32-bit thresholds the kernel searches.  Host code only.
#pragma once
#include <stdint.h>

#include <vector>

#include "cgrt_layout.h"

namespace cgrt {

const uint32_t SAMPLE_NO_PRIM = 0xffffffffu;  // `last` of a scene that is empty for sampling

// Per prim_id < ntris.  areas: area_ref (cgrt_math.h) of the triangle, an f32; what is NaN, infinite or not > 0 counts as 0 (and is stored
// as 0).  The running sum S_i is double, added one triangle after the other in prim_id order -- the order is part of the definition --,
// total = S_{ntris-1}.  thresholds[i] = min(floor((S_i / total) * 2^32), 2^32 - 1), evaluated in double.  last: the largest i with
// areas[i] > 0, SAMPLE_NO_PRIM when there is none (thresholds are all 0 then).
struct SampleTable {
    std::vector<float> areas;
    std::vector<uint32_t> thresholds;
    double total = 0.0;
    uint32_t last = SAMPLE_NO_PRIM;
};

// recs: the scene's ntris records in any order, each carrying its prim_id < ntris (every prim_id exactly once).  False when a record's
// prim_id is out of range.  May throw std::bad_alloc.
bool build_sample_table(const TriRecord* recs, uint32_t ntris, SampleTable& T);

}  // namespace cgrt
