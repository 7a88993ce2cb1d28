// surface_sample_builder.cpp -- builds the table of surface_sample_builder.h: the areas by the reference's own area function, one
// sequential double sum in prim_id order, the thresholds from it.
#include "surface_sample_builder.h"

#include <cmath>

#include "cgrt_math.h"

namespace cgrt {

bool build_sample_table(const TriRecord* recs, uint32_t ntris, SampleTable& T) {
    T.areas.assign(ntris, 0.0f);
    T.thresholds.assign(ntris, 0u);
    T.total = 0.0;
    T.last = SAMPLE_NO_PRIM;
    for (uint32_t k = 0; k < ntris; k++) {
        const TriRecord& R = recs[k];
        if (R.prim_id >= ntris) return false;
        const float a = area_ref(f3(R.v0[0], R.v0[1], R.v0[2]), f3(R.v1[0], R.v1[1], R.v1[2]), f3(R.v2[0], R.v2[1], R.v2[2]));
        T.areas[R.prim_id] = (std::isfinite(a) && a > 0.0f) ? a : 0.0f;
    }
    for (uint32_t i = 0; i < ntris; i++) {  // (sequential on purpose: the order of the additions is the definition's)
        T.total += (double)T.areas[i];
        if (T.areas[i] > 0.0f) T.last = i;
    }
    if (T.last == SAMPLE_NO_PRIM) return true;
    double sum = 0.0;
    for (uint32_t i = 0; i < ntris; i++) {
        sum += (double)T.areas[i];
        const double t = std::floor((sum / T.total) * 4294967296.0);
        T.thresholds[i] = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
    }
    return true;
}

}  // namespace cgrt
