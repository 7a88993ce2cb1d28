// surface_device.h -- the row mix the kernels that carry a per-vertex table share (surface_kernels.hip k_surface, surface_sample_kernels.hip
// k_sample_surface; DESIGN.md sections 5.19 and 5.27).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgrt_math.h"

namespace cgrt {

const uint32_t SURFACE_NONE = 0xffffffffu;  // in place of the first vertex row: the item gets zeros (miss, sphere, prim_id out of range)

// The wave's stores of its `cnt` items' rows (item-major output, C channels each): the 64 items' 64 x C outputs are one contiguous run of
// memory starting at out + C * wbase, lane l takes element (or, with vec4, 16-byte channel group) k * 64 + l of it, fetches that item's
// weights {wa, wb, wg} and vertex rows {r0, r1, r2} from the owning lane (ds_bpermute) and reads attr[row][channel] -- neighbouring lanes
// read and write neighbouring channels, whatever C is.  Every lane of the wave must call it, with the same attr, out, C, vec4, wbase, cnt.
__device__ __forceinline__ void surface_rows(const float* const attr, float* const out, const uint32_t C, const int vec4,
                                             const unsigned long long wbase, const uint32_t cnt, const uint32_t lane, const float wa,
                                             const float wb, const float wg, const uint32_t r0, const uint32_t r1, const uint32_t r2) {
    float* p = out + (unsigned long long)C * wbase;
    const uint32_t G = vec4 ? C >> 2 : C;  // channel groups per item
    const uint32_t total = cnt * G;
    for (uint32_t k = 0; k < total; k += 64u) {
        const uint32_t e = k + lane, hq = e / G, g = e - hq * G;
        const int h = (int)(hq & 63u);  // (lanes behind the last element ask a lane that exists; they store nothing)
        const float x = __shfl(wa, h, 64), y = __shfl(wb, h, 64), z = __shfl(wg, h, 64);
        const uint32_t s0 = __shfl(r0, h, 64), s1 = __shfl(r1, h, 64), s2 = __shfl(r2, h, 64);
        if (e >= total) continue;
        if (vec4) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s0 != SURFACE_NONE) {
                const float4 a0 = reinterpret_cast<const float4*>(attr + (unsigned long long)s0 * C)[g];
                const float4 a1 = reinterpret_cast<const float4*>(attr + (unsigned long long)s1 * C)[g];
                const float4 a2 = reinterpret_cast<const float4*>(attr + (unsigned long long)s2 * C)[g];
                v = make_float4(mix_weights(x, y, z, a0.x, a1.x, a2.x), mix_weights(x, y, z, a0.y, a1.y, a2.y),
                                mix_weights(x, y, z, a0.z, a1.z, a2.z), mix_weights(x, y, z, a0.w, a1.w, a2.w));
            }
            reinterpret_cast<float4*>(p)[e] = v;
        } else {
            float v = 0.0f;
            if (s0 != SURFACE_NONE)
                v = mix_weights(x, y, z, attr[(unsigned long long)s0 * C + g], attr[(unsigned long long)s1 * C + g],
                                attr[(unsigned long long)s2 * C + g]);
            p[e] = v;
        }
    }
}

}  // namespace cgrt
