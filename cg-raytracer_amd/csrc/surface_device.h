// surface_device.h -- the row mix the kernels that carry a per-vertex table share (surface_kernels.hip k_surface, surface_sample_kernels.hip
// k_sample_surface; DESIGN.md sections 5.19 and 5.27), and the item decoding of the gradient kernels (DESIGN.md sections 5.23 and 5.28).
// Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgrt_math.h"
#include "surface_kernels.h"
#include "walk_exact.h"

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

// Item i of a gradient launch, decoded as k_surface_grad decodes it (surface_kernels.hip: same lookup, same record loads, same
// hit_weights, hence the same weight bits): an invalid item or a lane behind n keeps zero weights, r0 == SURFACE_NONE and
// key == SURFACE_NONE.  Frames also get the item's view and pixel.  The reproducible kernels (surface_grad_repro_kernels.hip) call it;
// k_surface_grad keeps its own lines: calling this from it reordered its registers and instructions (tried, the device assembly
// compared), and its code object is to stay byte for byte what it was.
template <int SRC>
__device__ __forceinline__ void surface_grad_item(const SurfaceGradDev& A, const unsigned long long i, float& wa, float& wb, float& wg,
                                                  uint32_t& r0, uint32_t& r1, uint32_t& r2, uint32_t& view, uint32_t& q, uint32_t& key) {
    wa = wb = wg = 0.0f;
    r0 = key = SURFACE_NONE;
    r1 = r2 = view = q = 0;
    if (i >= (unsigned long long)A.n) return;
    uint32_t prim;
    float t;
    bool hit = true;
    if (SRC == SURFACE_LIST) {
        const CgrtHitDev h = A.hits[i];
        prim = h.prim_id;
        t = h.t;
        hit = h.hit != 0u;
    } else {
        prim = A.prim[i];
        t = A.depth[i];
        view = (uint32_t)i / A.plane;
        q = (uint32_t)i - view * A.plane;
    }
    if (!hit || prim >= A.ntris) return;
    const uint4 L = *reinterpret_cast<const uint4*>(A.lookup + prim);
    const float4* rec = reinterpret_cast<const float4*>(A.tris + L.x);
    const float4 a = rec[0], b = rec[1], c = rec[2];
    F3 o, d;
    if (SRC == SURFACE_LIST) {
        const float* r = A.rays + 7ull * i;
        o = ld3(r);
        d = ld3(r + 3);
    } else if (SRC == SURFACE_TRACKBALL) {
        const int y = (int)(q / (uint32_t)A.W), x = (int)(q - (uint32_t)y * (uint32_t)A.W);
        primary_ray(static_cast<const CameraDev*>(A.cams)[view], A.W, A.H, x, y, o, d);
    } else {
        const int y = (int)(q / (uint32_t)A.W), x = (int)(q - (uint32_t)y * (uint32_t)A.W);
        primary_ray(static_cast<const RayCameraDev*>(A.cams)[view], x, y, o, d);
    }
    hit_weights(f3(a.x, a.y, a.z), f3(a.w, b.x, b.y), f3(b.z, b.w, c.x), o, d, t, wa, wb, wg);
    r0 = L.y;
    r1 = L.z;
    r2 = L.w;
    key = prim;
}

}  // namespace cgrt
