// surface_kernels.hip -- surface attributes of hits (include/cgrt.h cgrt_hit_barycentrics*, cgrt_interpolate_hits*, cgrt_surface_*_device;
// DESIGN.md section 5.19): the three area ratios the reference mixes the vertex normals with (ray_tracing.cpp:94-96), kept, and a
// caller's per-vertex table mixed with them in the order of :97.  Nothing is traced: the hit comes from a ray list's {ray, hit} pair or
// from a frame's depth / prim_id planes and the pixel's regenerated primary ray (walk_exact.h primary_ray).
//
// One kernel, k_surface<source>.  Lane l of a wave owns item l of the wave's 64 consecutive items and evaluates its weights once
// (cgrt_math.h hit_weights: four area_ref, each a double sum and a correctly rounded double sqrt) from one SurfaceLookup (16-byte load)
// and the three positions of the TriRecord (three 16-byte loads).  The stores are then the WAVE's, not the lane's: the 64 items' 64 x C
// outputs are one contiguous run of memory, lane l takes element (or 16-byte channel group) k * 64 + l of it, fetches that item's weights
// and vertex rows from the owning lane (ds_bpermute) and reads attr[row][channel] -- neighbouring lanes read and write neighbouring
// channels, whatever C is.  Channel-major frames (chw) are written plane by plane instead: every lane walks the channels of its own
// pixel, and a wave's store is 64 consecutive pixels of one plane.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "surface_device.h"
#include "surface_kernels.h"
#include "walk_exact.h"

namespace cgrt {

namespace {

template <int SRC>
__global__ __launch_bounds__(256) void k_surface(const SurfaceDev A) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const bool live = i < (unsigned long long)A.n;
    float wa = 0.0f, wb = 0.0f, wg = 0.0f;
    uint32_t r0 = SURFACE_NONE, r1 = 0, r2 = 0;
    uint32_t view = 0, q = 0;
    if (live) {
        uint32_t prim;
        float t;
        bool hit = true;
        if (SRC == SURFACE_LIST) {
            const CgrtHitDev h = A.hits[i];
            prim = h.prim_id;
            t = h.t;
            hit = h.hit != 0u;
        } else {
            prim = A.prim[i];  // (a miss carries CGRT_NO_PRIM: there is no flag plane to read)
            t = A.depth[i];
            view = (uint32_t)i / A.plane;
            q = (uint32_t)i - view * A.plane;
        }
        if (hit && prim < A.ntris) {
            const uint4 L = *reinterpret_cast<const uint4*>(A.lookup + prim);
            const float4* rec = reinterpret_cast<const float4*>(A.tris + L.x);
            const float4 a = rec[0], b = rec[1], c = rec[2];  // v0 | v1 | v2 (the record's first 36 bytes)
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
        }
    }
    // from here on every lane of the wave takes the same branches: the loops below exchange values between lanes
    const unsigned long long wbase = i - lane;  // the wave's first item
    const uint32_t cnt = wbase >= (unsigned long long)A.n ? 0u : ((unsigned long long)A.n - wbase < 64ull ? (uint32_t)((unsigned long long)A.n - wbase) : 64u);
    const uint32_t C = A.channels;
    if (A.chw) {  // frames only: plane by plane, each lane its own pixel
        if (live) {
            if (A.bary) {
                float* p = A.bary + (3ull * view) * A.plane + q;
                p[0] = wa;
                p[A.plane] = wb;
                p[2ull * A.plane] = wg;
            }
            if (A.out) {
                float* p = A.out + ((unsigned long long)C * view) * A.plane + q;
                const bool ok = r0 != SURFACE_NONE;
                const float* a0 = A.attr + (unsigned long long)(ok ? r0 : 0u) * C;
                const float* a1 = A.attr + (unsigned long long)r1 * C;
                const float* a2 = A.attr + (unsigned long long)r2 * C;
                for (uint32_t c = 0; c < C; c++) p[(unsigned long long)c * A.plane] = ok ? mix_weights(wa, wb, wg, a0[c], a1[c], a2[c]) : 0.0f;
            }
        }
        return;
    }
    if (A.bary) {
        float* p = A.bary + 3ull * wbase;
        for (uint32_t k = 0; k < 3u; k++) {
            const uint32_t e = k * 64u + lane, h = e / 3u, c = e - 3u * h;
            const float x = __shfl(wa, (int)h, 64), y = __shfl(wb, (int)h, 64), z = __shfl(wg, (int)h, 64);
            if (h < cnt) p[e] = c == 0u ? x : (c == 1u ? y : z);
        }
    }
    if (A.out) surface_rows(A.attr, A.out, C, A.vec4, wbase, cnt, lane, wa, wb, wg, r0, r1, r2);  // (surface_device.h)
}

// The adjoint of k_surface's mix with respect to the table (include/cgrt.h cgrt_interpolate_hits_grad*, cgrt_surface_*_grad_device;
// DESIGN.md section 5.23): grad_attr[tri[prim][k]][c] += w_k * grad_out[item][c].  Lane l evaluates the weights of item l as k_surface
// does -- same lookup, same record loads, same hit_weights --, an invalid item or a lane behind n keeps zero weights and SURFACE_NONE and
// adds nothing (its grad_out is never read).  Every product is rounded on its own; the adds are atomicAdd(float*, float), one no-return
// global_atomic_add_f32 each, so the order of the additions into one element is not fixed.
//   by_item == 0 (lists and (B, H, W, C) frames): grad_out is read the way k_surface writes out -- lane l takes element k * 64 + l of
//     the wave's contiguous 64 x C run, fetches the owning item's weights and rows (ds_bpermute) and adds into channel g of the three
//     rows: neighbouring lanes add into neighbouring channels.  One dword per lane: an atomic has no 16-byte form, and a lane that took
//     four channels would put its neighbour 16 bytes away.
//   by_item != 0 (small C, and every (B, C, H, W) frame): each lane walks the channels of its own item.  With `combine`, consecutive
//     lanes that carry the same prim_id are summed inside the wave first (a segmented suffix sum over lanes, at most six steps and no
//     more than the wave's longest run needs) and only the first lane of each run adds.
template <int SRC>
__global__ __launch_bounds__(256) void k_surface_grad(const SurfaceGradDev A) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const bool live = i < (unsigned long long)A.n;
    float wa = 0.0f, wb = 0.0f, wg = 0.0f;
    uint32_t r0 = SURFACE_NONE, r1 = 0, r2 = 0;
    uint32_t view = 0, q = 0, key = SURFACE_NONE;
    if (live) {
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
        if (hit && prim < A.ntris) {
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
    }
    // from here on every lane of the wave takes the same branches: the loops below exchange values between lanes
    const uint32_t C = A.channels;
    if (!A.by_item) {
        const unsigned long long wbase = i - lane;  // the wave's first item
        const uint32_t cnt = wbase >= (unsigned long long)A.n ? 0u : ((unsigned long long)A.n - wbase < 64ull ? (uint32_t)((unsigned long long)A.n - wbase) : 64u);
        const float* p = A.grad_out + (unsigned long long)C * wbase;
        const uint32_t total = cnt * C;
        for (uint32_t k = 0; k < total; k += 64u) {
            const uint32_t e = k + lane, hq = e / C, g = e - hq * C;
            const int h = (int)(hq & 63u);  // (lanes behind the last element ask a lane that exists; they add nothing)
            const float x = __shfl(wa, h, 64), y = __shfl(wb, h, 64), z = __shfl(wg, h, 64);
            const uint32_t s0 = __shfl(r0, h, 64), s1 = __shfl(r1, h, 64), s2 = __shfl(r2, h, 64);
            if (e >= total || s0 == SURFACE_NONE) continue;
            const float v = p[e];
            atomicAdd(A.grad_attr + ((unsigned long long)s0 * C + g), x * v);
            atomicAdd(A.grad_attr + ((unsigned long long)s1 * C + g), y * v);
            atomicAdd(A.grad_attr + ((unsigned long long)s2 * C + g), z * v);
        }
        return;
    }
    const bool ok = r0 != SURFACE_NONE;
    bool head = true;
    uint32_t take = 0, lim = 1;  // take: bit s set = this lane's run reaches lane + 2^s; lim: the first power of two no lane of the wave takes
    if (A.combine) {
        const uint32_t before = __shfl_up(key, 1u, 64);
        head = lane == 0u || before != key;
        const unsigned long long heads = __ballot(head);
        const uint32_t run = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));  // the first lane of this lane's run
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t other = __shfl_down(run, d, 64);
            const bool same = lane + d < 64u && other == run;
            if (same) take |= d;
            if (__ballot(same)) lim = d << 1;
        }
    }
    const float* gp;
    unsigned long long step;
    if (A.chw) {
        gp = A.grad_out + ((unsigned long long)C * view) * A.plane + q;
        step = A.plane;
    } else {
        gp = A.grad_out + (unsigned long long)C * i;
        step = 1;
    }
    float* const a0 = A.grad_attr + (unsigned long long)(ok ? r0 : 0u) * C;
    float* const a1 = A.grad_attr + (unsigned long long)r1 * C;
    float* const a2 = A.grad_attr + (unsigned long long)r2 * C;
    for (uint32_t c = 0; c < C; c++) {
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (ok) {
            const float v = gp[(unsigned long long)c * step];
            x = wa * v;
            y = wb * v;
            z = wg * v;
        }
        for (uint32_t d = 1; d < lim; d <<= 1) {  // (lim == 1 without combining)
            const float ox = __shfl_down(x, d, 64), oy = __shfl_down(y, d, 64), oz = __shfl_down(z, d, 64);
            if (take & d) {
                x += ox;
                y += oy;
                z += oz;
            }
        }
        if (ok && head) {
            atomicAdd(a0 + c, x);
            atomicAdd(a1 + c, y);
            atomicAdd(a2 + c, z);
        }
    }
}

}  // namespace

// One policy (measured: DESIGN.md section 5.23, profiles/surface_grad_measure.json).
const uint32_t kSurfaceGradItemBelow = 32;  // lists and (B, H, W, C) frames with fewer channels go lane = item
void surface_grad_policy(uint32_t channels, int chw, int* by_item, int* combine) {
    *by_item = chw || channels < kSurfaceGradItemBelow;
    *combine = 1;
    if (const char* e = getenv("CGRT_SURFACE_GRAD_MAP")) {  // experiment knob (tools/measure_surface_grad.py): element / item / item_plain
        if (!strcmp(e, "element")) *by_item = chw != 0;
        if (!strcmp(e, "item") || !strcmp(e, "item_plain")) *by_item = 1;
        if (!strcmp(e, "item_plain")) *combine = 0;
    }
}

hipError_t launch_surface_grad(const SurfaceGradDev& A, int source, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    const dim3 grid((A.n + 255u) / 256u), block(256);
    switch (source) {
        case SURFACE_LIST:
            hipLaunchKernelGGL(k_surface_grad<SURFACE_LIST>, grid, block, 0, stream, A);
            break;
        case SURFACE_TRACKBALL:
            hipLaunchKernelGGL(k_surface_grad<SURFACE_TRACKBALL>, grid, block, 0, stream, A);
            break;
        case SURFACE_RAYCAM:
            hipLaunchKernelGGL(k_surface_grad<SURFACE_RAYCAM>, grid, block, 0, stream, A);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_surface(const SurfaceDev& A, int source, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    const dim3 grid((A.n + 255u) / 256u), block(256);
    switch (source) {
        case SURFACE_LIST:
            hipLaunchKernelGGL(k_surface<SURFACE_LIST>, grid, block, 0, stream, A);
            break;
        case SURFACE_TRACKBALL:
            hipLaunchKernelGGL(k_surface<SURFACE_TRACKBALL>, grid, block, 0, stream, A);
            break;
        case SURFACE_RAYCAM:
            hipLaunchKernelGGL(k_surface<SURFACE_RAYCAM>, grid, block, 0, stream, A);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace cgrt
