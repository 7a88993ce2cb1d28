// surface_grad_repro_kernels.hip -- the bitwise-reproducible form of the table adjoint (include/cgrt.h cgrt_interpolate_hits_grad_repro*,
// cgrt_surface_*_grad_repro_device).  The contributions are those of k_surface_grad (surface_kernels.hip): item
// decoding and weights through surface_grad_item (surface_device.h), every product x = w * g rounded to f32 on its own.  What differs is
// the sum: per table element the contributions are aligned to the element's largest exponent E, turned into integers T with S guard bits
// and added in int64 -- integer addition is associative, so the order the hardware picks cannot show in the result.
//
// The workspace holds, per table element, a 64-bit accumulator and a 32-bit word: bits 0..7 the largest e' seen (1..254; 0: untouched),
// bits 8..10 the non-finite kinds seen (+inf, -inf, NaN).  Passes, each a launch on the call's stream:
//   clear     hipMemsetAsync of the workspace
//   max       k_surface_grad_repro<SRC, 0>: per contribution one atomicMax(e') into the word (global_atomic_umax), or one atomicOr of its
//             kind for a non-finite one (global_atomic_or).  A word that carries a kind no longer takes part in the max: its element's
//             value is decided by the kinds alone.
//   add       k_surface_grad_repro<SRC, 1>: the same products again, the element's word read, T formed, one
//             atomicAdd(unsigned long long) into the accumulator (global_atomic_add_x2); zero terms and flagged elements add nothing.
//   finalise  k_surface_grad_repro_finalise: one lane per table element; a touched one gets fl32(fl64(a) + fl64(I) * 2^(E - 150 - S)),
//             or a + s for the kinds, stored plainly.
// The two mappings are k_surface_grad's: lanes over the wave's contiguous 64 x C run of grad_out (by_item == 0), or each lane the
// channels of its own item (by_item != 0), there with consecutive lanes of one prim_id combined inside the wave first -- the max pass
// combines codes, the add pass INTEGER terms, never floats.  256-thread blocks, no LDS, no scratch.  The element arithmetic (repro_code,
// repro_join, repro_mark, repro_term, repro_value_*) is grad_repro_device.h's, shared with the grid form (grid_field_grad_repro_kernels.hip).
#include <hip/hip_runtime.h>

#include "grad_repro_device.h"
#include "surface_device.h"
#include "surface_grad_repro_kernels.h"

namespace cgrt {

namespace {

struct SurfaceGradReproDev {
    SurfaceGradDev g;         // grad_attr is not touched by the max and add passes
    unsigned long long* acc;  // one per table element
    uint32_t* word;           // one per table element
    uint32_t shift;           // S
};

template <int PASS>
__device__ __forceinline__ void repro_contribute(const SurfaceGradReproDev& R, const unsigned long long at, const float x) {
    if (PASS == 0) {
        repro_mark(R.word + at, repro_code(x));
    } else {
        const long long T = repro_term(x, R.word[at], R.shift);
        if (T) atomicAdd(R.acc + at, (unsigned long long)T);
    }
}

template <int SRC, int PASS>
__global__ __launch_bounds__(256) void k_surface_grad_repro(const SurfaceGradReproDev R) {
    const SurfaceGradDev& A = R.g;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    float wa, wb, wg;
    uint32_t r0, r1, r2, view, q, key;
    surface_grad_item<SRC>(A, i, wa, wb, wg, r0, r1, r2, view, q, key);
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
            repro_contribute<PASS>(R, (unsigned long long)s0 * C + g, x * v);
            repro_contribute<PASS>(R, (unsigned long long)s1 * C + g, y * v);
            repro_contribute<PASS>(R, (unsigned long long)s2 * C + g, z * v);
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
    const unsigned long long a0 = (unsigned long long)(ok ? r0 : 0u) * C, a1 = (unsigned long long)r1 * C, a2 = (unsigned long long)r2 * C;
    for (uint32_t c = 0; c < C; c++) {
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (ok) {
            const float v = gp[(unsigned long long)c * step];
            x = wa * v;
            y = wb * v;
            z = wg * v;
        }
        if (PASS == 0) {
            uint32_t cx = ok ? repro_code(x) : 0u, cy = ok ? repro_code(y) : 0u, cz = ok ? repro_code(z) : 0u;
            for (uint32_t d = 1; d < lim; d <<= 1) {  // (lim == 1 without combining)
                const uint32_t ox = __shfl_down(cx, d, 64), oy = __shfl_down(cy, d, 64), oz = __shfl_down(cz, d, 64);
                if (take & d) {
                    cx = repro_join(cx, ox);
                    cy = repro_join(cy, oy);
                    cz = repro_join(cz, oz);
                }
            }
            if (ok && head) {
                repro_mark(R.word + a0 + c, cx);
                repro_mark(R.word + a1 + c, cy);
                repro_mark(R.word + a2 + c, cz);
            }
        } else {
            // (every lane of a run names the same three rows, so the lanes of a run align to the same E)
            long long tx = 0, ty = 0, tz = 0;
            if (ok) {
                tx = repro_term(x, R.word[a0 + c], R.shift);
                ty = repro_term(y, R.word[a1 + c], R.shift);
                tz = repro_term(z, R.word[a2 + c], R.shift);
            }
            for (uint32_t d = 1; d < lim; d <<= 1) {
                const long long ox = __shfl_down(tx, d, 64), oy = __shfl_down(ty, d, 64), oz = __shfl_down(tz, d, 64);
                if (take & d) {
                    tx += ox;
                    ty += oy;
                    tz += oz;
                }
            }
            if (ok && head) {
                if (tx) atomicAdd(R.acc + a0 + c, (unsigned long long)tx);
                if (ty) atomicAdd(R.acc + a1 + c, (unsigned long long)ty);
                if (tz) atomicAdd(R.acc + a2 + c, (unsigned long long)tz);
            }
        }
    }
}

// One lane per table element (a grid-stride loop for tables beyond the grid).  An untouched element is neither read nor written.
__global__ __launch_bounds__(256) void k_surface_grad_repro_finalise(const unsigned long long* const acc, const uint32_t* const word,
                                                                     float* const grad_attr, const unsigned long long elements,
                                                                     const uint32_t S) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; e < elements; e += stride) {
        const uint32_t w = word[e];
        if (!w) continue;
        const float a = grad_attr[e];
        float r;
        if (w & REPRO_KINDS) {  // (repro_value_kinds, kept as the lines it was moved from: through the call this kernel takes two more VGPRs)
            const uint32_t k = w & REPRO_KINDS;
            const float s = k == REPRO_POS_INF ? __uint_as_float(0x7f800000u) : (k == REPRO_NEG_INF ? __uint_as_float(0xff800000u) : __uint_as_float(0x7fc00000u));
            r = a + s;
        } else {
            r = repro_value_sum(a, w, (long long)acc[e], S);
        }
        r = repro_canonical(r);
        grad_attr[e] = r;
    }
}

template <int SRC>
void launch_passes(const SurfaceGradReproDev& R, hipStream_t stream) {
    const dim3 grid((R.g.n + 255u) / 256u), block(256);
    hipLaunchKernelGGL((k_surface_grad_repro<SRC, 0>), grid, block, 0, stream, R);
    hipLaunchKernelGGL((k_surface_grad_repro<SRC, 1>), grid, block, 0, stream, R);
}

}  // namespace

hipError_t launch_surface_grad_repro(const SurfaceGradDev& A, int source, uint64_t elements, void* workspace, hipStream_t stream) {
    if (A.n == 0 || elements == 0) return hipSuccess;
    SurfaceGradReproDev R;
    R.g = A;
    R.acc = static_cast<unsigned long long*>(workspace);
    R.word = reinterpret_cast<uint32_t*>(R.acc + elements);
    R.shift = surface_grad_repro_shift(A.n);
    hipError_t e = hipMemsetAsync(workspace, 0, surface_grad_repro_bytes(elements), stream);
    if (e != hipSuccess) return e;
    switch (source) {
        case SURFACE_LIST:
            launch_passes<SURFACE_LIST>(R, stream);
            break;
        case SURFACE_TRACKBALL:
            launch_passes<SURFACE_TRACKBALL>(R, stream);
            break;
        case SURFACE_RAYCAM:
            launch_passes<SURFACE_RAYCAM>(R, stream);
            break;
        default:
            return hipErrorInvalidValue;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const unsigned long long blocks = (elements + 255ull) / 256ull;
    const dim3 grid((uint32_t)(blocks < (1ull << 20) ? blocks : (1ull << 20))), block(256);
    hipLaunchKernelGGL(k_surface_grad_repro_finalise, grid, block, 0, stream, R.acc, R.word, A.grad_attr, (unsigned long long)elements, R.shift);
    return hipGetLastError();
}

}  // namespace cgrt
