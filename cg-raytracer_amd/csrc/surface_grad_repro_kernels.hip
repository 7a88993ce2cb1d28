// surface_grad_repro_kernels.hip -- the bitwise-reproducible form of the table adjoint (include/cgrt.h cgrt_interpolate_hits_grad_repro*,
// cgrt_surface_*_grad_repro_device).  The contributions are those of k_surface_grad (surface_kernels.hip): item
// decoding and weights through surface_grad_item (surface_device.h), every product x = w * g rounded to f32 on its own.  What differs is
// the sum: per table element the contributions are aligned to the element's largest exponent E, turned into integers T with S guard bits
// and added in int64 -- integer addition is associative, so the order the hardware picks cannot show in the result.
//
// The workspace holds, per table element, a 64-bit accumulator and a 32-bit word (grad_repro_kernels.h): bits 0..7 the largest e' seen
// (1..254; 0: untouched), bits 8..10 the non-finite kinds seen (+inf, -inf, NaN).  Passes, each a launch on the call's stream:
//   clear     repro_begin
//   max       k_surface_grad_repro<SRC, 0>: per contribution one atomicMax(e') into the word (global_atomic_umax), or one atomicOr of its
//             kind for a non-finite one (global_atomic_or).  A word that carries a kind no longer takes part in the max: its element's
//             value is decided by the kinds alone.
//   add       k_surface_grad_repro<SRC, 1>: the same products again, the element's word read, T formed, one
//             atomicAdd(unsigned long long) into the accumulator (global_atomic_add_x2); zero terms and flagged elements add nothing.
//   finalise  repro_finish (k_grad_repro_finalise of grad_repro_kernels.hip): one lane per table element; a touched one gets
//             fl32(fl64(a) + fl64(I) * 2^(E - 150 - S)), or a + s for the kinds, stored plainly.
// The two mappings are k_surface_grad's: lanes over the wave's contiguous 64 x C run of grad_out (by_item == 0), or each lane the
// channels of its own item (by_item != 0), there with consecutive lanes of one prim_id combined inside the wave first -- the max pass
// combines codes, the add pass INTEGER terms, never floats.  256-thread blocks, no LDS, no scratch.  The element arithmetic (repro_code,
// repro_join, repro_mark, repro_term) is grad_repro_device.h's and the accumulator (ReproAccum, repro_contribute, the clear and finalise
// passes) grad_repro_kernels.h's, both shared with the grid form (grid_field_grad_repro_kernels.hip).
#include <hip/hip_runtime.h>

#include "grad_repro_kernels.h"
#include "surface_device.h"
#include "surface_grad_repro_kernels.h"

namespace cgrt {

namespace {

template <int SRC, int PASS>
__global__ __launch_bounds__(256) void k_surface_grad_repro(const SurfaceGradDev A, const ReproAccum R) {  // (A.grad_attr is not touched)
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

template <int SRC>
void launch_passes(const SurfaceGradDev& A, const ReproAccum& R, hipStream_t stream) {
    const dim3 grid((A.n + 255u) / 256u), block(256);
    hipLaunchKernelGGL((k_surface_grad_repro<SRC, 0>), grid, block, 0, stream, A, R);
    hipLaunchKernelGGL((k_surface_grad_repro<SRC, 1>), grid, block, 0, stream, A, R);
}

}  // namespace

hipError_t launch_surface_grad_repro(const SurfaceGradDev& A, int source, uint64_t elements, void* workspace, hipStream_t stream) {
    if (A.n == 0 || elements == 0) return hipSuccess;
    // S of the definition: min(24, 38 - bitlength(3 n)), so that 3 n terms below 2^(24 + S) sum in int64.
    const ReproAccum R = repro_accum(workspace, elements, 3ull * A.n);
    hipError_t e = repro_begin(workspace, elements, stream);
    if (e != hipSuccess) return e;
    switch (source) {
        case SURFACE_LIST:
            launch_passes<SURFACE_LIST>(A, R, stream);
            break;
        case SURFACE_TRACKBALL:
            launch_passes<SURFACE_TRACKBALL>(A, R, stream);
            break;
        case SURFACE_RAYCAM:
            launch_passes<SURFACE_RAYCAM>(A, R, stream);
            break;
        default:
            return hipErrorInvalidValue;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return repro_finish(R, A.grad_attr, elements, stream);
}

}  // namespace cgrt
