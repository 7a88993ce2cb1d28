// surface_sample_kernels.hip -- area-weighted points on the scene's triangles (include/cgrt.h cgrt_sample_surface*; DESIGN.md section
// 5.27).  Everything that decides a sample is integer arithmetic: the random words, the position on the area axis, the triangle, the
// barycentric weights; the only f32 operations are the three exact conversions of the weights and the mix of the vertices.
//
// One kernel, k_sample_surface<STRATIFIED>.  Lane l of a wave owns sample l of the wave's 64 consecutive samples:
//   * Philox4x32-10 (philox_device.h) of counter {j, 0, 0} under key {seed}: ten rounds of two 32 x 32 -> 64 multiplies (v_mul_lo_u32 +
//     v_mul_hi_u32);
//   * the position word x = w0, or (STRATIFIED) floor((j 2^32 + w0) / strata): the one 64-bit division of the kernel;
//   * prim = the number of thresholds T[0 .. last) that are <= x, by a search of `steps` probes whose trip count is the launch's, so a
//     wave never diverges in it and nothing is indexed dynamically (no stack, no scratch); a probe beyond `last` reads entry last - 1
//     and is not taken.  The table is 4 bytes per triangle and stays in L2;
//   * one SurfaceLookup (16-byte load), the record's four 16-byte quarters (the positions and mesh_id), the folded weights, the mix in
//     the order of cgrt_interpolate_hits, and the record as two 16-byte stores (eight dword stores into a buffer that is only 4-byte
//     aligned);
//   * with a table, the wave's rows by surface_rows (surface_device.h), the store loop of k_surface.
#include <hip/hip_runtime.h>

#include "cgrt_math.h"
#include "philox_device.h"
#include "surface_device.h"
#include "surface_sample_kernels.h"

namespace cgrt {

namespace {

template <bool STRATIFIED>
__global__ __launch_bounds__(256) void k_sample_surface(const SampleArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const bool live = i < (unsigned long long)A.n;
    float wa = 0.0f, wb = 0.0f, wg = 0.0f;
    uint32_t r0 = SURFACE_NONE, r1 = 0, r2 = 0;
    if (live) {
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        uint32_t mesh = 0xffffffffu, prim = 0xffffffffu;
        if (A.last != 0xffffffffu) {
            const unsigned long long j = A.first + i;
            uint32_t w0, w1, w2, w3;  // (w3 is the Poisson-disk order's word, poisson_kernels.hip: unused here)
            philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), (uint32_t)A.seed, (uint32_t)(A.seed >> 32), w0, w1, w2, w3);
            uint32_t x = w0;
            if (STRATIFIED) x = (uint32_t)(((j << 32) | (unsigned long long)w0) / A.strata);  // (j < strata <= 2^32 - 1: below 2^32)
            uint32_t count = 0u;
            for (uint32_t s = A.steps; s-- > 0u;) {  // (steps > 0 only with last > 0)
                const uint32_t probe = count + (1u << s);
                const uint32_t t = A.thresholds[(probe <= A.last ? probe : A.last) - 1u];
                count = (probe <= A.last && t <= x) ? probe : count;
            }
            prim = count;
            uint32_t a = w1 >> 8, b = w2 >> 8;
            if (a + b > 0x1000000u) {
                a = 0x1000000u - a;
                b = 0x1000000u - b;
            }
            const uint32_t c = 0x1000000u - a - b;
            wa = (float)c * 5.9604644775390625e-8f;  // 2^-24: exact
            wb = (float)a * 5.9604644775390625e-8f;
            wg = (float)b * 5.9604644775390625e-8f;
            const uint4 L = *reinterpret_cast<const uint4*>(A.lookup + prim);
            const float4* rec = reinterpret_cast<const float4*>(A.tris + L.x);
            const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];  // v0 | v1 | v2 | .. | {D, prim_id, mesh_id, scan_k}
            px = mix_weights(wa, wb, wg, q0.x, q0.w, q1.z);
            py = mix_weights(wa, wb, wg, q0.y, q1.x, q1.w);
            pz = mix_weights(wa, wb, wg, q0.z, q1.y, q2.x);
            mesh = __float_as_uint(q3.z);
            r0 = L.y;
            r1 = L.z;
            r2 = L.w;
        }
        CgrtSurfaceSampleDev* const o = A.out + i;
        if (((uintptr_t)A.out & 15u) == 0u) {
            reinterpret_cast<float4*>(o)[0] = make_float4(px, py, pz, __uint_as_float(mesh));
            reinterpret_cast<float4*>(o)[1] = make_float4(__uint_as_float(prim), wa, wb, wg);
        } else {
            float* f = reinterpret_cast<float*>(o);
            f[0] = px;
            f[1] = py;
            f[2] = pz;
            f[3] = __uint_as_float(mesh);
            f[4] = __uint_as_float(prim);
            f[5] = wa;
            f[6] = wb;
            f[7] = wg;
        }
    }
    // from here on every lane of the wave takes the same branches: the loop below exchanges values between lanes
    if (A.out_attr) {
        const unsigned long long wbase = i - lane;  // the wave's first sample
        const uint32_t cnt = wbase >= (unsigned long long)A.n ? 0u : ((unsigned long long)A.n - wbase < 64ull ? (uint32_t)((unsigned long long)A.n - wbase) : 64u);
        surface_rows(A.attr, A.out_attr, A.channels, A.vec4, wbase, cnt, lane, wa, wb, wg, r0, r1, r2);
    }
}

}  // namespace

hipError_t launch_sample_surface(const SampleArgs& A, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    if (A.n > 0x7fffffffu) return hipErrorInvalidValue;
    const dim3 grid((A.n + 255u) / 256u), block(256);
    if (A.strata)
        hipLaunchKernelGGL(k_sample_surface<true>, grid, block, 0, stream, A);
    else
        hipLaunchKernelGGL(k_sample_surface<false>, grid, block, 0, stream, A);
    return hipGetLastError();
}

}  // namespace cgrt
