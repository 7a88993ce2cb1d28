// grid_field_kernels.hip -- grid fields (include/cgrt.h "Grid fields"): what a scalar grid is at a point, with its
// gradient, and where a ray first reaches a level of it.  The arithmetic is grid_field_device.h's, shared with the stand-alone checker.
//   k_sample_grid        one point per lane: the sample, stored to whichever of value / gradient / inside the caller gave
//   k_march_grid<COUNT>  one ray per lane: the bounded march and its bisection; COUNT adds the lane's three work figures to the
//                        counters and writes no record
//   k_sample_grid_grad   one point per lane: the sampler's adjoint -- field_grad_item (the forward's cell, eight
//                        contributions), up to eight no-return float atomic adds into the values' gradient; a zero contribution is not added
// A sample is eight gathers at one 64-bit element offset, issued together ahead of the first use; a lane's next offset depends on the
// value it just read, so a march is a chain of dependent round trips and its throughput comes from the waves in flight, not from a lane.
// Neighbouring rays walk neighbouring cells: the x-adjacent corner pairs share lines.  Plain vector loads and stores only (atomics in the
// counting instantiation and in the adjoint alone); no LDS; no scratch (no array is indexed by a run-time value).
#include <hip/hip_runtime.h>

#include "grid_field_kernels.h"

namespace cgrt {

namespace {

const unsigned kFieldBlock = 256;

__global__ __launch_bounds__(kFieldBlock) void k_sample_grid(const FieldSampleCall Q) {
    const uint32_t i = blockIdx.x * kFieldBlock + threadIdx.x;
    if (i >= Q.n) return;
    const float* p = Q.points + 3ull * i;
    float v, g[3];
    const bool in = field_sample<true>(Q.grid, p[0], p[1], p[2], Q.clamp != 0u, v, g);
    if (Q.value) reinterpret_cast<uint32_t*>(Q.value)[i] = in ? field_bits(v) : Q.outside_bits;
    if (Q.gradient) {
        uint32_t* o = reinterpret_cast<uint32_t*>(Q.gradient) + 3ull * i;
        o[0] = in ? field_bits(g[0]) : 0u;
        o[1] = in ? field_bits(g[1]) : 0u;
        o[2] = in ? field_bits(g[2]) : 0u;
    }
    if (Q.inside) Q.inside[i] = in ? 1 : 0;
}

// A lane behind n or outside the grid adds nothing and reads no grad.  The adds of one lane are scattered over four rows of the grid; only
// the two x-neighbours of a row are adjacent.  `c != 0` is false for a zero of either sign and true for a NaN, which is added.
__global__ __launch_bounds__(kFieldBlock) void k_sample_grid_grad(const FieldGradCall Q) {
    const uint32_t i = blockIdx.x * kFieldBlock + threadIdx.x;
    if (i >= Q.n) return;
    uint64_t at;
    float c[8];
    if (!field_grad_item(Q, i, at, c)) return;
    field_corners(Q.grid, at, [&](const int k, const uint64_t e) {
        if (c[k] != 0.0f) atomicAdd(Q.grad_values + e, c[k]);
    });
}

template <bool COUNT>
__global__ __launch_bounds__(kFieldBlock) void k_march_grid(const FieldMarchCall Q, unsigned long long* __restrict__ counters) {
    const uint32_t i = blockIdx.x * kFieldBlock + threadIdx.x;
    if (i >= Q.n) return;
    const float* r = Q.rays + 7ull * i;
    const float ray[7] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
    MarchResult R;
    uint32_t work[3];
    field_march<COUNT>(Q.grid, Q.rules, ray, R, work);
    if (COUNT) {
        if (work[0]) atomicAdd(counters, (unsigned long long)work[0]);
        if (work[1]) atomicAdd(counters + 1, (unsigned long long)work[1]);
        if (work[2]) atomicAdd(counters + 2, (unsigned long long)work[2]);
    } else {
        uint32_t* o = Q.hits + 8ull * i;
        o[0] = field_bits(R.t);
        o[1] = field_bits(R.value);
        o[2] = R.steps;
        o[3] = R.status;
        o[4] = field_bits(R.gradient[0]);
        o[5] = field_bits(R.gradient[1]);
        o[6] = field_bits(R.gradient[2]);
        o[7] = 0u;
    }
}

}  // namespace

hipError_t launch_sample_grid(const FieldSampleCall& Q, hipStream_t stream) {
    if (!Q.n) return hipSuccess;
    hipLaunchKernelGGL(k_sample_grid, dim3((Q.n + kFieldBlock - 1) / kFieldBlock), dim3(kFieldBlock), 0, stream, Q);
    return hipGetLastError();
}

hipError_t launch_sample_grid_grad(const FieldGradCall& Q, hipStream_t stream) {
    if (!Q.n) return hipSuccess;
    hipLaunchKernelGGL(k_sample_grid_grad, dim3((Q.n + kFieldBlock - 1) / kFieldBlock), dim3(kFieldBlock), 0, stream, Q);
    return hipGetLastError();
}

hipError_t launch_march_grid(const FieldMarchCall& Q, unsigned long long* counters, hipStream_t stream) {
    if (!Q.n) return hipSuccess;
    const dim3 grid((Q.n + kFieldBlock - 1) / kFieldBlock), block(kFieldBlock);
    if (counters)
        hipLaunchKernelGGL(k_march_grid<true>, grid, block, 0, stream, Q, counters);
    else
        hipLaunchKernelGGL(k_march_grid<false>, grid, block, 0, stream, Q, counters);
    return hipGetLastError();
}

}  // namespace cgrt
