// grid_field_grad_repro_kernels.hip -- the bitwise-reproducible form of the sampler's adjoint (include/cgrt.h
// cgrt_sample_grid_grad_repro*).  The contributions are those of k_sample_grid_grad (grid_field_kernels.hip):
// field_grad_item of grid_field_device.h, a zero of either sign not a contribution.  What differs is the sum: per grid element the
// contributions are aligned to the element's largest exponent E, turned into integers T with S guard bits and added in int64
// (grad_repro_kernels.h and grad_repro_device.h, shared with the surface form) -- integer addition is associative, so the order the
// hardware picks cannot show in the result.
//
// The workspace holds, per grid element, a 64-bit accumulator and a 32-bit word (grad_repro_kernels.h).  Passes, each on the call's stream:
//   clear     repro_begin
//   max       k_sample_grid_grad_repro<0>: one point per lane; per non-zero contribution one atomicMax(e') into the element's word
//             (global_atomic_umax), or one atomicOr of its kind for a non-finite one (global_atomic_or)
//   add       k_sample_grid_grad_repro<1>: the same eight contributions again, the element's word read, T formed, one
//             atomicAdd(unsigned long long) into the accumulator (global_atomic_add_x2); zero terms and flagged elements add nothing
//   finalise  repro_finish (k_grad_repro_finalise of grad_repro_kernels.hip)
// Lanes of a wave that share a cell are NOT merged before the atomics.  256-thread blocks, no LDS, no scratch (no array is indexed by a
// run-time value: field_corners names the eight corners with constants).
#include <hip/hip_runtime.h>

#include "grad_repro_kernels.h"
#include "grid_field_grad_repro_kernels.h"

namespace cgrt {

namespace {

const unsigned kReproBlock = 256;

// A lane behind n or outside the grid contributes nothing and reads no grad.  Both passes compute the same eight f32 bit patterns: the
// arithmetic is field_grad_item's, nothing contracted.
template <int PASS>
__global__ __launch_bounds__(kReproBlock) void k_sample_grid_grad_repro(const FieldGradCall Q, const ReproAccum R) {
    const uint32_t i = blockIdx.x * kReproBlock + threadIdx.x;
    if (i >= Q.n) return;
    uint64_t at;
    float c[8];
    if (!field_grad_item(Q, i, at, c)) return;
    field_corners(Q.grid, at, [&](const int k, const uint64_t e) {
        if (c[k] != 0.0f) repro_contribute<PASS>(R, e, c[k]);  // a zero of either sign is not a contribution; a NaN is not equal to 0 and is one
    });
}

}  // namespace

hipError_t launch_sample_grid_grad_repro(const FieldGradCall& Q, uint64_t elements, void* workspace, hipStream_t stream) {
    if (!Q.n || !elements) return hipSuccess;
    // Every dim is at least 2, so the eight corners of a point are eight distinct elements: an element receives at most one term per
    // point, and n terms below 2^(24 + S) sum in int64.
    const ReproAccum R = repro_accum(workspace, elements, Q.n);
    hipError_t e = repro_begin(workspace, elements, stream);
    if (e != hipSuccess) return e;
    const dim3 grid((Q.n + kReproBlock - 1) / kReproBlock), block(kReproBlock);
    hipLaunchKernelGGL(k_sample_grid_grad_repro<0>, grid, block, 0, stream, Q, R);
    hipLaunchKernelGGL(k_sample_grid_grad_repro<1>, grid, block, 0, stream, Q, R);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return repro_finish(R, Q.grad_values, elements, stream);
}

}  // namespace cgrt
