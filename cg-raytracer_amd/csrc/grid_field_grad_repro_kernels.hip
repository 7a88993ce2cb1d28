// grid_field_grad_repro_kernels.hip -- the bitwise-reproducible form of the sampler's adjoint (include/cgrt.h
// cgrt_sample_grid_grad_repro*).  The contributions are those of k_sample_grid_grad (grid_field_kernels.hip):
// field_cell and field_adjoint of grid_field_device.h, a zero of either sign not a contribution.  What differs is the sum: per grid
// element the contributions are aligned to the element's largest exponent E, turned into integers T with S guard bits and added in
// int64 (grad_repro_device.h, shared with the surface form) -- integer addition is associative, so the order the hardware picks cannot
// show in the result.
//
// The workspace holds, per grid element, a 64-bit accumulator and a 32-bit word (grad_repro_device.h).  Passes, each on the call's stream:
//   clear     hipMemsetAsync of the workspace
//   max       k_sample_grid_grad_repro<0>: one point per lane; per non-zero contribution one atomicMax(e') into the element's word
//             (global_atomic_umax), or one atomicOr of its kind for a non-finite one (global_atomic_or)
//   add       k_sample_grid_grad_repro<1>: the same eight contributions again, the element's word read, T formed, one
//             atomicAdd(unsigned long long) into the accumulator (global_atomic_add_x2); zero terms and flagged elements add nothing
//   finalise  k_sample_grid_grad_repro_finalise: one lane per grid element in a grid-stride loop; a touched one gets repro_value_sum or repro_value_kinds, stored
//             plainly; an untouched one is neither read nor written
// Lanes of a wave that share a cell are NOT merged before the atomics.  256-thread blocks, no LDS, no scratch (no array is indexed by a
// run-time value: the eight corners are written out).
#include <hip/hip_runtime.h>

#include "grid_field_grad_repro_kernels.h"

namespace cgrt {

namespace {

const unsigned kReproBlock = 256;

struct FieldGradReproCall {
    FieldGradCall q;          // grad_values is not touched by the max and add passes
    unsigned long long* acc;  // one per grid element
    uint32_t* word;           // one per grid element
    uint32_t shift;           // S
};

template <int PASS>
__device__ __forceinline__ void field_repro_contribute(const FieldGradReproCall& R, const uint64_t at, const float x) {
    if (x != 0.0f) {  // a zero of either sign is not a contribution; a NaN is not equal to 0 and is one
        if (PASS == 0) {
            repro_mark(R.word + at, repro_code(x));
        } else {
            const long long T = repro_term(x, R.word[at], R.shift);
            if (T) atomicAdd(R.acc + at, (unsigned long long)T);
        }
    }
}

// A lane behind n or outside the grid contributes nothing and reads no grad.  Both passes compute the same eight f32 bit patterns: the
// arithmetic is field_cell's and field_adjoint's, nothing contracted.
template <int PASS>
__global__ __launch_bounds__(kReproBlock) void k_sample_grid_grad_repro(const FieldGradReproCall R) {
    const FieldGradCall& Q = R.q;
    const uint32_t i = blockIdx.x * kReproBlock + threadIdx.x;
    if (i >= Q.n) return;
    const float* p = Q.points + 3ull * i;
    int ic[3];
    float f[3];
    if (!field_cell(Q.grid, p[0], p[1], p[2], Q.clamp != 0u, ic, f)) return;
    const bool has_gv = Q.grad_value != nullptr, has_gg = Q.grad_gradient != nullptr;
    float gv = 0.0f, gg[3] = {0.0f, 0.0f, 0.0f};
    if (has_gv) gv = Q.grad_value[i];
    if (has_gg) {
        const float* g = Q.grad_gradient + 3ull * i;
        gg[0] = g[0], gg[1] = g[1], gg[2] = g[2];
    }
    float c[8];
    field_adjoint(Q.grid.spacing, f, has_gv, gv, has_gg, gg, c);
    const uint64_t sy = Q.grid.nx, sz = (uint64_t)Q.grid.nx * Q.grid.ny;
    const uint64_t at = ((uint64_t)ic[2] * Q.grid.ny + (uint64_t)ic[1]) * Q.grid.nx + (uint64_t)ic[0];
    field_repro_contribute<PASS>(R, at, c[0]);
    field_repro_contribute<PASS>(R, at + 1, c[1]);
    field_repro_contribute<PASS>(R, at + sy, c[2]);
    field_repro_contribute<PASS>(R, at + sy + 1, c[3]);
    field_repro_contribute<PASS>(R, at + sz, c[4]);
    field_repro_contribute<PASS>(R, at + sz + 1, c[5]);
    field_repro_contribute<PASS>(R, at + sz + sy, c[6]);
    field_repro_contribute<PASS>(R, at + sz + sy + 1, c[7]);
}

// One lane per grid element (a grid-stride loop for grids beyond the launch).  An untouched element is neither read nor written.
__global__ __launch_bounds__(kReproBlock) void k_sample_grid_grad_repro_finalise(const unsigned long long* const acc, const uint32_t* const word,
                                                                                 float* const grad_values, const unsigned long long elements,
                                                                                 const uint32_t S) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kReproBlock;
    for (unsigned long long e = (unsigned long long)blockIdx.x * kReproBlock + threadIdx.x; e < elements; e += stride) {
        const uint32_t w = word[e];
        if (!w) continue;
        const float a = grad_values[e];
        float r;
        if (w & REPRO_KINDS)
            r = repro_value_kinds(a, w);
        else
            r = repro_value_sum(a, w, (long long)acc[e], S);
        grad_values[e] = repro_canonical(r);
    }
}

}  // namespace

hipError_t launch_sample_grid_grad_repro(const FieldGradCall& Q, uint64_t elements, void* workspace, hipStream_t stream) {
    if (!Q.n || !elements) return hipSuccess;
    FieldGradReproCall R;
    R.q = Q;
    R.acc = static_cast<unsigned long long*>(workspace);
    R.word = reinterpret_cast<uint32_t*>(R.acc + elements);
    R.shift = field_grad_repro_shift(Q.n);
    hipError_t e = hipMemsetAsync(workspace, 0, field_grad_repro_bytes(elements), stream);
    if (e != hipSuccess) return e;
    const dim3 grid((Q.n + kReproBlock - 1) / kReproBlock), block(kReproBlock);
    hipLaunchKernelGGL(k_sample_grid_grad_repro<0>, grid, block, 0, stream, R);
    hipLaunchKernelGGL(k_sample_grid_grad_repro<1>, grid, block, 0, stream, R);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const unsigned long long blocks = (elements + kReproBlock - 1ull) / kReproBlock;
    const dim3 fgrid((uint32_t)(blocks < (1ull << 20) ? blocks : (1ull << 20)));
    hipLaunchKernelGGL(k_sample_grid_grad_repro_finalise, fgrid, block, 0, stream, R.acc, R.word, Q.grad_values, (unsigned long long)elements, R.shift);
    return hipGetLastError();
}

}  // namespace cgrt
