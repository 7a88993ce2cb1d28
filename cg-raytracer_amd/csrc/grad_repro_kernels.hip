// grad_repro_kernels.hip -- the clear and finalise passes of the bitwise-reproducible adjoints (grad_repro_kernels.h; DESIGN.md sections
// 5.28 and 5.36), the same for every form.
//   clear     hipMemsetAsync of the workspace
//   finalise  k_grad_repro_finalise: one lane per output element in a grid-stride loop (at most 2^20 blocks); a touched one gets
//             fl32(fl64(a) + fl64(I) * 2^(E - 150 - S)) (repro_value_sum), or a + s for the kinds (repro_value_kinds), stored plainly; an
//             untouched one is neither read nor written
// 256-thread blocks, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "grad_repro_kernels.h"

namespace cgrt {

namespace {

const unsigned kReproBlock = 256;

__global__ __launch_bounds__(kReproBlock) void k_grad_repro_finalise(const ReproAccum R, float* const grad, const unsigned long long elements) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kReproBlock;
    for (unsigned long long e = (unsigned long long)blockIdx.x * kReproBlock + threadIdx.x; e < elements; e += stride) {
        const uint32_t w = R.word[e];
        if (!w) continue;
        const float a = grad[e];
        grad[e] = repro_canonical((w & REPRO_KINDS) ? repro_value_kinds(a, w) : repro_value_sum(a, w, (long long)R.acc[e], R.shift));
    }
}

}  // namespace

hipError_t repro_begin(void* workspace, uint64_t elements, hipStream_t stream) {
    return hipMemsetAsync(workspace, 0, repro_workspace_bytes(elements), stream);
}

hipError_t repro_finish(const ReproAccum& R, float* grad, uint64_t elements, hipStream_t stream) {
    const unsigned long long blocks = (elements + kReproBlock - 1ull) / kReproBlock;
    const dim3 grid((uint32_t)(blocks < (1ull << 20) ? blocks : (1ull << 20)));
    hipLaunchKernelGGL(k_grad_repro_finalise, grid, dim3(kReproBlock), 0, stream, R, grad, (unsigned long long)elements);
    return hipGetLastError();
}

}  // namespace cgrt
