// grid_field_grad_repro_kernels.h -- host-callable launcher of the bitwise-reproducible form of the sampler's adjoint in
// grid_field_grad_repro_kernels.hip (include/cgrt.h cgrt_sample_grid_grad_repro*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grid_field_kernels.h"

namespace cgrt {

// The four passes on `stream`: clear, max, add (neither touches Q.grad_values), finalise (the only pass that reads and writes
// Q.grad_values, and only the elements a contribution named).  `workspace`: repro_workspace_bytes(elements) bytes of device memory
// (grad_repro_kernels.h), elements = nx ny nz.
hipError_t launch_sample_grid_grad_repro(const FieldGradCall& Q, uint64_t elements, void* workspace, hipStream_t stream);

}  // namespace cgrt
