// surface_grad_repro_kernels.h -- host-callable launcher of the bitwise-reproducible table adjoint in surface_grad_repro_kernels.hip
// (include/cgrt.h cgrt_interpolate_hits_grad_repro*, cgrt_surface_*_grad_repro_device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surface_kernels.h"

namespace cgrt {

// The four passes on `stream`: clear, max, add (the launch of SurfaceGradDev A, whose grad_attr neither of them touches), finalise (the
// only pass that reads and writes A.grad_attr).  `workspace`: repro_workspace_bytes(elements) bytes of device memory
// (grad_repro_kernels.h), elements = nverts x channels.
hipError_t launch_surface_grad_repro(const SurfaceGradDev& A, int source, uint64_t elements, void* workspace, hipStream_t stream);

}  // namespace cgrt
