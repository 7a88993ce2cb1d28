// grid_field_kernels.h -- host-callable launchers of the grid-field kernels in grid_field_kernels.hip (include/cgrt.h "Grid fields";
// DESIGN.md section 5.34).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grid_field_device.h"

namespace cgrt {

const uint64_t kFieldMaxPoints = 0x7fffffffull;  // grid points of one call, and its points or rays

// One sampling call.  All pointers device memory; any of value / gradient / inside may be null.
struct FieldSampleCall {
    GridField grid;
    const float* points;  // n x 3
    uint32_t n;
    uint32_t outside_bits;  // CgrtFieldParams.outside, stored as it is
    uint32_t clamp;         // CGRT_FIELD_CLAMP
    float* value;           // n
    float* gradient;        // n x 3
    uint8_t* inside;        // n
};
// One marching call.  hits: n records of 8 words (CgrtGridHit), null with counters.
struct FieldMarchCall {
    GridField grid;
    MarchRules rules;
    const float* rays;  // n x 7
    uint32_t n;
    uint32_t* hits;
};
// (FieldGradCall, one call of the sampler's adjoint, is grid_field_device.h's: field_grad_item reads it.)
// All enqueue on `stream` and read nothing back.  n == 0: nothing is launched.
hipError_t launch_sample_grid(const FieldSampleCall& Q, hipStream_t stream);
hipError_t launch_sample_grid_grad(const FieldGradCall& Q, hipStream_t stream);
// counters (optional: three u64 {rays that entered the box, main-loop samples, refinement samples}, zeroed by the caller) selects the
// counting instantiation, which writes no record.
hipError_t launch_march_grid(const FieldMarchCall& Q, unsigned long long* counters, hipStream_t stream);

}  // namespace cgrt
