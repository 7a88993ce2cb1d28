// grid_field_grad_repro_kernels.h -- host-callable launcher of the bitwise-reproducible form of the sampler's adjoint in
// grid_field_grad_repro_kernels.hip (include/cgrt.h cgrt_sample_grid_grad_repro*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grad_repro_device.h"
#include "grid_field_kernels.h"

namespace cgrt {

// The per-call workspace of `elements` = nx ny nz grid elements: a 64-bit accumulator each, then a 32-bit exponent / flag word each
// (12 bytes per element; the base 8-byte aligned).  Its contents need no initialisation: the launch clears it.
inline uint64_t field_grad_repro_bytes(uint64_t elements) { return 12ull * elements; }

// S of the definition: min(24, 38 - bitlength(n)).  Every dim is at least 2, so the eight corners of a point are eight distinct
// elements: an element receives at most one term per point, and n terms below 2^(24 + S) sum in int64.
inline uint32_t field_grad_repro_shift(uint64_t n) { return repro_shift(n); }

// The four passes on `stream`: clear, max, add (neither touches Q.grad_values), finalise (the only pass that reads and writes
// Q.grad_values, and only the elements a contribution named).  `workspace`: field_grad_repro_bytes(elements) bytes of device memory.
hipError_t launch_sample_grid_grad_repro(const FieldGradCall& Q, uint64_t elements, void* workspace, hipStream_t stream);

}  // namespace cgrt
