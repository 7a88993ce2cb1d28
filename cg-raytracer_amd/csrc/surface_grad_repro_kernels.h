// surface_grad_repro_kernels.h -- host-callable launcher of the bitwise-reproducible table adjoint in surface_grad_repro_kernels.hip
// (include/cgrt.h cgrt_interpolate_hits_grad_repro*, cgrt_surface_*_grad_repro_device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surface_kernels.h"

namespace cgrt {

// The per-call workspace of `elements` = nverts x channels table elements: a 64-bit accumulator each, then a 32-bit exponent / flag word
// each (12 bytes per element; the base 8-byte aligned).  Its contents need no initialisation: the launch clears it.
inline uint64_t surface_grad_repro_bytes(uint64_t elements) { return 12ull * elements; }

// S of the definition: min(24, 38 - bitlength(3 n)), so that 3 n terms below 2^(24 + S) sum in int64.
inline uint32_t surface_grad_repro_shift(uint64_t n) {
    uint32_t bits = 0;
    for (uint64_t v = 3ull * n; v; v >>= 1) bits++;
    return bits + 24u > 38u ? 38u - bits : 24u;
}

// The four passes on `stream`: clear, max, add (the launch of SurfaceGradDev A, whose grad_attr neither of them touches), finalise (the
// only pass that reads and writes A.grad_attr).  `workspace`: surface_grad_repro_bytes(elements) bytes of device memory.
hipError_t launch_surface_grad_repro(const SurfaceGradDev& A, int source, uint64_t elements, void* workspace, hipStream_t stream);

}  // namespace cgrt
