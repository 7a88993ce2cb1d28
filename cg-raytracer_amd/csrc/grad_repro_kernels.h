// grad_repro_kernels.h -- the accumulator of the bitwise-reproducible adjoints (include/cgrt.h cgrt_*_grad_repro*; DESIGN.md sections 5.28
// and 5.36): the workspace layout, what one contribution does to it in the max and the add pass, and the clear and finalise passes that
// bracket a form's own max and add launches.  Used by surface_grad_repro_kernels.hip and grid_field_grad_repro_kernels.hip; the element
// arithmetic is grad_repro_device.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grad_repro_device.h"

namespace cgrt {

// The per-call workspace of `elements` output elements: a 64-bit accumulator each, then a 32-bit exponent / flag word each (12 bytes per
// element; the base 8-byte aligned).  Its contents need no initialisation: repro_begin clears it.
struct ReproAccum {
    unsigned long long* acc;  // one per element
    uint32_t* word;           // one per element
    uint32_t shift;           // S
};
inline uint64_t repro_workspace_bytes(uint64_t elements) { return 12ull * elements; }
// `terms`: the most terms one element can receive in this call (repro_shift)
inline ReproAccum repro_accum(void* workspace, uint64_t elements, uint64_t terms) {
    unsigned long long* const acc = static_cast<unsigned long long*>(workspace);
    return {acc, reinterpret_cast<uint32_t*>(acc + elements), repro_shift(terms)};
}

#if defined(__HIPCC__)
// Contribution x to element `at`.  PASS 0 (max): its code into the element's word.  PASS 1 (add): its integer term under that word into
// the accumulator; zero terms and flagged elements add nothing.
template <int PASS>
__device__ __forceinline__ void repro_contribute(const ReproAccum& R, const unsigned long long at, const float x) {
    if (PASS == 0) {
        repro_mark(R.word + at, repro_code(x));
    } else {
        const long long T = repro_term(x, R.word[at], R.shift);
        if (T) atomicAdd(R.acc + at, (unsigned long long)T);
    }
}
#endif

// The clear pass (hipMemsetAsync of the workspace) and the finalise pass (k_grad_repro_finalise: the only pass that reads and writes
// `grad`, and only the elements a contribution named), both on `stream`.  A form launches its max and add passes between the two.
hipError_t repro_begin(void* workspace, uint64_t elements, hipStream_t stream);
hipError_t repro_finish(const ReproAccum& R, float* grad, uint64_t elements, hipStream_t stream);

}  // namespace cgrt
