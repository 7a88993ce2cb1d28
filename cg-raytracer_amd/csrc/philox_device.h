// philox_device.h -- Philox4x32-10 (Salmon et al., Random123) for the kernels that draw random words: the surface sampler
// (surface_sample_kernels.hip, words 0..2) and the Poisson-disk order (poisson_kernels.hip, word 3).  include/cgrt.h "Surface sampling"
// states the constants and the known answer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cgrt {

// the four output words for counter {c0, c1, 0, 0} and key {k0, k1}; a caller that ignores a word pays nothing for it
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t& w0, uint32_t& w1, uint32_t& w2,
                                              uint32_t& w3) {
    uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w0 = c0;
    w1 = c1;
    w2 = c2;
    w3 = c3;
}

}  // namespace cgrt
