// grad_repro_device.h -- the element arithmetic of the bitwise-reproducible adjoints (include/cgrt.h cgrt_*_grad_repro*; DESIGN.md sections
// 5.28 and 5.36): what a contribution brings to its element's word, how two words join, the integer term of a contribution under the
// element's largest exponent, and the element's new value.  Shared by the accumulator (grad_repro_kernels.h, which both forms' kernels use)
// and the stand-alone checker (tools/grid_field_grad_repro_check.cpp, a C++ compiler that is not hipcc): the pure parts are written
// __host__ __device__, as grid_field_device.h and sym3_eigen.h are; repro_mark, which is two atomics, exists for hipcc alone.
// The word of an element: bits 0..7 the largest e' seen (1..254; 0: untouched), bits 8..10 the non-finite kinds seen (+inf, -inf, NaN).
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef CGRT_HD
#if defined(__HIPCC__)
#define CGRT_HD __host__ __device__ __forceinline__
#else
#define CGRT_HD inline
#endif
#endif

namespace cgrt {

const uint32_t REPRO_EXP = 0xffu;       // the word's exponent field
const uint32_t REPRO_POS_INF = 0x100u;  // kinds
const uint32_t REPRO_NEG_INF = 0x200u;
const uint32_t REPRO_NAN = 0x400u;
const uint32_t REPRO_KINDS = 0x700u;

// the bits of a float and back, and the double of a bit pattern: the device intrinsics under hipcc's device pass, memcpy elsewhere
CGRT_HD uint32_t repro_float_bits(const float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
#endif
}
CGRT_HD float repro_bits_float(const uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float x;
    memcpy(&x, &u, 4);
    return x;
#endif
}
CGRT_HD double repro_bits_double(const long long u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double(u);
#else
    double x;
    memcpy(&x, &u, 8);
    return x;
#endif
}

// S of a call whose elements receive at most `terms` terms each: min(24, 38 - bitlength(terms)), so that `terms` integers below
// 2^(24 + S) sum in int64.  (The surface form passes 3 n, the grid form n.)
CGRT_HD uint32_t repro_shift(const uint64_t terms) {
    uint32_t bits = 0;
    for (uint64_t v = terms; v; v >>= 1) bits++;
    return bits + 24u > 38u ? 38u - bits : 24u;
}

// What a contribution x brings to its element's word: e' = max(exponent field, 1) if it is finite, else its kind.
CGRT_HD uint32_t repro_code(const float x) {
    const uint32_t b = repro_float_bits(x), ef = (b >> 23) & 0xffu;
    if (ef == 0xffu) return (b & 0x7fffffu) ? REPRO_NAN : ((b >> 31) ? REPRO_NEG_INF : REPRO_POS_INF);
    return ef ? ef : 1u;
}
CGRT_HD uint32_t repro_join(const uint32_t a, const uint32_t b) {
    const uint32_t ea = a & REPRO_EXP, eb = b & REPRO_EXP;
    return ((a | b) & REPRO_KINDS) | (ea > eb ? ea : eb);
}
#if defined(__HIPCC__)
__device__ __forceinline__ void repro_mark(uint32_t* const w, const uint32_t code) {
    if (code & REPRO_KINDS) atomicOr(w, code & REPRO_KINDS);
    if (code & REPRO_EXP) atomicMax(w, code & REPRO_EXP);
}
#endif
// The integer term of a finite x under the element's word (E in its low byte) with S guard bits; 0 if the element carries a kind.
CGRT_HD long long repro_term(const float x, const uint32_t word, const uint32_t S) {
    const uint32_t b = repro_float_bits(x), ef = (b >> 23) & 0xffu;
    if (ef == 0xffu || (word & REPRO_KINDS)) return 0;
    const uint32_t e = ef ? ef : 1u, M = (b & 0x7fffffu) | (ef ? 0x800000u : 0u);
    const uint32_t d = (word & REPRO_EXP) - e;  // >= 0: the max pass saw this very x
    long long T;
    if (d <= S)
        T = (long long)((unsigned long long)M << (S - d));
    else
        T = d - S >= 24u ? 0 : (long long)(M >> (d - S));
    return (b >> 31) ? -T : T;
}
// The new value of a touched element (w != 0) with previous content a, in the three pieces of the finalise pass (which reads the integer
// sum of an element only where no kind is flagged).  An element that carries a kind: a + s.
CGRT_HD float repro_value_kinds(const float a, const uint32_t w) {
    const uint32_t k = w & REPRO_KINDS;
    const float s = k == REPRO_POS_INF ? repro_bits_float(0x7f800000u) : (k == REPRO_NEG_INF ? repro_bits_float(0xff800000u) : repro_bits_float(0x7fc00000u));
    return a + s;
}
// An element without a kind, with integer sum I: fl32(fl64(a) + fl64(I) * 2^(E - 150 - S)).
CGRT_HD float repro_value_sum(const float a, const uint32_t w, const long long I, const uint32_t S) {
    // 2^(E - 150 - S): E in 1..254, S in 5..24, |I| < 2^62 -- the product stays a normal double, so the scaling is exact
    const double scale = repro_bits_double((long long)(1023u + (w & REPRO_EXP) - 150u - S) << 52);
    return (float)((double)a + (double)I * scale);
}
CGRT_HD float repro_canonical(const float r) { return r != r ? repro_bits_float(0x7fc00000u) : r; }  // every NaN result is this one quiet NaN

}  // namespace cgrt
