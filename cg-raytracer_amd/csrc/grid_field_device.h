// grid_field_device.h -- include/cgrt.h "Grid fields" (DESIGN.md section 5.34): the trilinear sample of a scalar grid with its gradient,
// and the march of one ray to a level of it.  f32 throughout, every operation rounded on its own (-ffp-contract=off), only + - x / sqrt,
// floor and comparisons: the numpy restatement (tests/grid_field_ref.py) gives the same bits.  Written __host__ __device__: both kernels of
// grid_field_kernels.hip and the stand-alone checker (tools/grid_field_check.cpp, a C++ compiler that is not hipcc) share these bodies.
// field_cell is the one cell rule of the sample, the march and the adjoints.  field_grad_item, field_adjoint and field_corners are the
// sampler's adjoint (DESIGN.md sections 5.35 and 5.36; tests/grid_field_grad_ref.py), shared in the same way by k_sample_grid_grad,
// k_sample_grid_grad_repro and the two adjoint checkers (tools/grid_field_grad_check.cpp, tools/grid_field_grad_repro_check.cpp).
// min and max are the header's: a < b ? a : b and a > b ? a : b, so a NaN first operand yields the second.
#pragma once
#include <math.h>
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

const uint32_t kFieldClamp = 1u;        // CGRT_FIELD_CLAMP
const uint32_t kMarchInsideAbove = 1u;  // CGRT_ISO_INSIDE_ABOVE
const uint32_t kMarchMiss = 0u, kMarchHit = 1u, kMarchExhausted = 2u, kMarchNonfinite = 3u;
const uint32_t kCanonicalNan = 0x7fc00000u;

// the grid as the sampler reads it; top[c] = (float)(dims[c] - 1)
struct GridField {
    const float* values;  // nx ny nz, index (iz ny + iy) nx + ix
    float origin[3], spacing[3], top[3];
    uint32_t nx, ny, nz;
};
// CgrtMarchParams with the flag decoded
struct MarchRules {
    float iso, relax, min_step, hit_eps;
    uint32_t max_steps, refine, above;
};
// CgrtGridHit before its NaNs are made canonical
struct MarchResult {
    float t, value;
    uint32_t steps, status;
    float gradient[3];
};

CGRT_HD float field_min(const float a, const float b) { return a < b ? a : b; }
CGRT_HD float field_max(const float a, const float b) { return a > b ? a : b; }
CGRT_HD uint32_t field_bits(const float v) {  // the stored word: every NaN is 0x7fc00000
    uint32_t u;
    memcpy(&u, &v, 4);
    return v != v ? kCanonicalNan : u;
}
CGRT_HD bool field_finite(const float v) { return fabsf(v) <= 3.402823466e+38f; }

// The cell of p under the sampler's rule: the clamp, the containment test, min(floor, n - 2) and the fraction -- the one definition that
// the sample, the march and both adjoints share.  false: p is outside and i, f are not written.
CGRT_HD bool field_cell(const GridField& G, const float px, const float py, const float pz, const bool clamp, int (&i)[3], float (&f)[3]) {
    float u[3] = {(px - G.origin[0]) / G.spacing[0], (py - G.origin[1]) / G.spacing[1], (pz - G.origin[2]) / G.spacing[2]};
    if (clamp) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int c = 0; c < 3; c++) u[c] = u[c] < 0.0f ? 0.0f : (u[c] > G.top[c] ? G.top[c] : u[c]);
    }
    if (!(0.0f <= u[0] && u[0] <= G.top[0] && 0.0f <= u[1] && u[1] <= G.top[1] && 0.0f <= u[2] && u[2] <= G.top[2])) return false;
    const int fx = (int)floorf(u[0]), fy = (int)floorf(u[1]), fz = (int)floorf(u[2]);
    const int mx = (int)G.nx - 2, my = (int)G.ny - 2, mz = (int)G.nz - 2;
    i[0] = fx < mx ? fx : mx, i[1] = fy < my ? fy : my, i[2] = fz < mz ? fz : mz;
    f[0] = u[0] - (float)i[0], f[1] = u[1] - (float)i[1], f[2] = u[2] - (float)i[2];
    return true;
}

// The sample at p.  false: p is outside (the caller stores its `outside` value and a zero gradient).  GRAD false: g is not touched.
// The eight corner loads are issued together, ahead of the first use; the element offset is 64-bit.
template <bool GRAD>
CGRT_HD bool field_sample(const GridField& G, const float px, const float py, const float pz, const bool clamp, float& value, float (&g)[3]) {
    int i[3];
    float t[3];
    if (!field_cell(G, px, py, pz, clamp, i, t)) return false;
    const float tx = t[0], ty = t[1], tz = t[2];
    const uint64_t sy = G.nx, sz = (uint64_t)G.nx * G.ny;
    const float* q = G.values + (((uint64_t)i[2] * G.ny + (uint64_t)i[1]) * G.nx + (uint64_t)i[0]);
    const float v000 = q[0], v100 = q[1], v010 = q[sy], v110 = q[sy + 1], v001 = q[sz], v101 = q[sz + 1], v011 = q[sz + sy],
                v111 = q[sz + sy + 1];
    // along x: d_yz and a_yz
    const float d00 = v100 - v000, d10 = v110 - v010, d01 = v101 - v001, d11 = v111 - v011;
    const float a00 = v000 + tx * d00, a10 = v010 + tx * d10, a01 = v001 + tx * d01, a11 = v011 + tx * d11;
    // along y: e_z and b_z
    const float e0 = a10 - a00, e1 = a11 - a01;
    const float b0 = a00 + ty * e0, b1 = a01 + ty * e1;
    // along z
    const float w = b1 - b0;
    value = b0 + tz * w;
    if (GRAD) {
        const float dz0 = d00 + ty * (d10 - d00), dz1 = d01 + ty * (d11 - d01);
        g[0] = (dz0 + tz * (dz1 - dz0)) / G.spacing[0];
        g[1] = (e0 + tz * (e1 - e0)) / G.spacing[1];
        g[2] = w / G.spacing[2];
    }
    return true;
}

// The eight contributions of an inside point to the values' gradient (include/cgrt.h "Grid fields, the adjoint"),
// c[x + 2 y + 4 z] for the corner (i_x + x, i_y + y, i_z + z).  gv / gg are read only where has_gv / has_gg say they were given; the terms of
// an input that was not given are left out of the sum.  Every loop has constant bounds: unrolled, no array is indexed at run time.
CGRT_HD void field_adjoint(const float (&spacing)[3], const float (&f)[3], const bool has_gv, const float gv, const bool has_gg,
                           const float (&gg)[3], float (&c)[8]) {
    const float wx[2] = {1.0f - f[0], f[0]}, wy[2] = {1.0f - f[1], f[1]}, wz[2] = {1.0f - f[2], f[2]};
    float q[3] = {0.0f, 0.0f, 0.0f};
    if (has_gg) q[0] = gg[0] / spacing[0], q[1] = gg[1] / spacing[1], q[2] = gg[2] / spacing[2];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        const int x = k & 1, y = (k >> 1) & 1, z = k >> 2;
        const float wxy = wx[x] * wy[y];
        float s = 0.0f;
        if (has_gv) s = gv * (wxy * wz[z]);
        if (has_gg) {
            const float tx = (x ? q[0] : -q[0]) * (wy[y] * wz[z]);
            const float ty = (y ? q[1] : -q[1]) * (wx[x] * wz[z]);
            const float tz = (z ? q[2] : -q[2]) * wxy;
            s = has_gv ? ((s + tx) + ty) + tz : (tx + ty) + tz;
        }
        c[k] = s;
    }
}

// One call of the sampler's adjoint.  grid.values is not read (the sampler is linear in it).  One of grad_value /
// grad_gradient may be null; grad_values (nx ny nz) is added into.
struct FieldGradCall {
    GridField grid;
    const float* points;  // n x 3
    uint32_t n;
    uint32_t clamp;             // CGRT_FIELD_CLAMP
    const float* grad_value;    // n
    const float* grad_gradient; // n x 3
    float* grad_values;
};
// Point i of an adjoint call (i < Q.n): its cell, its grads where they were given, its eight contributions c and the element offset `at`
// of corner 0.  false: the point is outside -- it contributes nothing, no grad is read, at and c are not written.
CGRT_HD bool field_grad_item(const FieldGradCall& Q, const uint32_t i, uint64_t& at, float (&c)[8]) {
    const float* p = Q.points + 3ull * i;
    int ic[3];
    float f[3];
    if (!field_cell(Q.grid, p[0], p[1], p[2], Q.clamp != 0u, ic, f)) return false;
    const bool has_gv = Q.grad_value != nullptr, has_gg = Q.grad_gradient != nullptr;
    float gv = 0.0f, gg[3] = {0.0f, 0.0f, 0.0f};
    if (has_gv) gv = Q.grad_value[i];
    if (has_gg) {
        const float* g = Q.grad_gradient + 3ull * i;
        gg[0] = g[0], gg[1] = g[1], gg[2] = g[2];
    }
    field_adjoint(Q.grid.spacing, f, has_gv, gv, has_gg, gg, c);
    at = ((uint64_t)ic[2] * Q.grid.ny + (uint64_t)ic[1]) * Q.grid.nx + (uint64_t)ic[0];
    return true;
}
// fn(k, element offset) for the eight corners of the cell at `at`, k = x + 2 y + 4 z a constant in every call.
template <class F>
CGRT_HD void field_corners(const GridField& G, const uint64_t at, F fn) {
    const uint64_t sy = G.nx, sz = (uint64_t)G.nx * G.ny;
    fn(0, at);
    fn(1, at + 1);
    fn(2, at + sy);
    fn(3, at + sy + 1);
    fn(4, at + sz);
    fn(5, at + sz + 1);
    fn(6, at + sz + sy);
    fn(7, at + sz + sy + 1);
}

// The march of one ray {o, d, t_ray}.  work (COUNT only): {1 if the ray entered the box, main-loop samples, refinement samples} are added.
// At most max_steps + refine samples and one closing sample (value and gradient of a HIT) whatever the data.
template <bool COUNT>
CGRT_HD void field_march(const GridField& G, const MarchRules& P, const float* ray, MarchResult& R, uint32_t (&work)[3]) {
    const float ox = ray[0], oy = ray[1], oz = ray[2], dx = ray[3], dy = ray[4], dz = ray[5], t_ray = ray[6];
    R.t = INFINITY;
    R.value = 0.0f;
    R.steps = 0u;
    R.status = kMarchMiss;
    R.gradient[0] = R.gradient[1] = R.gradient[2] = 0.0f;
    if (COUNT) work[0] = work[1] = work[2] = 0u;
    const float len = sqrtf(((dx * dx) + (dy * dy)) + (dz * dz));
    if (!(field_finite(ox) && field_finite(oy) && field_finite(oz) && field_finite(dx) && field_finite(dy) && field_finite(dz))) return;
    if (t_ray != t_ray || !(len > 0.0f) || !field_finite(len)) return;
    // the box
    float t0 = 0.0f, t1 = t_ray;
    const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 3; c++) {
        const float far_c = G.origin[c] + G.top[c] * G.spacing[c];
        const float lo = field_min(G.origin[c], far_c), hi = field_max(G.origin[c], far_c);
        if (d[c] == 0.0f) {
            if (!(lo <= o[c] && o[c] <= hi)) return;
        } else {
            const float ta = (lo - o[c]) / d[c], tb = (hi - o[c]) / d[c];
            t0 = field_max(t0, field_min(ta, tb));
            t1 = field_min(t1, field_max(ta, tb));
        }
    }
    if (!(t0 <= t1)) return;
    if (COUNT) work[0] = 1u;
    float t = t0, t_prev = 0.0f, v = 0.0f, unused[3];
    bool have_prev = false;
    uint32_t k = 0u;
    for (;;) {  // at most max_steps passes: k grows by one per pass and the pass with k + 1 == max_steps leaves
        if (!field_sample<false>(G, ox + t * dx, oy + t * dy, oz + t * dz, true, v, unused)) v = NAN;
        if (COUNT) work[1]++;
        const float g = P.above ? P.iso - v : v - P.iso;
        if (g != g) {
            R.t = t, R.value = NAN, R.steps = k, R.status = kMarchNonfinite;
            return;
        }
        if (g <= P.hit_eps) break;
        if (t >= t1) {
            R.steps = k;
            return;
        }
        if (k + 1u == P.max_steps) {
            R.t = t, R.value = v, R.steps = P.max_steps, R.status = kMarchExhausted;
            return;
        }
        const float dt = field_max((P.relax * g) / len, P.min_step);
        t_prev = t;
        have_prev = true;
        t = field_min(t + dt, t1);
        k++;
    }
    // the hit: bisection of (t_prev, t] on g <= hit_eps
    float ta = t_prev, tb = t;
    if (have_prev)
        for (uint32_t r = 0; r < P.refine; r++) {
            const float tm = ta + 0.5f * (tb - ta);
            float vm;
            if (!field_sample<false>(G, ox + tm * dx, oy + tm * dy, oz + tm * dz, true, vm, unused)) vm = NAN;
            if (COUNT) work[2]++;
            const float gm = P.above ? P.iso - vm : vm - P.iso;
            if (gm <= P.hit_eps)
                tb = tm;
            else
                ta = tm;
        }
    R.t = tb, R.steps = k, R.status = kMarchHit;
    if (!field_sample<true>(G, ox + tb * dx, oy + tb * dy, oz + tb * dz, true, R.value, R.gradient)) {  // (not reached: tb was sampled inside)
        R.value = NAN;
        R.gradient[0] = R.gradient[1] = R.gradient[2] = 0.0f;
    }
}

}  // namespace cgrt
