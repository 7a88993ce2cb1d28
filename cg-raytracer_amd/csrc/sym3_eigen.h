// sym3_eigen.h -- steps 4 to 6 of include/cgrt.h "Point-set frames" (DESIGN.md section 5.33): the eigenvalues and eigenvectors of a
// symmetric 3 x 3 matrix by cyclic Jacobi, their ascending order, and the signs of the frame.  f32 throughout, every operation rounded
// on its own (-ffp-contract=off), only + - x / sqrt and comparisons: the numpy restatement (tests/point_frames_ref.py) gives the same
// bits.  No array is indexed by a run-time value, so on the device everything stays in registers.  Written __host__ __device__: a host
// program can call it as it stands (a C++ compiler that is not hipcc sees plain inline functions).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CGRT_HD __host__ __device__ __forceinline__
#else
#define CGRT_HD inline
#endif

namespace cgrt {

const int kSym3Sweeps = 8;  // the solve ends after this many sweeps in any case

// a symmetric matrix {xx, xy, xz, yy, yz, zz} and what becomes of it: lambda ascending, n / u / v the matching columns of V
struct Sym3 {
    float xx, xy, xz, yy, yz, zz;
};
struct Sym3Frame {
    float lambda[3];
    float n[3], u[3], v[3];
};

// One rotation in the plane (p, q), r the third index; vp, vq the columns p and q of V.  a_pq == 0: nothing to do.
CGRT_HD void sym3_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float (&vp)[3], float (&vq)[3]) {
    if (apq == 0.0f) return;
    const float theta = (aqq - app) / (2.0f * apq);
    const float t = (theta < 0.0f ? -1.0f : 1.0f) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
    const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
    const float h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0f;
    const float rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 3; i++) {
        const float a = c * vp[i] - s * vq[i], b = s * vp[i] + c * vq[i];
        vp[i] = a;
        vq[i] = b;
    }
}

// d_b < d_a: the two eigenvalues and their columns change places (a stable three-element sort is three of these)
CGRT_HD void sym3_order2(float& da, float& db, float (&va)[3], float (&vb)[3]) {
    if (db < da) {
        float t = da;
        da = db;
        db = t;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < 3; i++) {
            t = va[i];
            va[i] = vb[i];
            vb[i] = t;
        }
    }
}

// the component of largest magnitude, the first one on a tie (a NaN is never larger), made non-negative
CGRT_HD void sym3_lead_sign(float (&v)[3]) {
    float best = fabsf(v[0]), pick = v[0];
    if (fabsf(v[1]) > best) best = fabsf(v[1]), pick = v[1];
    if (fabsf(v[2]) > best) pick = v[2];
    if (pick < 0.0f) v[0] = -v[0], v[1] = -v[1], v[2] = -v[2];
}

// Steps 4 and 5.  Returns the number of sweeps run.
CGRT_HD int sym3_eigen(const Sym3& A, Sym3Frame& F) {
    float a00 = A.xx, a01 = A.xy, a02 = A.xz, a11 = A.yy, a12 = A.yz, a22 = A.zz;
    float c0[3] = {1.0f, 0.0f, 0.0f}, c1[3] = {0.0f, 1.0f, 0.0f}, c2[3] = {0.0f, 0.0f, 1.0f};  // the columns of V
    int sweeps = 0;
    while (sweeps < kSym3Sweeps) {
        sym3_rotate(a00, a11, a01, a02, a12, c0, c1);  // (0, 1), r = 2
        sym3_rotate(a00, a22, a02, a01, a12, c0, c2);  // (0, 2), r = 1
        sym3_rotate(a11, a22, a12, a01, a02, c1, c2);  // (1, 2), r = 0
        sweeps++;
        if (a01 == 0.0f && a02 == 0.0f && a12 == 0.0f) break;
    }
    sym3_order2(a00, a11, c0, c1);
    sym3_order2(a11, a22, c1, c2);
    sym3_order2(a00, a11, c0, c1);
    F.lambda[0] = a00, F.lambda[1] = a11, F.lambda[2] = a22;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 3; i++) F.n[i] = c0[i], F.u[i] = c1[i], F.v[i] = c2[i];
    return sweeps;
}

// Step 6.  oriented: (ox, oy, oz) is the query's orientation vector (used only if all three components are finite).
CGRT_HD void sym3_signs(Sym3Frame& F, const bool oriented, const float ox, const float oy, const float oz) {
    sym3_lead_sign(F.n);
    sym3_lead_sign(F.u);
    if (oriented) {
        const bool finite = fabsf(ox) <= 3.402823466e+38f && fabsf(oy) <= 3.402823466e+38f && fabsf(oz) <= 3.402823466e+38f;
        if (finite && (F.n[0] * ox + F.n[1] * oy) + F.n[2] * oz < 0.0f) F.n[0] = -F.n[0], F.n[1] = -F.n[1], F.n[2] = -F.n[2];
    }
    const float cx = F.n[1] * F.u[2] - F.n[2] * F.u[1], cy = F.n[2] * F.u[0] - F.n[0] * F.u[2], cz = F.n[0] * F.u[1] - F.n[1] * F.u[0];
    if ((cx * F.v[0] + cy * F.v[1]) + cz * F.v[2] < 0.0f) F.v[0] = -F.v[0], F.v[1] = -F.v[1], F.v[2] = -F.v[2];
}

// what a record stores in the place of any NaN: the sign and payload of a NaN are the one thing IEEE arithmetic leaves open
CGRT_HD float sym3_canonical(float x) { return x != x ? __builtin_bit_cast(float, (uint32_t)0x7fc00000u) : x; }

}  // namespace cgrt
