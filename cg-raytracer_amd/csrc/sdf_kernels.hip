// sdf_kernels.hip -- signed distance and occupancy (include/cgrt.h cgrt_signed_distance*): for every point the
// square root of cgrt_closest_points' dist2, signed by a majority vote over the parities of cgrt_count_crossings along a few fixed
// directions.  One kernel, one point per lane, nothing in between:
//
// phase 1  the closest-point search of k_closest (closest_device.h: closest_tri, box_lb2, child_key, order2 -- the same arithmetic, the
//          same `lb2 > bound` rule).  Only the bound and the winner's id are read afterwards, so the point and the barycentrics of Best
//          are dead and cost no register; the equal-dist2 tie rule does not change the value.
// phase 2  per direction the count search of k_crossings<false, ..> (crossing_device.h: cross_records, cross_packet_step; walk_exact.h
//          sub_node_step), keeping only the parity.  Once more than ndirs / 2 walks agree the others are skipped: the vote is decided.
//          BRUTE_PARITY and a ray outside the conservative test's envelope test every record, as the crossing entries do.
// Both phases use one lane-interleaved LDS region, sized for the closest stack (two dwords per entry) and reused by the parity walks (one
// dword per entry): a lane only ever touches its own column, so no barrier separates them.  One f32 and / or one byte is stored per point.
// GRID: the lane makes its point from its grid index (SdfPoints).
#include <hip/hip_runtime.h>

#include "closest_device.h"
#include "crossing_device.h"
#include "sdf_kernels.h"

namespace cgrt {

namespace {

#define CGRT_SDF_BLOCK 128
static_assert(CGRT_SDF_BLOCK == CGRT_CLOSEST_BLOCK && CGRT_SDF_BLOCK == CGRT_CROSS_BLOCK, "the stacks are laid out for 128 lanes");

template <bool COUNT>
__device__ __forceinline__ void sdf_closest(const SceneDev& S, const float px, const float py, const float pz, uint32_t* const stk, Best& B,
                                            unsigned long long& c_nodes, unsigned long long& c_tris) {
    uint32_t cur = topo_ref(S.root_ref);
    int sp = 0;
    for (;;) {
        bool pop = true;
        if (cur & REF_LEAF) {  // a run of 1..32 records
            const uint32_t first = cur & REF_INDEX26, cnt = ((cur >> 26) & 31u) + 1u;
            const float4* q = reinterpret_cast<const float4*>(S.tris + first);
            if (COUNT) c_tris += cnt;
            for (uint32_t k = 0; k < cnt; k++) closest_tri(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3], px, py, pz, B);
        } else if (cur & CL_LEAF) {  // a reference leaf scanned linearly
            const LeafRec L = S.leaves[cur & ~CL_LEAF];
            const float4* q = reinterpret_cast<const float4*>(S.tris + L.first);
            if (COUNT) c_tris += L.count;
            for (uint32_t k = 0; k < L.count; k++) closest_tri(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3], px, py, pz, B);
        } else {
            if (COUNT) c_nodes++;
            uint32_t k0, k1, k2 = 0xffffffffu, k3 = 0xffffffffu, f0, f1, f2 = REF_NONE, f3 = REF_NONE;
            if (cur & CL_SUB) {  // a transposed node: lo.x, hi.x, lo.y, hi.y, lo.z, hi.z of the four children, then the references
                const float4* q = reinterpret_cast<const float4*>(S.subnodes + (cur & ~CL_SUB));
                const float4 lx = q[0], hx = q[1], ly = q[2], hy = q[3], lz = q[4], hz = q[5];
                const uint4 m = *reinterpret_cast<const uint4*>(q + 6);
                const float l0 = box_lb2(lx.x, hx.x, ly.x, hy.x, lz.x, hz.x, px, py, pz);
                const float l1 = box_lb2(lx.y, hx.y, ly.y, hy.y, lz.y, hz.y, px, py, pz);
                const float l2 = box_lb2(lx.z, hx.z, ly.z, hy.z, lz.z, hz.z, px, py, pz);
                const float l3 = box_lb2(lx.w, hx.w, ly.w, hy.w, lz.w, hz.w, px, py, pz);
                k0 = child_key(m.x, l0, B.d2);
                k1 = child_key(m.y, l1, B.d2);
                k2 = child_key(m.z, l2, B.d2);
                k3 = child_key(m.w, l3, B.d2);
                f0 = sub_ref(m.x), f1 = sub_ref(m.y), f2 = sub_ref(m.z), f3 = sub_ref(m.w);  // (only read where the key is not all ones)
            } else {  // NodePacket: two child boxes {lo.xyz, hi.xyz}
                const float4* q = reinterpret_cast<const float4*>(S.packets + cur);
                const float4 a = q[0], b = q[1], c = q[2];
                const uint4 m = *reinterpret_cast<const uint4*>(q + 3);
                const float l0 = box_lb2(a.x, a.w, a.y, b.x, a.z, b.y, px, py, pz);
                const float l1 = box_lb2(b.z, c.y, b.w, c.z, c.x, c.w, px, py, pz);
                k0 = child_key(m.x, l0, B.d2);
                k1 = child_key(m.y, l1, B.d2);
                f0 = topo_ref(m.x), f1 = topo_ref(m.y);
            }
            // ascending by key: absent and culled children (all ones) last
            order2(k0, f0, k1, f1);
            order2(k2, f2, k3, f3);
            order2(k0, f0, k2, f2);
            order2(k1, f1, k3, f3);
            order2(k1, f1, k2, f2);
            // farthest first, so that the deferred children pop nearest first
            if (k3 != 0xffffffffu) {
                stk[(2 * sp) * 64] = f3, stk[(2 * sp + 1) * 64] = k3;
                sp++;
            }
            if (k2 != 0xffffffffu) {
                stk[(2 * sp) * 64] = f2, stk[(2 * sp + 1) * 64] = k2;
                sp++;
            }
            if (k1 != 0xffffffffu) {
                stk[(2 * sp) * 64] = f1, stk[(2 * sp + 1) * 64] = k1;
                sp++;
            }
            if (k0 != 0xffffffffu) {
                cur = f0;
                pop = false;
            }
        }
        if (pop) {
            bool got = false;
            while (sp > 0) {
                sp--;
                const uint32_t r = stk[(2 * sp) * 64];
                const float lb = __uint_as_float(stk[(2 * sp + 1) * 64]);
                if (!(lb > B.d2)) {  // the bound may have fallen since the child was deferred
                    cur = r;
                    got = true;
                    break;
                }
            }
            if (!got) break;
        }
    }
}

// the parity of cgrt_count_crossings' count for the ray {o, d, +inf}
template <bool COUNT, bool BRUTE_PARITY>
__device__ __forceinline__ uint32_t sdf_parity(const SceneDev& S, const F3 o, const F3 d, uint32_t* const stk, unsigned long long& c_nodes,
                                               unsigned long long& c_tris) {
    CrossSlot Q;
    Q.t_in = __builtin_inff();
    Q.bound = Q.t_in;
    Q.kept = 0u;
    Q.count = 0u;
    Q.rec = nullptr;
    Q.len = 0ull;
    Q.room = 0u;
    Q.shrink = false;
    LaneCounters cnt;
    const RayPre P = make_raypre(S, o, d, Q.t_in);
    if (BRUTE_PARITY || !P.regular) {
        if (COUNT) c_tris += S.ntris;
        for (uint32_t r = 0; r < S.ntris; r += SUB_RUN_MAX)
            cross_records<false>(S, (unsigned long long)S.tri_base + r, min(SUB_RUN_MAX, S.ntris - r), o, d, Q);
    } else {
        uint32_t cur = cross_topo_ref(S.root_ref);
        int sp = 0;
        for (;;) {
            if (cur == REF_NONE) {
                if (sp == 0) break;
                sp--;
                cur = stk[sp * CGRT_STRIDE];
            }
            if (cur & REF_LEAF) {  // a run of 1..32 records
                if (COUNT) c_tris += run_count(cur);
                cross_records<false>(S, run_first(cur), run_count(cur), o, d, Q);
                cur = REF_NONE;
            } else if (cur & CR_LEAF) {  // a reference leaf scanned linearly
                const LeafRec L = S.leaves[cur & ~CR_LEAF];
                if (COUNT) c_tris += L.count;
                for (uint32_t r = 0; r < L.count; r += SUB_RUN_MAX)
                    cross_records<false>(S, (unsigned long long)L.first + r, min(SUB_RUN_MAX, L.count - r), o, d, Q);
                cur = REF_NONE;
            } else if (cur & CR_PACKET) {
                if (COUNT) c_nodes++;
                cross_packet_step(S, P, Q.bound, cur, sp, stk);
            } else {  // an accelerator node: the nearest hit child becomes cur, the others are deferred
                sub_node_step<COUNT>(S, P, Q.bound, cur, sp, stk, cnt);
            }
        }
    }
    if (COUNT) c_nodes += cnt.sub;
    return Q.count & 1u;
}

template <int GRID, bool COUNT, bool BRUTE_PARITY>
__global__ __launch_bounds__(CGRT_SDF_BLOCK) void k_sdf(const SceneDev S, const SdfArgs A, unsigned long long* __restrict__ counters) {
    // phase 1: slot s of lane l of wave w at w * (2 * CLOSEST_STACK_ENTRIES * 64) + s * 64 + l, entry e = slots 2e {ref}, 2e + 1 {lb2};
    // phase 2: entry e of the same lane in slot e
    __shared__ uint32_t s_stk[2 * CLOSEST_STACK_ENTRIES * CGRT_SDF_BLOCK];
    unsigned long long i;  // the result's index, below A.n
    float px, py, pz;
    if (GRID == SDF_LIST) {
        i = (unsigned long long)blockIdx.x * CGRT_SDF_BLOCK + threadIdx.x;
        if (i >= A.n) return;
        px = A.points[3 * i], py = A.points[3 * i + 1], pz = A.points[3 * i + 2];
    } else {
        const uint32_t nx = A.dims[0], ny = A.dims[1], nz = A.dims[2];
        uint32_t ix, iy, iz;
        if (GRID == SDF_GRID_BRICK) {  // a block: 8 x 4 x 4 grid points, wave w the brick at x offset 4w, lane l at {l & 3, (l >> 2) & 3, l >> 4}
            const uint32_t bx = (nx + 7u) >> 3, by = (ny + 3u) >> 2;
            const uint32_t b = blockIdx.x, bxi = b % bx, rest = b / bx, byi = rest % by, bzi = rest / by;
            ix = bxi * 8u + (threadIdx.x >> 6) * 4u + (threadIdx.x & 3u);
            iy = byi * 4u + ((threadIdx.x >> 2) & 3u);
            iz = bzi * 4u + ((threadIdx.x >> 4) & 3u);
            if (ix >= nx || iy >= ny || iz >= nz) return;  // beyond the grid's edge
        } else {
            const unsigned long long j = (unsigned long long)blockIdx.x * CGRT_SDF_BLOCK + threadIdx.x;
            if (j >= A.n) return;
            const uint32_t row = (uint32_t)(j / nx);
            ix = (uint32_t)(j % nx), iy = row % ny, iz = row / ny;
        }
        i = ((unsigned long long)iz * ny + iy) * nx + ix;
        // origin + (float)index * spacing: the product rounded, then the sum (an index is below 2^24: exact as f32)
        px = __fadd_rn(A.origin[0], __fmul_rn((float)ix, A.spacing[0]));
        py = __fadd_rn(A.origin[1], __fmul_rn((float)iy, A.spacing[1]));
        pz = __fadd_rn(A.origin[2], __fmul_rn((float)iz, A.spacing[2]));
    }
    uint32_t* const stk = s_stk + (threadIdx.x >> 6) * (2 * CLOSEST_STACK_ENTRIES * 64) + (threadIdx.x & 63u);
    unsigned long long c_cl_nodes = 0, c_cl_tris = 0, c_cr_nodes = 0, c_cr_tris = 0, c_walks = 0;
    float s = __builtin_inff();
    bool inside = false;
    if (S.root_ref != REF_NONE && finite3(px, py, pz)) {
        if (A.want_sdf) {
            Best B;  // (only the bound and whether a triangle qualified are read: the compiler drops the point and the barycentrics)
            B.d2 = A.max_dist2;
            B.prim = REF_NONE;
            B.qx = B.qy = B.qz = B.v = B.w = 0.0f;
            sdf_closest<COUNT>(S, px, py, pz, stk, B, c_cl_nodes, c_cl_tris);
            if (B.prim != REF_NONE) s = sqrtf(B.d2);  // (IEEE: the Makefile's -fhip-fp32-correctly-rounded-divide-sqrt)
        }
        const uint32_t half = A.ndirs >> 1;
        uint32_t odd = 0u, even = 0u;
        for (uint32_t j = 0; j < A.ndirs && odd <= half && even <= half; j++) {
            const uint32_t par = sdf_parity<COUNT, BRUTE_PARITY>(S, f3(px, py, pz), f3(A.dirs[j][0], A.dirs[j][1], A.dirs[j][2]), stk, c_cr_nodes,
                                                                 c_cr_tris);
            odd += par;
            even += 1u - par;
            if (COUNT) c_walks++;
        }
        inside = odd > half;
    }
    if (A.sdf) A.sdf[i] = inside ? -s : s;
    if (A.inside) A.inside[i] = inside ? 1 : 0;
    if (COUNT) {
        atomicAdd(counters, c_cl_nodes);
        atomicAdd(counters + 1, c_cl_tris);
        atomicAdd(counters + 2, c_cr_nodes);
        atomicAdd(counters + 3, c_cr_tris);
        atomicAdd(counters + 4, c_walks);
    }
}

template <int GRID, bool COUNT>
hipError_t launch_one(const SceneDev& S, const SdfArgs& A, const unsigned blocks, bool brute_parity, unsigned long long* counters,
                      hipStream_t stream) {
    const dim3 grid(blocks), block(CGRT_SDF_BLOCK);
    if (brute_parity)
        hipLaunchKernelGGL((k_sdf<GRID, COUNT, true>), grid, block, 0, stream, S, A, counters);
    else
        hipLaunchKernelGGL((k_sdf<GRID, COUNT, false>), grid, block, 0, stream, S, A, counters);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sdf(const SceneDev& S, const SdfArgs& A, SdfPoints how, bool brute_parity, unsigned long long* counters, hipStream_t stream) {
    if (A.n == 0) return hipSuccess;
    if (A.n > 0x7fffffffu || (!A.sdf && !A.inside && !counters) || A.ndirs < 1 || A.ndirs > 7 || !(A.ndirs & 1u) || (counters && how != SDF_LIST))
        return hipErrorInvalidValue;
    const unsigned linear = (unsigned)(((uint64_t)A.n + CGRT_SDF_BLOCK - 1) / CGRT_SDF_BLOCK);
    if (how == SDF_LIST) {
        if (!A.points) return hipErrorInvalidValue;
        return counters ? launch_one<SDF_LIST, true>(S, A, linear, brute_parity, counters, stream)
                        : launch_one<SDF_LIST, false>(S, A, linear, brute_parity, nullptr, stream);
    }
    const uint64_t plane = (uint64_t)A.dims[0] * A.dims[1];  // (n fits 31 bits: no product below wraps)
    if (plane == 0 || plane > A.n || plane * A.dims[2] != A.n) return hipErrorInvalidValue;
    if (how == SDF_GRID_LINEAR) return launch_one<SDF_GRID_LINEAR, false>(S, A, linear, brute_parity, nullptr, stream);
    // (at most as many bricks as grid points: the count fits the launch's 32-bit grid)
    const uint64_t bricks = (uint64_t)((A.dims[0] + 7u) >> 3) * ((A.dims[1] + 3u) >> 2) * ((A.dims[2] + 3u) >> 2);
    return launch_one<SDF_GRID_BRICK, false>(S, A, (unsigned)bricks, brute_parity, nullptr, stream);
}

}  // namespace cgrt
