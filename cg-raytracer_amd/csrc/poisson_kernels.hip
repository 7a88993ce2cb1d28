// poisson_kernels.hip -- Poisson-disk sets: the lexicographically first maximal independent set of "closer than a radius" (include/cgrt.h
// cgrt_poisson_disk*).  Point i comes before j iff (P_i, i) < (P_j, j), compared as ONE 64-bit key; i is kept iff it is
// finite and no kept point before it conflicts with it.  The result is a function of the points, the radius and the order alone.
//
// Passes, all on the call's stream:
//   k_poisson_init     per point: finite?, its order word P (Philox word 3 of philox_device.h, or the caller's priority), its first state;
//                      the per-axis minimum and maximum of the finite points by ordered-integer atomics, one set per wave
//   k_poisson_count    per finite point: its cell, the cell's bucket, one atomic add on the bucket's count
//   k_poisson_scan_*   an exclusive scan of the bucket counts in tiles of 1024: tile sums, their scan by one block, the tiles again
//   k_poisson_scatter  per finite point: {x, y, z, index} and P into the bucket's range (the order inside a bucket is whatever the atomics
//                      gave, and no result depends on it); the first work list: every finite point
//   k_poisson_round    one round over the work list of undecided points (below), as often as the data needs
//   k_poisson_finish   keep[i] = (state == KEPT), and the count
//
// The grid: point_grid_device.h, which states its arithmetic and argues that the cell range of a point holds every point that can conflict
// with it; the point-neighbour queries (point_neighbor_kernels.hip) share it.
//
// The rounds.  A state only ever goes from UNDECIDED to KEPT or REJECTED and never changes again.  An undecided i scans the points that come
// before it and conflict with it: one of them KEPT -> i is REJECTED; none of them UNDECIDED (all REJECTED) -> i is KEPT; else i goes on
// the next list.  Both verdicts rest on FINAL states of other points only, so a decision taken on any mix of states from before and during
// the round is the sequential one; a stale read (another CU's L1, a store still in flight) shows UNDECIDED for a decided point and only
// delays i.  Nothing is fenced inside a round; the kernel boundary publishes the states to the next round.  The earliest undecided point
// sees only final states before it, so it decides in every round: at most n rounds, with the Philox order about log n.
// The three list counters rotate: round r reads counter r % 3, appends under (r + 1) % 3 and clears (r + 2) % 3, which round r - 1 read.
//
// Plain vector loads, stores and atomics only; no scratch; LDS only in the scan (4 words per block).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>

#include "philox_device.h"
#include "point_grid_device.h"
#include "poisson_kernels.h"

namespace cgrt {

namespace {

enum : uint32_t { P_UNDECIDED = 0, P_KEPT = 1, P_REJECTED = 2 };
// header words (H_LO = 0 and H_HI = 3: point_grid_device.h)
enum : uint32_t { H_CNT = 6, H_KEPT = 9, H_PAIRS = 10 /* 64 bits */, H_USED = 12, H_ROUNDS = 13 };

struct PoissonDev {
    const float* points;
    const uint32_t* priority;
    uint32_t n;
    float m, R;
    unsigned long long seed;
    uint32_t bmask;  // buckets - 1
    uint32_t* hdr;
    uint32_t* bcount;
    uint32_t* bstart;
    uint32_t* sums;
    uint32_t* P;
    uint8_t* state;
    uint32_t* list[2];
    uint32_t* eP;
    float4* epos;
    uint8_t* keep;
};

// the conflict test of include/cgrt.h: every operation rounded on its own (-ffp-contract=off), symmetric in the two points
__device__ __forceinline__ bool conflict(float xi, float yi, float zi, float xj, float yj, float zj, float m) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return (dx * dx + dy * dy) + dz * dz < m;
}
// every lane of the wave calls this; the lanes with `pred` append `value` under one atomic add of the wave
__device__ __forceinline__ void wave_append(bool pred, uint32_t value, uint32_t* counter, uint32_t* list) {
    const unsigned long long mask = __ballot(pred);
    if (mask == 0ull) return;
    const uint32_t lane = lane_id();
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0u;
    if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    if (pred) list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = value;
}
// first: the state of a finite point (P_KEPT when nothing can conflict)
__global__ __launch_bounds__(256) void k_poisson_init(const PoissonDev A, const uint32_t first, const int bounds) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t klo[3] = {0u, 0u, 0u}, khi[3] = {0u, 0u, 0u};
    if (i < A.n) {
        const float x = A.points[3ull * i], y = A.points[3ull * i + 1], z = A.points[3ull * i + 2];
        const bool finite = isfinite(x) && isfinite(y) && isfinite(z);
        uint32_t p;
        if (A.priority) {
            p = A.priority[i];
        } else {
            uint32_t w0, w1, w2;
            philox4x32_10(i, 0u, (uint32_t)A.seed, (uint32_t)(A.seed >> 32), w0, w1, w2, p);
        }
        A.P[i] = p;
        A.state[i] = (uint8_t)(finite ? first : (uint32_t)P_REJECTED);
        if (finite) {
            khi[0] = ordered(x), khi[1] = ordered(y), khi[2] = ordered(z);
            klo[0] = ~khi[0], klo[1] = ~khi[1], klo[2] = ~khi[2];
        }
    }
    if (!bounds) return;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const uint32_t l = wave_max(klo[a]), h = wave_max(khi[a]);
        if (lane_id() == 0u && h != 0u) {
            atomicMax(A.hdr + H_LO + a, l);
            atomicMax(A.hdr + H_HI + a, h);
        }
    }
}

template <bool COUNTED>
__global__ __launch_bounds__(256) void k_poisson_count(const PoissonDev A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n || A.state[i] == P_REJECTED) return;
    const Grid g = load_grid(A.hdr, A.R);
    const float x = A.points[3ull * i], y = A.points[3ull * i + 1], z = A.points[3ull * i + 2];
    const uint32_t b = bucket(cell(x, g.lo[0], g.h), cell(y, g.lo[1], g.h), cell(z, g.lo[2], g.h), A.bmask);
    if (COUNTED) {
        if (atomicAdd(A.bcount + b, 1u) == 0u) atomicAdd(A.hdr + H_USED, 1u);
    } else {
        atomicAdd(A.bcount + b, 1u);
    }
}

__global__ __launch_bounds__(256) void k_poisson_scan_tiles(const uint32_t* counts, uint32_t* sums) {
    __shared__ uint32_t lds[4];
    const uint4 c = reinterpret_cast<const uint4*>(counts)[blockIdx.x * 256u + threadIdx.x];
    uint32_t total;
    (void)block_scan(c.x + c.y + c.z + c.w, lds, &total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}
// one block: the tile sums to their exclusive scan, in place; the grand total to *end
__global__ __launch_bounds__(256) void k_poisson_scan_sums(uint32_t* sums, const uint32_t ntiles, uint32_t* end) {
    __shared__ uint32_t lds[4];
    uint32_t carry = 0u;
    for (uint32_t base = 0u; base < ntiles; base += 256u) {
        const uint32_t k = base + threadIdx.x;
        const uint32_t v = k < ntiles ? sums[k] : 0u;
        uint32_t total;
        const uint32_t excl = block_scan(v, lds, &total);
        if (k < ntiles) sums[k] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0u) *end = carry;
}
__global__ __launch_bounds__(256) void k_poisson_scan_apply(const uint32_t* counts, const uint32_t* sums, uint32_t* starts) {
    __shared__ uint32_t lds[4];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const uint4 c = reinterpret_cast<const uint4*>(counts)[k];
    uint32_t total;
    const uint32_t s = sums[blockIdx.x] + block_scan(c.x + c.y + c.z + c.w, lds, &total);
    reinterpret_cast<uint4*>(starts)[k] = make_uint4(s, s + c.x, s + c.x + c.y, s + c.x + c.y + c.z);
}

// (takes the counts back down to 0: slot = start + what is left of the count)
__global__ __launch_bounds__(256) void k_poisson_scatter(const PoissonDev A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < A.n && A.state[i] != P_REJECTED;
    if (live) {
        const Grid g = load_grid(A.hdr, A.R);
        const float x = A.points[3ull * i], y = A.points[3ull * i + 1], z = A.points[3ull * i + 2];
        const uint32_t b = bucket(cell(x, g.lo[0], g.h), cell(y, g.lo[1], g.h), cell(z, g.lo[2], g.h), A.bmask);
        const uint32_t slot = A.bstart[b] + atomicSub(A.bcount + b, 1u) - 1u;
        A.epos[slot] = make_float4(x, y, z, __uint_as_float(i));
        A.eP[slot] = A.P[i];
    }
    wave_append(live, i, A.hdr + H_CNT, A.list[0]);
}
// the brute form's first list
__global__ __launch_bounds__(256) void k_poisson_list(const PoissonDev A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    wave_append(i < A.n && A.state[i] != P_REJECTED, i, A.hdr + H_CNT, A.list[0]);
}

template <bool BRUTE, bool COUNTED>
__global__ __launch_bounds__(256) void k_poisson_round(const PoissonDev A, const uint32_t r) {
    const uint32_t cnt = A.hdr[H_CNT + r % 3u];
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx == 0u) {
        A.hdr[H_CNT + (r + 2u) % 3u] = 0u;
        if (cnt) A.hdr[H_ROUNDS] += 1u;
    }
    bool pending = false;
    uint32_t i = 0u;
    unsigned long long tests = 0ull;
    if (idx < cnt) {
        i = A.list[r & 1u][idx];
        const float x = A.points[3ull * i], y = A.points[3ull * i + 1], z = A.points[3ull * i + 2];
        const unsigned long long key = ((unsigned long long)A.P[i] << 32) | i;
        bool rejected = false;
        if (BRUTE) {
            for (uint32_t j = 0u; j < A.n && !rejected; j++) {
                if (COUNTED) tests++;
                if ((((unsigned long long)A.P[j] << 32) | j) >= key) continue;
                const uint32_t sj = A.state[j];
                if (sj == P_REJECTED) continue;
                if (!conflict(x, y, z, A.points[3ull * j], A.points[3ull * j + 1], A.points[3ull * j + 2], A.m)) continue;
                rejected = sj == P_KEPT;
                pending = true;
            }
        } else {
            const Grid g = load_grid(A.hdr, A.R);
            const uint32_t x0 = cell(x - A.R, g.lo[0], g.h), x1 = cell(x + A.R, g.lo[0], g.h);
            const uint32_t y0 = cell(y - A.R, g.lo[1], g.h), y1 = cell(y + A.R, g.lo[1], g.h);
            const uint32_t z0 = cell(z - A.R, g.lo[2], g.h), z1 = cell(z + A.R, g.lo[2], g.h);
            for (uint32_t cz = z0; cz <= z1 && !rejected; cz++)
                for (uint32_t cy = y0; cy <= y1 && !rejected; cy++)
                    for (uint32_t cx = x0; cx <= x1 && !rejected; cx++) {
                        const uint32_t b = bucket(cx, cy, cz, A.bmask);
                        const uint32_t end = A.bstart[b + 1u];
                        for (uint32_t t = A.bstart[b]; t < end; t++) {
                            const float4 q = A.epos[t];
                            const uint32_t j = __float_as_uint(q.w);
                            if (COUNTED) tests++;
                            if ((((unsigned long long)A.eP[t] << 32) | j) >= key) continue;
                            if (!conflict(x, y, z, q.x, q.y, q.z, A.m)) continue;
                            const uint32_t sj = A.state[j];
                            if (sj == P_REJECTED) continue;
                            pending = true;
                            if (sj == P_KEPT) {
                                rejected = true;
                                break;
                            }
                        }
                    }
        }
        if (rejected || !pending) A.state[i] = (uint8_t)(rejected ? P_REJECTED : P_KEPT);
        pending = pending && !rejected;
    }
    wave_append(pending, i, A.hdr + H_CNT + (r + 1u) % 3u, A.list[(r + 1u) & 1u]);
    if (COUNTED) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) tests += (unsigned long long)__shfl_xor((long long)tests, d);
        if (lane_id() == 0u && tests) atomicAdd(reinterpret_cast<unsigned long long*>(A.hdr + H_PAIRS), tests);
    }
}

__global__ __launch_bounds__(256) void k_poisson_finish(const PoissonDev A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool kept = i < A.n && A.state[i] == P_KEPT;
    if (i < A.n) A.keep[i] = kept ? 1 : 0;
    const unsigned long long mask = __ballot(kept);
    if (lane_id() == 0u && mask) atomicAdd(A.hdr + H_KEPT, (uint32_t)__popcll(mask));
}

uint64_t now_ns() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

void launch_bucket_scan(const uint32_t* bcount, uint32_t* sums, uint32_t* bstart, uint32_t B, hipStream_t stream) {
    const uint32_t ntiles = B / 1024u;
    const dim3 block(256);
    hipLaunchKernelGGL(k_poisson_scan_tiles, dim3(ntiles), block, 0, stream, bcount, sums);
    hipLaunchKernelGGL(k_poisson_scan_sums, dim3(1), block, 0, stream, sums, ntiles, bstart + B);
    hipLaunchKernelGGL(k_poisson_scan_apply, dim3(ntiles), block, 0, stream, bcount, sums, bstart);
}

hipError_t run_poisson_disk(const PoissonCall& Q, bool brute, uint32_t* pinned, hipStream_t stream, uint64_t* kept, PoissonWork* work) {
    if (Q.n == 0u || Q.n > 0x7fffffffu || !pinned) return hipErrorInvalidValue;
    const uint64_t n = Q.n, B = poisson_buckets(n);
    PoissonDev A{};
    char* p = reinterpret_cast<char*>(((uintptr_t)Q.workspace + 15u) & ~(uintptr_t)15u);
    auto carve = [&p](uint64_t bytes) {
        char* q = p;
        p += poisson_round16(bytes);
        return q;
    };
    A.hdr = reinterpret_cast<uint32_t*>(carve(64));
    A.bcount = reinterpret_cast<uint32_t*>(carve(4 * B));
    A.bstart = reinterpret_cast<uint32_t*>(carve(4 * (B + 1)));
    A.sums = reinterpret_cast<uint32_t*>(carve(4 * (B / 1024)));
    A.P = reinterpret_cast<uint32_t*>(carve(4 * n));
    A.state = reinterpret_cast<uint8_t*>(carve(n));
    A.list[0] = reinterpret_cast<uint32_t*>(carve(4 * n));
    A.list[1] = reinterpret_cast<uint32_t*>(carve(4 * n));
    A.eP = reinterpret_cast<uint32_t*>(carve(4 * n));
    A.epos = reinterpret_cast<float4*>(carve(16 * n));
    A.points = Q.points;
    A.priority = Q.priority;
    A.n = Q.n;
    A.m = Q.min_dist2;
    A.seed = Q.seed;
    A.bmask = (uint32_t)B - 1u;
    A.keep = Q.keep;
    const bool none = !(Q.min_dist2 > 0.0f);  // NaN or <= 0: nothing conflicts, every finite point is kept
    if (!none) {
        const double root = std::sqrt((double)Q.min_dist2);
        float R = (float)root;
        if ((double)R < root) R = std::nextafterf(R, INFINITY);
        A.R = std::nextafterf(R, INFINITY);
    }
    const dim3 block(256), grid((Q.n + 255u) / 256u);
    hipError_t e = work ? hipStreamSynchronize(stream) : hipSuccess;  // (a counted run's times begin behind the upload)
    if (e != hipSuccess) return e;
    const uint64_t t0 = work ? now_ns() : 0;
    e = hipMemsetAsync(A.hdr, 0, brute || none ? 64 : 64 + 4 * B, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_poisson_init, grid, block, 0, stream, A, none ? (uint32_t)P_KEPT : (uint32_t)P_UNDECIDED, !brute && !none ? 1 : 0);
    if (brute && !none) {
        hipLaunchKernelGGL(k_poisson_list, grid, block, 0, stream, A);
    } else if (!none) {
        if (work)
            hipLaunchKernelGGL(k_poisson_count<true>, grid, block, 0, stream, A);
        else
            hipLaunchKernelGGL(k_poisson_count<false>, grid, block, 0, stream, A);
        launch_bucket_scan(A.bcount, A.sums, A.bstart, (uint32_t)B, stream);
        hipLaunchKernelGGL(k_poisson_scatter, grid, block, 0, stream, A);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint64_t t1 = 0;
    if (work) {
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        t1 = now_ns();
    }
    // batches of rounds: the grid covers the last count read back (a list only shrinks); one read-back of the header per batch
    uint32_t upper = none ? 0u : Q.n, r = 0u;
    for (uint32_t batch = 0; upper; batch++) {
        if ((uint64_t)r > n + 16u) return hipErrorLaunchFailure;  // (cannot happen: the earliest undecided point decides in every round)
        const dim3 rgrid((upper + 255u) / 256u);
        for (uint32_t k = batch < 2u ? 4u : 8u; k-- > 0u; r++) {
            if (brute && work)
                hipLaunchKernelGGL((k_poisson_round<true, true>), rgrid, block, 0, stream, A, r);
            else if (brute)
                hipLaunchKernelGGL((k_poisson_round<true, false>), rgrid, block, 0, stream, A, r);
            else if (work)
                hipLaunchKernelGGL((k_poisson_round<false, true>), rgrid, block, 0, stream, A, r);
            else
                hipLaunchKernelGGL((k_poisson_round<false, false>), rgrid, block, 0, stream, A, r);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(pinned, A.hdr, 64, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        const uint32_t left = pinned[H_CNT + r % 3u];
        if (left > upper) return hipErrorLaunchFailure;
        upper = left;
    }
    const uint64_t t2 = work ? now_ns() : 0;
    hipLaunchKernelGGL(k_poisson_finish, grid, block, 0, stream, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(pinned, A.hdr, 64, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    if (kept) *kept = pinned[H_KEPT];
    if (work) {
        work->rounds = pinned[H_ROUNDS];
        work->pair_tests = (uint64_t)pinned[H_PAIRS] | ((uint64_t)pinned[H_PAIRS + 1] << 32);
        work->buckets_used = pinned[H_USED];
        work->buckets = brute || none ? 0 : B;
        work->build_ns = t1 - t0;
        work->rounds_ns = t2 - t1;
    }
    return hipSuccess;
}

}  // namespace cgrt
