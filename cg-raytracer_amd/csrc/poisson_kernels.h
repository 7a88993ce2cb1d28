// poisson_kernels.h -- host-callable driver of the Poisson-disk kernels in poisson_kernels.hip (include/cgrt.h cgrt_poisson_disk*;
// DESIGN.md section 5.29).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cgrt {

// The hashed grid has a power of two of buckets, about one per point, within these bounds (a multiple of the scan's 1024-entry tile).
// (The point-neighbour grid, point_neighbor_kernels.h, takes its bucket count and its rounding from here, on the host and in its kernels.)
const uint32_t kPoissonMinBuckets = 1024u, kPoissonMaxBuckets = 1u << 26;
__host__ __device__ inline uint32_t poisson_buckets(uint64_t n) {
    uint32_t b = kPoissonMinBuckets;
    while (b < kPoissonMaxBuckets && b < n) b <<= 1;
    return b;
}
__host__ __device__ inline uint64_t poisson_round16(uint64_t bytes) { return (bytes + 15ull) & ~15ull; }
// The workspace, carved in this order from its first 16-byte boundary (hence the 8 bytes of slack behind an 8-byte aligned pointer):
//   header 64 | bucket counts 4 B | bucket starts 4 (B + 1) | tile sums 4 (B / 1024) | order words 4 n | states n | two work lists 4 n
//   each | bucket entries: order words 4 n, {x, y, z, index} 16 n
// Every part is written before it is read: the contents need no initialisation.
inline uint64_t poisson_workspace_bytes(uint64_t n) {
    const uint64_t B = poisson_buckets(n);
    return 8ull + 64ull + 4ull * B + poisson_round16(4ull * (B + 1ull)) + poisson_round16(4ull * (B / 1024ull)) + poisson_round16(4ull * n) +
           poisson_round16(n) + 2ull * poisson_round16(4ull * n) + poisson_round16(4ull * n) + 16ull * n;
}

// One call.  All pointers device memory; priority NULL: the Philox order under `seed`.
struct PoissonCall {
    const float* points;       // n x 3
    uint32_t n;                // <= 0x7fffffff, > 0
    float min_dist2;           // not +inf (NaN or <= 0: nothing conflicts)
    unsigned long long seed;
    const uint32_t* priority;  // n words, or NULL
    uint8_t* keep;             // n bytes
    void* workspace;           // poisson_workspace_bytes(n) bytes, 8-byte aligned
};
// what cgrt_debug_poisson_work reports (only a counted run fills pair_tests, buckets_used and the two times)
struct PoissonWork {
    uint64_t rounds, pair_tests, buckets_used, buckets, build_ns, rounds_ns;
};
// Runs the whole selection on `stream` and returns when keep[] is complete: the passes, then batches of rounds with one read-back of the
// header into `pinned` (64 bytes of pinned host memory, this call's alone) per batch, then the flags and the count.  brute: no grid, every
// pair in every round.  work non-NULL: the counted kernels.  hipErrorLaunchFailure if the rounds did not end within n (they must).
hipError_t run_poisson_disk(const PoissonCall& Q, bool brute, uint32_t* pinned, hipStream_t stream, uint64_t* kept, PoissonWork* work);

// The exclusive scan of B bucket counts (B a multiple of 1024) on `stream`: bstart[b] = the sum of bcount[0 .. b), bstart[B] = the total;
// sums: B / 1024 words of scratch.  The three k_poisson_scan_* kernels, launched here for both grids: one copy of them in the library.
void launch_bucket_scan(const uint32_t* bcount, uint32_t* sums, uint32_t* bstart, uint32_t B, hipStream_t stream);

}  // namespace cgrt
