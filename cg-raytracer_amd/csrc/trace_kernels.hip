// trace_kernels.hip -- the shipped gfx950 kernels of the hot path: BoundingVolumeHierarchy::intersect
// (src/bounding_volume_hierarchy.cpp:850-881) for batches of rays, with optional fused primary-ray generation
// (src/main.cpp:691-694 + framework/src/trackball.cpp:92-103).  One ray per lane; the walk itself is in walk_exact.h
// (the reference's steps, one by one) and walk_fast.h (the certified walk: same answer from a better structure plus a
// proof, exact walk as fallback).  FAST selects the latter; the launchers take it when the scene carries a fast tree.
// Variants that are not shipped (persistent waves, per-wave stamps) live in variant_kernels.hip, the element-wise
// primitives of src/ray_tracing.h in prim_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "walk_quad.h"

#ifndef CGRT_LANE16_MAX_RAYS_DEFAULT
#define CGRT_LANE16_MAX_RAYS_DEFAULT 131072ull  // ray lists of at most this many rays: 16 rays per wave (see "kernel shape per launch")
#endif
#ifndef CGRT_STRIDED_WAVES_DEFAULT
#define CGRT_STRIDED_WAVES_DEFAULT 6144u  // waves per count-driven launch of an enqueued frame (strided_waves)
#endif
#ifndef CGRT_QUAD4_MAX_RAYS_DEFAULT
#define CGRT_QUAD4_MAX_RAYS_DEFAULT 8192ull  // ... of at most this many: 4 rays per wave, 16 lanes per ray (walk_quad.h)
#endif

namespace cgrt {

// Quad shape (walk_quad.h): a launch of single-wave workgroups, FOUR per 8x8 tile.  Workgroup b serves tile-block
// tb = (b / 32) * 8 + b % 8 -- the workgroup index the lane-per-ray launch with 64 threads gives that tile, same blockIdx % 8
// residue, i.e. same XCD -- and of its 64 pixels the 16 with index (b / 8 % 4) * 16 + threadIdx / 4; the four lanes of a quad
// carry the same pixel.  Results land where the lane-per-ray launch puts them (packed or not).
// VIEWS: a multi-view frame (FrameDev::views); *view = the lane's view (wave-uniform).
template <bool QUAD, bool VIEWS = false, bool ORDER = false>
__device__ __forceinline__ bool frame_pixel(const FrameDev& F, int& x, int& y, size_t& packed_index, bool& writer, uint32_t* view = nullptr) {
    if (QUAD) {
        const uint32_t b = blockIdx.x, tb = ((b >> 5) << 3) | (b & 7u);
        const uint32_t p = ((b >> 3) & 3u) * 16u + (threadIdx.x >> 2);
        packed_index = (size_t)tb * 64u + p;
        writer = (threadIdx.x & 3u) == 0u;
        return tile_pixel_of<VIEWS>(F, tb, p, x, y, view);
    }
    packed_index = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    writer = true;
    return tile_pixel_of<VIEWS, ORDER>(F, blockIdx.x, threadIdx.x, x, y, view);
}
// A multi-view frame's pixel index: view * W * H + y * W + x (< 2^31: the entries check nviews * W * H).
__device__ __forceinline__ size_t view_pixel(const FrameDev& F, uint32_t view, int x, int y) {
    return (size_t)view * (size_t)F.W * (size_t)F.H + (size_t)y * F.W + x;
}

// Frame gate (FrameDev::gate_*, capi.cpp frame_gate_rect): true for the whole wave when none of its lanes has a pixel
// inside the rectangle outside which every ray fails the mesh root gate -- the wave then needs no ray.  One scalar test when the
// launch carries no rectangle; four compares and a ballot otherwise.
__device__ __forceinline__ bool wave_outside_gate(const FrameDev& F, const bool active, const int x, const int y) {
    if (F.gate_x1 == 0) return false;
    const bool inside = active && x >= F.gate_x0 && x < F.gate_x1 && y >= F.gate_y0 && y < F.gate_y1;
    return __ballot(inside) == 0ull;
}

// HINT: the launch carries frame hints (cgrt_layout.h HintDev) -- an instantiation of its own, so that the plain frame kernel is the
// kernel it was (the hint code costs every launch a few percent when it is merely compiled in: measured).
// VIEWS: a multi-view frame (FrameDev::views, cgrt_trace_primary_views_device) -- also an instantiation of its own, for the same
// reason; each wave reads its view's camera from the device table (C is not used) and writes at view_pixel.  Never with HINT.
// RAYCAM (with VIEWS only): the table holds ray cameras (FrameDev::raycams, cgrt_*_raycams*) -- again instantiations of their own.  The
// wave reads its 80-byte entry before the walk; only o and d live through it.
// ORDER: the launch carries an order table (FrameDev::order) -- an instantiation of its own for HINT's reason; the plain
// frame kernel plus one scalar load per wave.
// STAMP: a profile frame of the order policy -- the plain kernel, and every wave that enters the tree leaves its wall time (s_memrealtime,
// 10 ns ticks) in ticks[its super-tile] by one atomicMax; `counters` carries the ticks (one u32 per padded super-tile, zeroed in front of
// the launch).  The start stamp waits in LDS like hint_park's.  Never timed against the plain kernel: one frame in CGRT_ORDER_PERIOD.
template <bool COUNT, bool FAST, bool QUAD = false, bool HINT = false, bool VIEWS = false, bool RAYCAM = false, bool ORDER = false, bool STAMP = false>
__global__ CGRT_LB void k_trace_primary(SceneDev S, CameraDev C, FrameDev F, CgrtHitDev* __restrict__ hits, float* __restrict__ normals,
                                        unsigned long long* counters) {
    static_assert(!(HINT && VIEWS), "multi-view frames take no hints");
    static_assert(VIEWS || !RAYCAM, "ray cameras come from the views table");
    static_assert(!((ORDER || STAMP) && (COUNT || QUAD || HINT || VIEWS)) && !(ORDER && STAMP), "ordered and profile frames: the plain kernel only");
    extern __shared__ uint32_t s_lds[];  // CGRT_LDS_WORDS(blockDim.x): stacks, quad-tail owner maps, workgroup scratch
    int x = 0, y = 0;
    size_t pidx;
    bool writer;
    bool active;
    uint32_t view = 0;
    if (HINT && F.hint) {  // (the run-time test is redundant; with it the compiler keeps the walk out of scratch)
        pidx = 0;          // (hinted frames are never packed)
        writer = true;
        active = hinted_tile_pixel(F, x, y, CGRT_HINT_SCRATCH(s_lds));
    } else {
        if (HINT && (threadIdx.x & 63u) == 0u) CGRT_HINT_SCRATCH(s_lds)[1] = 0xffffffffu;  // nothing for hint_finish
        if (STAMP && (threadIdx.x & 63u) == 0u) CGRT_HINT_SCRATCH(s_lds)[0] = (uint32_t)__builtin_amdgcn_s_memrealtime();
        active = frame_pixel<QUAD, VIEWS, ORDER>(F, x, y, pidx, writer, &view);
    }
    // The counting instantiations take every pixel through the per-pixel gate (their counters are the per-pixel path's), the multi-view
    // ones carry no rectangle, and the hinted one is the kernel it was: its frames are as long as their longest wave, not their empty ones
    // (DESIGN.md 5.22).  A wave outside the rectangle writes what finish_ray writes for a ray that failed the root gate of a scene
    // without spheres -- the same 16 bytes at the same address, no normal -- and ends.
    if (!COUNT && !VIEWS && !HINT && wave_outside_gate(F, active, x, y)) {
        if (active && writer) {
            CgrtHitDev miss;
            miss.t = 3.402823466e+38f;
            miss.prim_id = 0xffffffffu;
            miss.material_id = -1;
            miss.hit = 0u;
            hits[F.packed ? pidx : (size_t)y * F.W + x] = miss;
        }
        return;
    }
    LaneCounters cnt;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
    if (RAYCAM) {
        if (active) primary_ray(F.raycams[view], x, y, o, d);
    } else if (active) {
        primary_ray(VIEWS ? F.views[view] : C, F.W, F.H, x, y, o, d);
    }
    float t = 3.402823466e+38f;  // std::numeric_limits<float>::max(), trackball.cpp:101
    uint32_t hit_rec = REF_NONE;
    if (QUAD)
        walk_tree_quad<COUNT>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), cnt);
    else
        walk_tree<COUNT, FAST>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt);
    if (VIEWS) (void)frame_pixel<QUAD, VIEWS>(F, x, y, pidx, writer, &view);  // (rebuilt, not kept through the walk: that cost 12 B of scratch)
    if (active && writer) {
        const size_t pix = VIEWS ? view_pixel(F, view, x, y) : (F.packed ? pidx : (size_t)y * F.W + x);
        finish_ray(S, o, d, t, hit_rec, hits + pix, normals ? normals + 3 * pix : nullptr);
    }
    if (COUNT) flush_counters(cnt, active && writer, counters);
    if (HINT) hint_finish(CGRT_HINT_SCRATCH(s_lds));
    if (STAMP && (threadIdx.x & 63u) == 0u) {  // (single-wave workgroups: the launcher sees to it)
        const uint32_t dt = (uint32_t)__builtin_amdgcn_s_memrealtime() - CGRT_HINT_SCRATCH(s_lds)[0];
        atomicMax(reinterpret_cast<uint32_t*>(counters) + ((blockIdx.x >> 9) * 8u + (blockIdx.x & 7u)), dt);
    }
}

// The order builder (tests/frame_order_ref.py states it in NumPy): from the ticks a profile frame left, per % 8 lane,
// the positions with ticks >= live are LIVE; every other position keeps its own super-tile, and the live super-tiles are dealt to the live
// positions in descending order of ticks, ties by position -- the launch keeps its pattern of heavy and background super-tiles, the
// super-tile with the longest wave starts first, those whose waves are all short start last.  One workgroup per lane, the lane's ticks
// in LDS; a rank sort: the thread of live position p counts the live positions of the lane that go before it in the sorted order (r) and
// in the launch (c), leaves p at by_rank[r], and after a barrier takes by_rank[c] -- the ranks of a lane are distinct, so every slot of
// by_rank and of the table is written exactly once, by one thread.
__global__ __launch_bounds__(256) void k_build_frame_order(const uint32_t* __restrict__ ticks, uint32_t n_pad, uint32_t nst, uint32_t live,
                                                           uint16_t* __restrict__ out) {
    __shared__ uint32_t s_ticks[CGRT_ORDER_MAX_POSITIONS / 8];
    __shared__ uint16_t s_by_rank[CGRT_ORDER_MAX_POSITIONS / 8], s_before[CGRT_ORDER_MAX_POSITIONS / 8];
    const uint32_t lane8 = blockIdx.x, m = n_pad >> 3;  // the lane's positions: lane8 + 8 i, i < m (m <= CGRT_ORDER_MAX_POSITIONS / 8: the launcher)
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
        const uint32_t p = lane8 + 8u * i;
        s_ticks[i] = p < nst ? ticks[p] : 0u;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
        const uint32_t tp = s_ticks[i];
        if (tp < live) continue;
        uint32_t r = 0, c = 0;
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t tq = s_ticks[k];
            const bool lv = tq >= live;
            r += (lv && (tq > tp || (tq == tp && k < i))) ? 1u : 0u;
            c += (lv && k < i) ? 1u : 0u;
        }
        s_by_rank[r] = (uint16_t)(lane8 + 8u * i);
        s_before[i] = (uint16_t)c;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
        const uint32_t p = lane8 + 8u * i;
        out[p] = s_ticks[i] >= live ? s_by_rank[s_before[i]] : (uint16_t)p;
    }
}

// Primary frame for the shading wavefront (cgrt_render): the fused kernel's walk, but only the rays that HIT are written,
// appended to a compact list {ray, hit, normal, pixel} (one atomic per workgroup, lanes ranked by ballot; workgroups
// finish roughly in launch order, so the list keeps the frame's tile order).  Pixels that miss need no further work upstream
// either (main.cpp:293: black).  count = one zeroed device word.
// VIEWS: a multi-view frame (k_trace_primary's VIEWS): camera per view from F.views, pixels (and rgb) at view_pixel.
// RAYCAM (with VIEWS only): ray cameras from F.raycams (k_trace_primary's RAYCAM).
template <bool COUNT, bool FAST, bool QUAD = false, bool VIEWS = false, bool RAYCAM = false>
__global__ CGRT_LB void k_trace_primary_compact(SceneDev S, CameraDev C, FrameDev F, float* __restrict__ rays, CgrtHitDev* __restrict__ hits,
                                                float* __restrict__ normals, int* __restrict__ pixels, uint32_t* __restrict__ count,
                                                unsigned long long* counters, float* __restrict__ rgb, const SpawnDev* __restrict__ spawn_dev) {
    static_assert(VIEWS || !RAYCAM, "ray cameras come from the views table");
    extern __shared__ uint32_t s_lds[];  // CGRT_LDS_WORDS(blockDim.x): stacks, quad-tail owner maps, workgroup scratch
    const int lane = threadIdx.x & 63;
    int x = 0, y = 0;
    size_t pidx;
    bool writer;
    uint32_t view = 0;
    const bool owned = frame_pixel<QUAD, VIEWS>(F, x, y, pidx, writer, &view);
    if (owned && writer && rgb) {  // every pixel this rank owns starts black (main.cpp:293); the hits are written over it at the end of the frame
        float* p = rgb + 3ull * (VIEWS ? view_pixel(F, view, x, y) : (unsigned long long)y * F.W + x);
        p[0] = p[1] = p[2] = 0.0f;
    }
    // A wave outside the frame gate (wave_outside_gate; never the counting and the multi-view instantiations) traces nothing: its pixels
    // miss, and a miss appends nothing.  It stays for the workgroup's count below.
    const bool active = owned && !(!COUNT && !VIEWS && wave_outside_gate(F, owned, x, y));
    LaneCounters cnt;
    CgrtHitDev h;
    h.hit = 0;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0), nn = f3(0, 0, 0);
    if (RAYCAM) {
        if (active) primary_ray(F.raycams[view], x, y, o, d);
    } else if (active) {
        primary_ray(VIEWS ? F.views[view] : C, F.W, F.H, x, y, o, d);
    }
    float t = 3.402823466e+38f;  // std::numeric_limits<float>::max(), trackball.cpp:101
    uint32_t hit_rec = REF_NONE;
    if (QUAD)
        walk_tree_quad<COUNT>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), cnt);
    else
        walk_tree<COUNT, FAST>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt);
    if (active && writer) resolve_hit(S, o, d, t, hit_rec, true, h, nn);
    if (COUNT) flush_counters(cnt, active && writer, counters);
    // one atomic per workgroup (same-address atomics serialise at the L2); the workgroup's LDS is only released when its
    // last wave ends anyway, so waiting for it here costs no occupancy
    const bool keep = active && writer && h.hit != 0;
    // Fused level-0 spawn (a predicted frame, capi_frames.cpp render_impl; k_spawn's work from this lane's registers, spawn_rays.h): does
    // the hit want a mirror ray?  (The parameters are read from device memory HERE: as kernel arguments they were loaded before
    // the walk and their 22 scalar registers pushed the walk into scratch.)
    F3 ks = f3(0.f, 0.f, 0.f);
    bool wants_mirror = false;
    if (spawn_dev && keep) {
        const int mid = h.material_id;
        const float* mats = spawn_dev->materials;
        if (mid >= 0) ks = f3(mats[8 * mid + 3], mats[8 * mid + 4], mats[8 * mid + 5]);
        wants_mirror = !(ks.z <= 0.01f) && spawn_dev->spawn;  // (:246 tests ks.z only; spawn = level + 1 < maxLevel, :267)
    }
    const unsigned long long m = __ballot(keep), mm = __ballot(wants_mirror);
    uint32_t* s_cnt = CGRT_BLOCK_SCRATCH(s_lds);
    const unsigned w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) s_cnt[w] = (uint32_t)__popcll(m) | ((uint32_t)__popcll(mm) << 16);  // (a workgroup has at most 1024 lanes)
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0, mtot = 0;
        for (unsigned k = 0; k < nw; k++) {
            const uint32_t c = s_cnt[k];
            s_cnt[k] = tot | (mtot << 16);
            tot += c & 0xffffu;
            mtot += c >> 16;
        }
        if (!tot) {
            s_cnt[nw] = 0u;
        } else if (spawn_dev) {
            // count[0] = hits, count[1] = mirror rays, ONE 64-bit atomic for both: three more counters of their own (the shadow rays and
            // hits of k_spawn's counter block, the mirror rays) quadrupled the same-line atomics and the Cornell frame's primary
            // kernel went from 70 to 174 us.  (The level's shadow rays are hits x lights: no counter.)
            const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long*>(count), (unsigned long long)tot | ((unsigned long long)mtot << 32));
            s_cnt[nw] = (uint32_t)old;
            s_lds[0] = (uint32_t)(old >> 32);  // (wave 0's stack: its walk is over)
        } else {
            s_cnt[nw] = atomicAdd(count, tot);
        }
    }
    __syncthreads();
    if (keep) {
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long idx = s_cnt[nw] + (s_cnt[w] & 0xffffu) + (uint32_t)__popcll(m & below);
        float* r = rays + 7 * idx;
        r[0] = o.x;
        r[1] = o.y;
        r[2] = o.z;
        r[3] = d.x;
        r[4] = d.y;
        r[5] = d.z;
        r[6] = 3.402823466e+38f;
        hits[idx] = h;
        normals[3 * idx] = nn.x;
        normals[3 * idx + 1] = nn.y;
        normals[3 * idx + 2] = nn.z;
        int px = 0, py = 0;  // (the pixel is rebuilt rather than kept in registers through the walk)
        size_t pi;
        bool wr;
        uint32_t pv = 0;
        (void)frame_pixel<QUAD, VIEWS>(F, px, py, pi, wr, &pv);
        pixels[idx] = VIEWS ? (int)view_pixel(F, pv, px, py) : py * F.W + px;
        if (spawn_dev) {
            // Entry idx's shadow ray towards light l is shadow ray idx * nlights + l (every entry of level 0 is a hit: no append).
            const SpawnDev SP = *spawn_dev;
            const F3 pointOn = add(o, scale(d, h.t));
            for (unsigned l = 0; l < SP.nlights; l++) {
                const unsigned long long q = idx * SP.nlights + l;
                SP.sslot[q] = (int)q;
                spawn_shadow_ray(SP.lights, l, pointOn, q, SP.srays, SP.sdist);
            }
            const uint32_t child = s_lds[0] + (s_cnt[w] >> 16) + (uint32_t)__popcll(mm & below);
            if (wants_mirror) {
                spawn_mirror_ray(pointOn, d, nn, child, SP.next_rays);
                SP.next_pixels[child] = VIEWS ? (int)view_pixel(F, pv, px, py) : py * F.W + px;
            }
            SP.lvl[2 * idx + 1] = make_float4(ks.x, ks.y, ks.z, __int_as_float(wants_mirror ? (int)child : -1));
        }
    }
}
// Level 0 of the shading wavefront from a CALLER's ray list (cgrt_shade_rays): getFinalColor(scene, bvh, ray i) for every i of the
// list (main.cpp:298-310).  The lanes are laid out like k_trace_batch's (the list shapes: quad, sparse or one ray per lane), the walk
// starts from the caller's t as k_trace_batch's does (the reference's `t >= ray.t` rule), and the tail is k_trace_primary_compact's:
// rgb[3i..3i+2] = black for every i (main.cpp:293), the rays that hit appended to level 0's list with pixel = i, ONE atomic per
// workgroup.  The entry keeps the caller's ray as given, t included.  count = one zeroed device word.
template <bool COUNT, bool FAST, bool QUAD = false>
__global__ CGRT_LB void k_trace_list_compact(SceneDev S, const float* __restrict__ in_rays, unsigned long long n, float* __restrict__ rays,
                                             CgrtHitDev* __restrict__ hits, float* __restrict__ normals, int* __restrict__ pixels,
                                             uint32_t* __restrict__ count, unsigned long long* counters, float* __restrict__ rgb, unsigned qrpw) {
    extern __shared__ uint32_t s_lds[];  // CGRT_LDS_WORDS(blockDim.x): stacks, quad-tail owner maps, workgroup scratch
    const int lane = threadIdx.x & 63;
    const bool sparse = !QUAD && qrpw < 64u;  // (see k_trace_batch)
    const unsigned long long i = QUAD ? ((unsigned long long)blockIdx.x * qrpw + (threadIdx.x >> 2))
                                      : (sparse ? (unsigned long long)blockIdx.x * qrpw + threadIdx.x : (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x);
    const bool writer = !QUAD || (threadIdx.x & 3u) == 0u;
    const bool active = i < n && (!QUAD || (threadIdx.x >> 2) < qrpw) && (!sparse || threadIdx.x < qrpw);
    if (active && writer) {  // every ray of the list starts black (main.cpp:293); the hits are written over it at the end
        float* p = rgb + 3ull * i;
        p[0] = p[1] = p[2] = 0.0f;
    }
    LaneCounters cnt;
    CgrtHitDev h;
    h.hit = 0;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0), nn = f3(0, 0, 0);
    float t = 0.0f;
    if (active) {
        const float* r = in_rays + 7 * i;
        o = f3(r[0], r[1], r[2]);
        d = f3(r[3], r[4], r[5]);
        t = r[6];
    }
    uint32_t hit_rec = REF_NONE;
    if (QUAD)
        walk_tree_quad<COUNT>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), cnt);
    else
        walk_tree<COUNT, FAST>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt);
    if (active && writer) resolve_hit(S, o, d, t, hit_rec, true, h, nn);
    if (COUNT) flush_counters(cnt, active && writer, counters);
    const bool keep = active && writer && h.hit != 0;
    const unsigned long long m = __ballot(keep);
    uint32_t* s_cnt = CGRT_BLOCK_SCRATCH(s_lds);
    const unsigned w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) s_cnt[w] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (unsigned k = 0; k < nw; k++) {
            const uint32_t c = s_cnt[k];
            s_cnt[k] = tot;
            tot += c;
        }
        s_cnt[nw] = tot ? atomicAdd(count, tot) : 0u;
    }
    __syncthreads();
    if (keep) {
        const unsigned long long idx = s_cnt[nw] + s_cnt[w] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        // (the ray's index is rebuilt rather than kept in two registers through the walk; its t is read again, the walk moved it)
        const unsigned long long k = QUAD ? ((unsigned long long)blockIdx.x * qrpw + (threadIdx.x >> 2))
                                          : (sparse ? (unsigned long long)blockIdx.x * qrpw + threadIdx.x : (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x);
        float* r = rays + 7 * idx;
        r[0] = o.x;
        r[1] = o.y;
        r[2] = o.z;
        r[3] = d.x;
        r[4] = d.y;
        r[5] = d.z;
        r[6] = in_rays[7 * k + 6];
        hits[idx] = h;
        normals[3 * idx] = nn.x;
        normals[3 * idx + 1] = nn.y;
        normals[3 * idx + 2] = nn.z;
        pixels[idx] = (int)k;
    }
}
// Two lists in ONE launch: a level's shadow list (occlusion queries, k_trace_shadow's body) and its mirror list (closest hits,
// k_trace_batch's body), workgroups dealt alternately so that both are on the chip at once.  A predicted frame (capi_frames.cpp
// render_impl) used to run them on two streams; the event that started the second stream and the wait that joined it again cost
// ~17 us of an idle GPU per frame (profiles/r3_config3.txt) -- one launch on one stream needs neither.  Lane shapes only (64 or 16
// rays per single-wave workgroup, by the host's estimate or on the device: see "kernel shape per launch").
struct ListPairDev {
    const float* rays_a;  // the shadow list
    const float* dist_a;
    CgrtHitDev* hits_a;
    const uint32_t* dcount_a;
    unsigned long long n_a;
    unsigned dmul_a, rpw_a, adapt_a, blocks_a;
    const float* rays_b;  // the mirror list
    CgrtHitDev* hits_b;
    float* normals_b;
    const uint32_t* dcount_b;
    unsigned long long n_b;
    unsigned rpw_b, adapt_b, blocks_b;
};
// one workgroup's rays of the shadow list (a) / the mirror list (b) of k_trace_pair; bid = the workgroup's index within its list
template <bool FAST>
__device__ __forceinline__ void pair_a_wg(const SceneDev& S, const ListPairDev& P, unsigned long long n, unsigned rpw, unsigned long long bid,
                                          uint32_t* s_lds) {
    LaneCounters cnt;
    const unsigned long long i = bid * rpw + threadIdx.x;
    const bool active = i < n && threadIdx.x < rpw;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
    float t = 0.0f, qlen = 0.0f;
    if (active) {
        const float* r = P.rays_a + 7 * i;
        o = f3(r[0], r[1], r[2]);
        d = f3(r[3], r[4], r[5]);
        t = r[6];
        qlen = P.dist_a[i];
    }
    uint32_t hit_rec = REF_NONE;
    walk_tree<false, FAST, WALK_OCCLUDED>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt, qlen);
    if (active) finish_ray(S, o, d, t, hit_rec, P.hits_a + i, nullptr);
}
template <bool FAST>
__device__ __forceinline__ void pair_b_wg(const SceneDev& S, const ListPairDev& P, unsigned long long n, unsigned rpw, unsigned long long bid,
                                          uint32_t* s_lds) {
    LaneCounters cnt;
    const unsigned long long i = bid * rpw + threadIdx.x;
    const bool active = i < n && threadIdx.x < rpw;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
    float t = 0.0f;
    if (active) {
        const float* r = P.rays_b + 7 * i;
        o = f3(r[0], r[1], r[2]);
        d = f3(r[3], r[4], r[5]);
        t = r[6];
    }
    uint32_t hit_rec = REF_NONE;
    walk_tree<false, FAST>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt);
    if (active) finish_ray(S, o, d, t, hit_rec, P.hits_b + i, P.normals_b ? P.normals_b + 3 * i : nullptr);
}
// STRIDED (enqueued frames, capi_frames.cpp enqueue_impl): the grid is capped (P.blocks_a / P.blocks_b workgroups per list, whatever the lists'
// capacities) and each workgroup strides over the entries its list's device count holds, blocks_a (blocks_b) workgroups at a time.
template <bool FAST, bool STRIDED = false>
__global__ CGRT_LB void k_trace_pair(SceneDev S, ListPairDev P) {
    if constexpr (STRIDED) {
        extern __shared__ uint32_t s_lds[];
        const unsigned b = blockIdx.x, both = P.blocks_a < P.blocks_b ? P.blocks_a : P.blocks_b;
        const bool is_a = b < 2u * both ? (b & 1u) == 0u : P.blocks_a > P.blocks_b;
        const unsigned bid = b < 2u * both ? (b >> 1) : b - both;  // the workgroup's first index within its list
        // (as k_trace_batch's: the counts are read again for every pass, only the index lives across a walk)
        for (unsigned k = bid;; k += is_a ? P.blocks_a : P.blocks_b) {
            const uint32_t* dc = is_a ? P.dcount_a : P.dcount_b;
            const unsigned long long cap = is_a ? P.n_a : P.n_b, adapt = is_a ? P.adapt_a : P.adapt_b;
            const unsigned long long present = (unsigned long long)*(const volatile uint32_t*)dc * (is_a ? P.dmul_a : 1u), m = present < cap ? present : cap;
            const unsigned rpw = adapt ? ((m <= adapt) ? 16u : 64u) : (is_a ? P.rpw_a : P.rpw_b);
            if ((unsigned long long)k * rpw >= m) break;
            if (is_a)
                pair_a_wg<FAST>(S, P, m, rpw, k, s_lds);
            else
                pair_b_wg<FAST>(S, P, m, rpw, k, s_lds);
        }
    } else {
    extern __shared__ uint32_t s_lds[];
    const unsigned b = blockIdx.x, both = P.blocks_a < P.blocks_b ? P.blocks_a : P.blocks_b;
    const bool is_a = b < 2u * both ? (b & 1u) == 0u : P.blocks_a > P.blocks_b;
    const unsigned bid = b < 2u * both ? (b >> 1) : b - both;  // the workgroup's index within its list's launch
    LaneCounters cnt;
    if (is_a) {
        unsigned long long n = P.n_a;
        if (P.dcount_a) {
            const unsigned long long present = (unsigned long long)*P.dcount_a * P.dmul_a;
            n = present < n ? present : n;
        }
        unsigned rpw = P.rpw_a;
        if (P.adapt_a) rpw = (n <= P.adapt_a) ? 16u : 64u;
        const unsigned long long i = (unsigned long long)bid * rpw + threadIdx.x;
        const bool active = i < n && threadIdx.x < rpw;
        F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
        float t = 0.0f, qlen = 0.0f;
        if (active) {
            const float* r = P.rays_a + 7 * i;
            o = f3(r[0], r[1], r[2]);
            d = f3(r[3], r[4], r[5]);
            t = r[6];
            qlen = P.dist_a[i];
        }
        uint32_t hit_rec = REF_NONE;
        walk_tree<false, FAST, WALK_OCCLUDED>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt, qlen);
        if (active) finish_ray(S, o, d, t, hit_rec, P.hits_a + i, nullptr);
    } else {
        unsigned long long n = P.n_b;
        if (P.dcount_b) {
            const unsigned long long present = *P.dcount_b;
            n = present < n ? present : n;
        }
        unsigned rpw = P.rpw_b;
        if (P.adapt_b) rpw = (n <= P.adapt_b) ? 16u : 64u;
        const unsigned long long i = (unsigned long long)bid * rpw + threadIdx.x;
        const bool active = i < n && threadIdx.x < rpw;
        F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
        float t = 0.0f;
        if (active) {
            const float* r = P.rays_b + 7 * i;
            o = f3(r[0], r[1], r[2]);
            d = f3(r[3], r[4], r[5]);
            t = r[6];
        }
        uint32_t hit_rec = REF_NONE;
        walk_tree<false, FAST>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt);
        if (active) finish_ray(S, o, d, t, hit_rec, P.hits_b + i, P.normals_b ? P.normals_b + 3 * i : nullptr);
    }
    }
}
// rgb of every pixel this rank owns := 0 (main.cpp:293; the hits are written over it afterwards)
__global__ __launch_bounds__(CGRT_BLOCK) void k_clear_owned(FrameDev F, float* __restrict__ rgb) {
    int x = 0, y = 0;
    if (!tile_pixel_of(F, blockIdx.x, threadIdx.x, x, y)) return;
    float* p = rgb + 3ull * ((unsigned long long)y * F.W + x);
    p[0] = p[1] = p[2] = 0.0f;
}

// one workgroup's rays of k_trace_batch (bid: its index in the launch's layout; qrpw as the kernel has chosen it), for the STRIDED form.
// The one-pass instantiations keep their own copy of this body (calling this helper changed their VGPRs and scratch, measured with
// tools/enqueue_resource_usage.py): the two copies must stay in step.  trace_shadow_wg and pair_a_wg / pair_b_wg likewise.
template <bool COUNT, bool FAST, bool QUAD>
__device__ __forceinline__ void trace_batch_wg(const SceneDev& S, const float* __restrict__ rays, unsigned long long n, CgrtHitDev* __restrict__ hits,
                                               float* __restrict__ normals, unsigned long long* counters, unsigned qrpw, unsigned long long bid,
                                               uint32_t* s_lds) {
    const unsigned long long g = bid * blockDim.x + threadIdx.x;
    const bool sparse = !QUAD && qrpw < 64u;
    const unsigned long long i = QUAD ? (bid * qrpw + (threadIdx.x >> 2)) : (sparse ? bid * qrpw + threadIdx.x : g);
    const bool writer = !QUAD || (threadIdx.x & 3u) == 0u;
    const bool active = i < n && (!QUAD || (threadIdx.x >> 2) < qrpw) && (!sparse || threadIdx.x < qrpw);
    LaneCounters cnt;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
    float t = 0.0f;
    if (active) {
        const float* r = rays + 7 * i;
        o = f3(r[0], r[1], r[2]);
        d = f3(r[3], r[4], r[5]);
        t = r[6];
    }
    uint32_t hit_rec = REF_NONE;
    if (QUAD)
        walk_tree_quad<COUNT>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), cnt);
    else
        walk_tree<COUNT, FAST>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt);
    if (active && writer) {
        // (the ray's index is rebuilt rather than kept in two registers through the walk)
        const unsigned long long k = QUAD ? (bid * qrpw + (threadIdx.x >> 2)) : (sparse ? bid * qrpw + threadIdx.x : bid * blockDim.x + threadIdx.x);
        finish_ray(S, o, d, t, hit_rec, hits + k, normals ? normals + 3 * k : nullptr);
    }
    if (COUNT) flush_counters(cnt, active && writer, counters);
}
// dcount (optional): device word holding the number of rays actually present (<= n); the grid covers n.  The shapes: see the
// comment in the body.
// STRIDED (lane shapes, enqueued frames): the grid is capped instead (capi_frames.cpp enqueue_impl) and each workgroup strides over the rays
// present, gridDim.x workgroups at a time; the rays' layout on the lanes is the one a full grid gives them.
template <bool COUNT, bool FAST, bool QUAD = false, bool STRIDED = false>
__global__ CGRT_LB void k_trace_batch(SceneDev S, const float* __restrict__ rays, unsigned long long n,
                                                            CgrtHitDev* __restrict__ hits, float* __restrict__ normals,
                                                            unsigned long long* counters, const uint32_t* __restrict__ dcount, unsigned qrpw, unsigned adapt_max) {
    static_assert(!(STRIDED && (QUAD || COUNT)), "strided launches are lane-shaped and uncounted");
    if constexpr (STRIDED) {
        extern __shared__ uint32_t s_lds[];
        // (the count is read again for every pass and nothing but the workgroup index lives across a walk: the walk needs every register)
        for (unsigned b = blockIdx.x;; b += gridDim.x) {
            const unsigned long long present = *(const volatile uint32_t*)dcount, m = present < n ? present : n;
            const unsigned rpw = adapt_max ? ((m <= adapt_max) ? 16u : 64u) : qrpw;
            if ((unsigned long long)b * (rpw < 64u ? rpw : blockDim.x) >= m) break;
            trace_batch_wg<false, FAST, false>(S, rays, m, hits, normals, counters, rpw, b, s_lds);
        }
    } else {
    extern __shared__ uint32_t s_lds[];  // CGRT_LDS_WORDS(blockDim.x): stacks, quad-tail owner maps, workgroup scratch
    if (dcount) {
        const unsigned long long present = *dcount;
        n = present < n ? present : n;
    }
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    // quad shape: the four lanes of a quad carry the same ray; a wave carries qrpw rays (16, or 4: the wide tail from the start)
    // lane shape: one ray per lane; a SPARSE launch (single-wave workgroups with qrpw < 64 rays each) leaves the upper lanes of every
    // wave empty, so that a wave of <= 16 rays runs the quad tail (four lanes per ray, four stack entries in flight) from its
    // first step.  adapt_max (lists whose length only the device knows): sparse iff that length is at most adapt_max -- the grid
    // covers both layouts.
    if (!QUAD && adapt_max) qrpw = (n <= adapt_max) ? 16u : 64u;
    const bool sparse = !QUAD && qrpw < 64u;
    const unsigned long long i = QUAD ? ((unsigned long long)blockIdx.x * qrpw + (threadIdx.x >> 2)) : (sparse ? (unsigned long long)blockIdx.x * qrpw + threadIdx.x : g);
    const bool writer = !QUAD || (threadIdx.x & 3u) == 0u;
    const bool active = i < n && (!QUAD || (threadIdx.x >> 2) < qrpw) && (!sparse || threadIdx.x < qrpw);
    LaneCounters cnt;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
    float t = 0.0f;
    if (active) {
        const float* r = rays + 7 * i;
        o = f3(r[0], r[1], r[2]);
        d = f3(r[3], r[4], r[5]);
        t = r[6];
    }
    uint32_t hit_rec = REF_NONE;
    if (QUAD)
        walk_tree_quad<COUNT>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), cnt);
    else
        walk_tree<COUNT, FAST>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt);
    if (active && writer) {
        // (the ray's index is rebuilt rather than kept in two registers through the walk)
        const unsigned long long k = QUAD ? ((unsigned long long)blockIdx.x * qrpw + (threadIdx.x >> 2))
                                          : (sparse ? (unsigned long long)blockIdx.x * qrpw + threadIdx.x : (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x);
        finish_ray(S, o, d, t, hit_rec, hits + k, normals ? normals + 3 * k : nullptr);
    }
    if (COUNT) flush_counters(cnt, active && writer, counters);
    }
}

// pointInShadow's rays (main.cpp:104-135) for the shading wavefront: dist[i] = |fromPosToLight| of ray i.  The caller only
// evaluates `hit && !(t + epsilon >= dist)`: the certified walk answers that question directly (WALK_OCCLUDED: bounded by
// the light's distance, stops at the first qualifying triangle); a ray without certificate gets the exact closest hit.
// hits[i] therefore holds a hit that decides the test like the reference's own, not necessarily the closest one.
template <bool COUNT, bool FAST, bool QUAD>
__device__ __forceinline__ void trace_shadow_wg(const SceneDev& S, const float* __restrict__ rays, const float* __restrict__ dist, unsigned long long n,
                                                CgrtHitDev* __restrict__ hits, unsigned long long* counters, unsigned qrpw, unsigned long long bid,
                                                uint32_t* s_lds) {
    const unsigned long long g = bid * blockDim.x + threadIdx.x;
    const bool sparse = !QUAD && qrpw < 64u;
    const unsigned long long i = QUAD ? (bid * qrpw + (threadIdx.x >> 2)) : (sparse ? bid * qrpw + threadIdx.x : g);
    const bool writer = !QUAD || (threadIdx.x & 3u) == 0u;
    const bool active = i < n && (!QUAD || (threadIdx.x >> 2) < qrpw) && (!sparse || threadIdx.x < qrpw);
    LaneCounters cnt;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
    float t = 0.0f, qlen = 0.0f;
    if (active) {
        const float* r = rays + 7 * i;
        o = f3(r[0], r[1], r[2]);
        d = f3(r[3], r[4], r[5]);
        t = r[6];
        qlen = dist[i];
    }
    uint32_t hit_rec = REF_NONE;
    if (QUAD)
        walk_tree_quad<COUNT, WALK_OCCLUDED>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), cnt, qlen);
    else
        walk_tree<COUNT, FAST, WALK_OCCLUDED>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt, qlen);
    if (active && writer) finish_ray(S, o, d, t, hit_rec, hits + i, nullptr);
    if (COUNT) flush_counters(cnt, active && writer, counters);
}
// STRIDED: as k_trace_batch's.
template <bool COUNT, bool FAST, bool QUAD = false, bool STRIDED = false>
__global__ CGRT_LB void k_trace_shadow(SceneDev S, const float* __restrict__ rays, const float* __restrict__ dist, unsigned long long n,
                                       CgrtHitDev* __restrict__ hits, const uint32_t* __restrict__ dcount, unsigned long long* counters, unsigned qrpw, unsigned adapt_max,
                                       unsigned dmul) {
    static_assert(!(STRIDED && (QUAD || COUNT)), "strided launches are lane-shaped and uncounted");
    if constexpr (STRIDED) {
        extern __shared__ uint32_t s_lds[];
        for (unsigned b = blockIdx.x;; b += gridDim.x) {  // (as k_trace_batch's)
            const unsigned long long present = (unsigned long long)*(const volatile uint32_t*)dcount * dmul, m = present < n ? present : n;
            const unsigned rpw = adapt_max ? ((m <= adapt_max) ? 16u : 64u) : qrpw;
            if ((unsigned long long)b * (rpw < 64u ? rpw : blockDim.x) >= m) break;
            trace_shadow_wg<false, FAST, false>(S, rays, dist, m, hits, counters, rpw, b, s_lds);
        }
    } else {
    extern __shared__ uint32_t s_lds[];
    if (dcount) {  // dmul: *dcount counts the entries whose shadow rays these are, dmul rays (lights) each
        const unsigned long long present = (unsigned long long)*dcount * dmul;
        n = present < n ? present : n;
    }
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (!QUAD && adapt_max) qrpw = (n <= adapt_max) ? 16u : 64u;  // (see k_trace_batch)
    const bool sparse = !QUAD && qrpw < 64u;
    const unsigned long long i = QUAD ? ((unsigned long long)blockIdx.x * qrpw + (threadIdx.x >> 2)) : (sparse ? (unsigned long long)blockIdx.x * qrpw + threadIdx.x : g);
    const bool writer = !QUAD || (threadIdx.x & 3u) == 0u;
    const bool active = i < n && (!QUAD || (threadIdx.x >> 2) < qrpw) && (!sparse || threadIdx.x < qrpw);
    LaneCounters cnt;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
    float t = 0.0f, qlen = 0.0f;
    if (active) {
        const float* r = rays + 7 * i;
        o = f3(r[0], r[1], r[2]);
        d = f3(r[3], r[4], r[5]);
        t = r[6];
        qlen = dist[i];
    }
    uint32_t hit_rec = REF_NONE;
    if (QUAD)
        walk_tree_quad<COUNT, WALK_OCCLUDED>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), cnt, qlen);
    else
        walk_tree<COUNT, FAST, WALK_OCCLUDED>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt, qlen);
    if (active && writer) finish_ray(S, o, d, t, hit_rec, hits + i, nullptr);
    if (COUNT) flush_counters(cnt, active && writer, counters);
    }
}

// Visibility queries of a caller's (include/cgrt.h cgrt_occluded*, cgrt_in_shadow*): ONE answer byte per query, written by the lane (or
// quad leader) that owns it -- a wave of 64 queries writes 64 consecutive bytes.  The lanes are laid out like k_trace_batch's (the list
// shapes: quad, sparse or one query per lane); no answer depends on the shape.
//   POINTS = false: query g is the ray src[7 g ..] as given, its t included; out[g] = the bool BoundingVolumeHierarchy::intersect returns
//       (bvh.cpp:850-881).  The meshes are searched with WALK_ANYHIT (k_soft_shadow's argument: the flag of the first accepting leaf is
//       the reference's flag), the spheres only when no mesh accepted a triangle (bvh.cpp:875-880: the bool is true either way).
//   POINTS = true: query g = i * nlights + l is pointInShadow(src[3 i ..], light l) (main.cpp:104-135): the ray is built in registers by
//       the frame's expressions (spawn_rays.h shadow_ray), walked as k_trace_shadow walks it (WALK_OCCLUDED bounded by |fromPosToLight|,
//       spheres as finish_ray tests them), and out[g] = k_shade's verdict `hit && !(t + 0.001f >= dist)`.
template <bool POINTS, bool FAST, bool QUAD = false>
__global__ CGRT_LB void k_visibility(SceneDev S, const float* __restrict__ src, const float* __restrict__ lights, unsigned nlights, unsigned long long n,
                                     uint8_t* __restrict__ out, unsigned qrpw) {
    extern __shared__ uint32_t s_lds[];  // CGRT_LDS_WORDS(blockDim.x): stacks, quad-tail owner maps, workgroup scratch
    const bool sparse = !QUAD && qrpw < 64u;  // (see k_trace_batch)
    const unsigned long long i = QUAD ? ((unsigned long long)blockIdx.x * qrpw + (threadIdx.x >> 2))
                                      : (sparse ? (unsigned long long)blockIdx.x * qrpw + threadIdx.x : (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x);
    const bool writer = !QUAD || (threadIdx.x & 3u) == 0u;
    const bool active = i < n && (!QUAD || (threadIdx.x >> 2) < qrpw) && (!sparse || threadIdx.x < qrpw);
    LaneCounters cnt;
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
    float t = 0.0f, qlen = 0.0f;
    if (active) {
        if (POINTS) {
            const unsigned long long p = i / nlights;
            const float* q = src + 3 * p;
            shadow_ray(lights, (unsigned)(i - p * nlights), f3(q[0], q[1], q[2]), o, d, qlen);
            t = 3.402823466e+38f;
        } else {
            const float* r = src + 7 * i;
            o = f3(r[0], r[1], r[2]);
            d = f3(r[3], r[4], r[5]);
            t = r[6];
        }
    }
    uint32_t hit_rec = REF_NONE;
    constexpr int MODE = POINTS ? WALK_OCCLUDED : WALK_ANYHIT;
    if (QUAD)
        walk_tree_quad<false, MODE>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), cnt, qlen);
    else
        walk_tree<false, FAST, MODE>(S, active, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt, qlen);
    if (active && writer) {
        // (the query's index is rebuilt rather than kept in two registers through the walk; n <= 0x7fffffff)
        const uint32_t k = QUAD ? blockIdx.x * qrpw + (threadIdx.x >> 2) : (sparse ? blockIdx.x * qrpw + threadIdx.x : blockIdx.x * blockDim.x + threadIdx.x);
        bool v;
        if (POINTS) {
            CgrtHitDev h;
            F3 nn;
            resolve_hit(S, o, d, t, hit_rec, false, h, nn);
            const uint32_t p = k / nlights;  // (|fromPosToLight| is computed again rather than kept through the walk)
            const float* q = src + 3ull * p;
            F3 o2, d2;
            float dist;
            shadow_ray(lights, k - p * nlights, f3(q[0], q[1], q[2]), o2, d2, dist);
            v = h.hit && !(h.t + CGRT_SHADOW_EPS >= dist);  // k_shade, main.cpp:118-130
        } else {
            v = hit_rec != REF_NONE;
            if (!v) {
                for (uint32_t s = 0; s < S.nspheres; s++) {
                    F3 nrm;
                    v |= ray_sphere(f3(S.spheres[s].c[0], S.spheres[s].c[1], S.spheres[s].c[2]), S.spheres[s].radius, o, d, t, nrm);
                }
            }
        }
        out[k] = v ? 1u : 0u;
    }
}

// Soft shadows of spherical lights (main.cpp:168-218): `samples` shadow rays per (hit item, light), generated in
// registers from the item's ray + hit and the unit-vector table (no ray buffer: 200 samples x 2 M hits would be 12 GB),
// traversed, and counted: lit[item * nlights + l] = number of samples with !intersect || ray.t > lightT (:183-199).
// Thread g = (item * nlights + l) * samples + smp: a wave's rays leave one or two surface points towards one small
// sphere, the most coherent batch this library sees.  ANYHIT stops a ray at its first accepting leaf: the count needs
// the hit flag only (an accepted t is below lightT by construction, or 0 from the on-plane rule, never above).
// POINTS: the items are the caller's points (cgrt_soft_lit*): `rays` holds 3 floats per item, pointOn = that point, every item is live and
// samples as pixel = item (hits and item_pixels are not read).
// VIEWS: the items belong to a multi-view frame, whose pixels are view * W * H + (in-view pixel): samples are drawn with the in-view
// pixel item_pixels[item] % Q.view_pixels, so that every view draws what its single-camera frame draws.
// SETS (k_soft_shadow_sets, light sets): light l is a distinct key of the batch and draws as light Q.set_index[l], its index within its
// own set, so that every set draws what its single frame draws.
// thread g of k_soft_shadow's layout (every lane of the wave calls it: the counts are aggregated per wave)
template <bool ANYHIT, bool FAST, bool POINTS, bool VIEWS, bool SETS = false>
__device__ __forceinline__ void soft_shadow_thread(const SceneDev& S, const SoftDev& Q, const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                   const int* __restrict__ item_pixels, unsigned long long g, unsigned long long nthreads,
                                                   uint32_t* __restrict__ lit, uint32_t* s_lds) {
    const bool in = g < nthreads;
    const unsigned long long key = in ? g / Q.samples : 0ull;  // item * nlights + l
    const uint32_t smp = in ? (uint32_t)(g - key * Q.samples) : 0u;
    const unsigned long long item = key / Q.nlights;
    const uint32_t l = (uint32_t)(key - item * Q.nlights);
    bool is_lit = false;
    const bool live = in && (POINTS || hits[item].hit != 0);
    F3 o = f3(0, 0, 0), d = f3(0, 0, 0);
    float t = 0.0f;
    if (live) {
        F3 pointOn;
        uint32_t pixel;
        if (POINTS) {
            const float* p = rays + 3 * item;
            pointOn = f3(p[0], p[1], p[2]);
            pixel = (uint32_t)item;
        } else {
            const float* r = rays + 7 * item;
            pointOn = add(f3(r[0], r[1], r[2]), scale(f3(r[3], r[4], r[5]), hits[item].t));
            pixel = (uint32_t)item_pixels[item];
            if (VIEWS) pixel %= Q.view_pixels;
        }
        const float* L = Q.lights + 7 * l;
        const float* u = Q.units + 3ull * soft_sample_index(Q.seed, pixel, Q.level, SETS ? Q.set_index[l] : l, smp, Q.nunits);
        soft_shadow_ray(pointOn, f3(L[0], L[1], L[2]), L[3], f3(u[0], u[1], u[2]), o, d, t);
    }
    const float lightT = t;
    uint32_t hit_rec = REF_NONE;
    LaneCounters cnt;
    walk_tree<false, FAST, ANYHIT ? WALK_ANYHIT : WALK_CLOSEST>(S, live, o, d, t, hit_rec, CGRT_WAVE_STACK(s_lds), CGRT_WAVE_MAP(s_lds), cnt);
    if (live) {
        bool hit = hit_rec != REF_NONE;
        if (!ANYHIT || !hit) {  // spheres come after the meshes in BoundingVolumeHierarchy::intersect (bvh.cpp:875-880)
            for (uint32_t k = 0; k < S.nspheres; k++) {
                F3 nrm;
                hit |= ray_sphere(f3(S.spheres[k].c[0], S.spheres[k].c[1], S.spheres[k].c[2]), S.spheres[k].radius, o, d, t, nrm);
            }
        }
        is_lit = !hit || t > lightT;
    }
    // one atomic per (wave, key): a wave's keys are consecutive
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const unsigned long long k0 = __shfl(key, first);
        const unsigned long long same = __ballot(live && key == k0);
        const uint32_t c = (uint32_t)__popcll(__ballot(live && key == k0 && is_lit));
        if ((int)(threadIdx.x & 63) == first && c) atomicAdd(lit + k0, c);
        todo &= ~same;
    }
}
template <bool ANYHIT, bool FAST, bool POINTS = false, bool VIEWS = false>
__global__ CGRT_LB void k_soft_shadow(SceneDev S, SoftDev Q, const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                      const int* __restrict__ item_pixels, unsigned long long nthreads, uint32_t* __restrict__ lit) {
    extern __shared__ uint32_t s_lds[];  // CGRT_LDS_WORDS(blockDim.x): stacks, quad-tail owner maps, workgroup scratch
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    soft_shadow_thread<ANYHIT, FAST, POINTS, VIEWS>(S, Q, rays, hits, item_pixels, g, nthreads, lit, s_lds);
}
// k_soft_shadow with the SETS flag (a kernel of its own: the instantiations above keep their names and their code)
template <bool ANYHIT, bool FAST>
__global__ CGRT_LB void k_soft_shadow_sets(SceneDev S, SoftDev Q, const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                           const int* __restrict__ item_pixels, unsigned long long nthreads, uint32_t* __restrict__ lit) {
    extern __shared__ uint32_t s_lds[];
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    soft_shadow_thread<ANYHIT, FAST, false, false, true>(S, Q, rays, hits, item_pixels, g, nthreads, lit, s_lds);
}
// k_soft_shadow_sets for a multi-view batch of light sets (cgrt_render_views_light_sets*): VIEWS and SETS together -- sample smp of a key
// draws with the in-view pixel and the key's in-set index, as the single frame of that view under that set draws it
template <bool ANYHIT, bool FAST>
__global__ CGRT_LB void k_soft_shadow_views_sets(SceneDev S, SoftDev Q, const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                 const int* __restrict__ item_pixels, unsigned long long nthreads, uint32_t* __restrict__ lit) {
    extern __shared__ uint32_t s_lds[];
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    soft_shadow_thread<ANYHIT, FAST, false, true, true>(S, Q, rays, hits, item_pixels, g, nthreads, lit, s_lds);
}
// The count-driven form (enqueued frames): the level's items are the first *dcount (<= nitems, the list's capacity) entries, known only on
// the device; a capped grid strides over their present x nlights x samples threads, gridDim.x * blockDim.x at a time.  Thread g draws
// and counts what it draws in k_soft_shadow: the draws hash the pixel and the level, never the grid.
template <bool ANYHIT, bool FAST, bool VIEWS>
__global__ CGRT_LB void k_soft_shadow_strided(SceneDev S, SoftDev Q, const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                              const int* __restrict__ item_pixels, unsigned long long nitems, const uint32_t* __restrict__ dcount,
                                              uint32_t* __restrict__ lit) {
    extern __shared__ uint32_t s_lds[];
    for (unsigned b = blockIdx.x;; b += gridDim.x) {  // (as k_trace_batch's: only the index lives across a walk)
        const unsigned long long present = *(const volatile uint32_t*)dcount;
        const unsigned long long nthreads = (present < nitems ? present : nitems) * Q.nlights * Q.samples, base = (unsigned long long)b * blockDim.x;
        if (base >= nthreads) break;
        soft_shadow_thread<ANYHIT, FAST, false, VIEWS>(S, Q, rays, hits, item_pixels, base + threadIdx.x, nthreads, lit, s_lds);
    }
}
// k_soft_shadow_strided for an enqueued batch of light sets (always a multi-view batch, one view or more): k_soft_shadow_views_sets' threads
template <bool ANYHIT, bool FAST>
__global__ CGRT_LB void k_soft_shadow_sets_strided(SceneDev S, SoftDev Q, const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                   const int* __restrict__ item_pixels, unsigned long long nitems, const uint32_t* __restrict__ dcount,
                                                   uint32_t* __restrict__ lit) {
    extern __shared__ uint32_t s_lds[];
    for (unsigned b = blockIdx.x;; b += gridDim.x) {
        const unsigned long long present = *(const volatile uint32_t*)dcount;
        const unsigned long long nthreads = (present < nitems ? present : nitems) * Q.nlights * Q.samples, base = (unsigned long long)b * blockDim.x;
        if (base >= nthreads) break;
        soft_shadow_thread<ANYHIT, FAST, false, true, true>(S, Q, rays, hits, item_pixels, base + threadIdx.x, nthreads, lit, s_lds);
    }
}

__global__ __launch_bounds__(CGRT_BLOCK) void k_generate_rays(CameraDev C, int W, int H, int x0, int y0, int x1, int y1,
                                                              float* __restrict__ rays) {
    const unsigned long long i = (unsigned long long)blockIdx.x * CGRT_BLOCK + threadIdx.x;
    const int rw = x1 - x0;
    const unsigned long long n = (unsigned long long)rw * (unsigned long long)(y1 - y0);
    if (i >= n) return;
    const int x = x0 + (int)(i % (unsigned long long)rw), y = y0 + (int)(i / (unsigned long long)rw);
    F3 o, d;
    primary_ray(C, W, H, x, y, o, d);
    float* r = rays + 7 * i;
    r[0] = o.x;
    r[1] = o.y;
    r[2] = o.z;
    r[3] = d.x;
    r[4] = d.y;
    r[5] = d.z;
    r[6] = 3.402823466e+38f;
}
// k_generate_rays for a ray camera (cgrt_generate_rays_raycam): the whole W x H frame, row-major.
__global__ __launch_bounds__(CGRT_BLOCK) void k_generate_rays_raycam(RayCameraDev C, int W, int H, float* __restrict__ rays) {
    const unsigned long long i = (unsigned long long)blockIdx.x * CGRT_BLOCK + threadIdx.x;
    const unsigned long long n = (unsigned long long)W * (unsigned long long)H;
    if (i >= n) return;
    F3 o, d;
    primary_ray(C, (int)(i % (unsigned long long)W), (int)(i / (unsigned long long)W), o, d);
    float* r = rays + 7 * i;
    r[0] = o.x;
    r[1] = o.y;
    r[2] = o.z;
    r[3] = d.x;
    r[4] = d.y;
    r[5] = d.z;
    r[6] = 3.402823466e+38f;
}
// ---------------------------------------------------------------------------------------------
// launchers (host).  A scene with a fast tree (SceneDev::fast_root) takes the FAST instantiations; the C-ABI clears
// fast_root in its copy of SceneDev to force the exact walk (cgrt_scene_set_walk).  Workgroup size: FrameDev::block for
// frames, trace_block() for ray lists -- 64 threads (one wave, its LDS released the moment it ends) for the certified walk,
// whose waves differ widely in length; 256 for the exact walk (measured: profiles/r2_exp_block_size.txt).
// ---------------------------------------------------------------------------------------------
static inline unsigned grid_for(unsigned long long n, unsigned block) { return (unsigned)((n + block - 1) / block); }
static inline size_t lds_bytes(unsigned block) { return sizeof(uint32_t) * (size_t)CGRT_LDS_WORDS(block); }
int trace_block(const SceneDev& S) {
    static const int forced = [] {
        const char* e = getenv("CGRT_BLOCK_THREADS");  // experiment knob: 64 / 128 / 256
        const int v = e ? atoi(e) : 0;
        return (v == 64 || v == 128 || v == 256) ? v : 0;
    }();
    if (forced) return forced;
    return S.fast_root != REF_NONE ? 64 : 256;
}
// From run-time bools to template arguments: f(std::true_type) or f(std::false_type), so that a generic lambda names its kernel as
// k<decltype(B)::value, ..>.  A lambda instantiates what it names for both values: `if constexpr` keeps out the combinations no launch
// takes (quad shapes only FAST, STRIDED only uncounted lane shapes, HINT only <false, true, false, true>).
template <class F>
static inline void with_bool(bool b, F&& f) {
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}
template <class F>
static inline void with_bools(bool a, bool b, F&& f) {
    with_bool(a, [&](auto A) { with_bool(b, [&](auto B) { f(A, B); }); });
}
// every traversal kernel takes the LDS of its workgroup size (CGRT_LDS_WORDS)
template <class K, class... A>
static inline void launch(K kernel, unsigned grid, unsigned block, hipStream_t stream, const A&... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes(block), stream, args...);
}

// ---- kernel shape per launch ----
// How a launch lays its rays out on the lanes (results never depend on it; tests/test_quad_shape_gpu.py):
//   LANE64  one ray per lane, 64 per wave: the throughput shape (walk_fast.h), every frame and every large list;
//   LANE16  one ray per lane, 16 rays per single-wave workgroup: the wave is in the quad tail -- four lanes per ray, four stack
//           entries in flight -- from its first step, and a hard ray shares its wave with 15 others instead of 63;
//   QUAD4   four rays per wave, a row of 16 lanes each: four stack entries x four child boxes per round (walk_quad.h);
//   QUAD16  quad per ray, 16 rays per wave (walk_quad.h's basic shape; never chosen by size, kept selectable).
// A launch ends when its hardest rays end, and a hard ray is a dependent chain that gets ~2x faster when it does not share its
// wave's bodies with 63 others (profiles/r3_exp_list_shapes.txt: 64 hard rays 97 us as one wave, 51 us as four, 45 us as
// sixteen) -- but sparse waves cost throughput, so the shape goes by the number of rays: <= g_quad4_max -> QUAD4,
// <= g_lane16_max -> LANE16, else LANE64 (crossovers measured: 4 K rays 75 / 49 / 46 us, 16 K 84 / 56 / 60, 64 K 94 / 79 / 136,
// 255 K 126 / 142 / 372 for LANE64 / LANE16 / QUAD4).  Lists whose length only the device knows (cgrt_render's wavefront) choose
// between LANE64 and LANE16 on the device (adapt_max).  Frames keep LANE64: 71 % of a frame's waves die at the root gate and a
// sparse shape pays its per-wave set-up four times for them (share of a 4K frame: 94 us -> 151 us, profiles/r3_exp_quad_shape.txt).
enum { SHAPE_AUTO = -1, SHAPE_LANE64 = 0, SHAPE_QUAD16 = 1, SHAPE_LANE16 = 2, SHAPE_QUAD4 = 3 };
static std::atomic<int> g_shape_mode{SHAPE_AUTO};
static std::atomic<unsigned long long> g_lane16_max{CGRT_LANE16_MAX_RAYS_DEFAULT};
static std::atomic<unsigned long long> g_quad4_max{CGRT_QUAD4_MAX_RAYS_DEFAULT};
void set_quad_shape(int mode, unsigned long long max_rays) {
    g_shape_mode.store((mode < 0 || mode > 3) ? SHAPE_AUTO : mode);
    if (max_rays) {
        g_lane16_max.store(max_rays);
        g_quad4_max.store(std::min<unsigned long long>(max_rays, CGRT_QUAD4_MAX_RAYS_DEFAULT));
    }
}
void get_quad_shape(int* mode, unsigned long long* max_rays) {
    *mode = g_shape_mode.load();
    *max_rays = g_lane16_max.load();
}
static int shape_mode() {
    static const int env_mode = [] {
        const char* e = getenv("CGRT_SHAPE");  // experiment knob: -1 auto / 0 lane64 / 1 quad16 / 2 lane16 / 3 quad4
        return e ? atoi(e) : -2;
    }();
    return env_mode != -2 ? env_mode : g_shape_mode.load();
}
static unsigned long long env_ull(const char* name) {
    const char* e = getenv(name);
    return e ? strtoull(e, nullptr, 10) : 0ull;
}
// shape of a ray LIST of n rays (n known to the host)
static int list_shape(const SceneDev& S, unsigned long long n) {
    if (S.fast_root == REF_NONE || trace_block(S) != 64) return SHAPE_LANE64;
    const int mode = shape_mode();
    if (mode != SHAPE_AUTO) return mode;
    static const unsigned long long e16 = env_ull("CGRT_LANE16_MAX"), e4 = env_ull("CGRT_QUAD4_MAX");
    if (n <= (e4 ? e4 : g_quad4_max.load())) return SHAPE_QUAD4;
    if (n <= (e16 ? e16 : g_lane16_max.load())) return SHAPE_LANE16;
    return SHAPE_LANE64;
}
// lists sized on the device: 0 = the host's choice stands, else "LANE16 iff the device count is at most this"
static unsigned list_adapt_max(const SceneDev& S, const uint32_t* dcount) {
    if (!dcount || S.fast_root == REF_NONE || trace_block(S) != 64 || shape_mode() != SHAPE_AUTO) return 0u;
    static const unsigned long long e16 = env_ull("CGRT_LANE16_MAX");
    return (unsigned)std::min<unsigned long long>(e16 ? e16 : g_lane16_max.load(), 0x7fffffffull);
}
bool quad_shape_for(const SceneDev& S, unsigned long long rays) {  // frames: the quad shape only when forced
    (void)rays;
    return S.fast_root != REF_NONE && trace_block(S) == 64 && shape_mode() == SHAPE_QUAD16;
}
// grid of a list launch in the lane shapes: covers 64 rays per workgroup, and 16 per workgroup up to the adaptive bound
static unsigned lane_grid(unsigned long long n, unsigned block, unsigned rpw, unsigned adapt_max) {
    if (adapt_max) return std::max(grid_for(n, block), grid_for(std::min<unsigned long long>(n, adapt_max), 16));
    return grid_for(n, rpw < 64u ? rpw : block);
}
// ---- capped, count-driven grids (GRID_STRIDED; enqueued frames: capi_frames.cpp enqueue_impl) ----
// Every list of an enqueued frame is sized for the worst case and only the device knows its length, so a launch covers at most
// strided_waves() waves, whatever the capacity, and its workgroups stride over the entries present (the STRIDED instantiations).
// The default is twice the walk waves the chip holds at once (256 CUs x 4 SIMDs x 3 waves); CGRT_STRIDED_WAVES overrides it.
unsigned strided_waves() {
    static const unsigned w = [] {
        const unsigned long long e = env_ull("CGRT_STRIDED_WAVES");
        return (e >= 64 && e <= (1ull << 24)) ? (unsigned)e : (unsigned)CGRT_STRIDED_WAVES_DEFAULT;
    }();
    return w;
}
unsigned strided_blocks(unsigned full, unsigned block) {
    const unsigned cap = std::max(1u, strided_waves() / (block / 64u));
    return std::min(full, cap);
}
// ---- the plan of a list launch: everything the rules above derive from a list of capacity n ----
// expected (with dcount): the host's estimate of *dcount picks the shape, as an exact length would, and switches adapt off.  GRID_STRIDED
// ignores it, caps the grid and selects the STRIDED instantiation -- but a quad shape (forced: a checking tool) keeps the full-capacity
// grid of the quad kernel.  pair (k_trace_pair): one list of the two, 64-thread workgroups, and a quad shape of a short list becomes 16
// rays per wave.
struct ListPlan {
    bool quad;      // QUAD4 / QUAD16: the <.., true, true> instantiation, single-wave workgroups of qrpw rays
    bool strided;   // the STRIDED instantiation, its grid capped
    bool fast;      // the scene has a fast tree
    unsigned qrpw;  // rays per wave: 4 or 16 (quad), 16 or 64 (lane)
    unsigned adapt;  // list_adapt_max: LANE16 or LANE64 is chosen on the device (then the host's shape is LANE64)
    unsigned block, grid;
};
static ListPlan plan_list(const SceneDev& S, unsigned long long n, const uint32_t* dcount, unsigned long long expected, ListGrid grid,
                          bool pair = false) {
    ListPlan p{};
    if (grid == GRID_STRIDED) expected = 0;
    p.fast = S.fast_root != REF_NONE;
    p.adapt = expected ? 0u : list_adapt_max(S, dcount);
    const int shape = p.adapt ? SHAPE_LANE64 : list_shape(S, expected ? expected : n);
    p.quad = !pair && (shape == SHAPE_QUAD16 || shape == SHAPE_QUAD4);
    if (p.quad) {
        p.qrpw = shape == SHAPE_QUAD4 ? 4u : 16u;
        p.block = 64u;
        p.grid = grid_for(n, p.qrpw);
        return p;
    }
    p.qrpw = shape == SHAPE_LANE64 ? 64u : 16u;
    p.block = pair ? 64u : (unsigned)trace_block(S);
    p.grid = lane_grid(n, p.block, p.qrpw, p.adapt);
    p.strided = grid == GRID_STRIDED;
    if (p.strided) p.grid = strided_blocks(p.grid, p.block);
    return p;
}
template <class K, class... A>
static inline void launch(K kernel, const ListPlan& p, hipStream_t stream, const A&... args) {
    launch(kernel, p.grid, p.block, stream, args...);
}
// a frame's grid: F.nblocks workgroups of F.block threads, or -- the quad shape, when forced -- four single-wave workgroups for each
struct FramePlan {
    bool quad, fast;
    unsigned grid, block;
};
static FramePlan plan_frame(const SceneDev& S, const FrameDev& F) {
    const bool quad = F.block == 64 && quad_shape_for(S, (unsigned long long)F.nblocks * 64ull);
    return FramePlan{quad, S.fast_root != REF_NONE, quad ? 4u * F.nblocks : F.nblocks, quad ? 64u : (unsigned)F.block};
}

hipError_t launch_trace_primary(const SceneDev& S, const CameraDev& C, const FrameDev& F, CgrtHitDev* hits, float* normals,
                                unsigned long long* counters, hipStream_t stream) {
    if (F.nblocks == 0) return hipSuccess;
    const FramePlan p = plan_frame(S, F);
    const bool hint = !p.quad && F.hint && p.fast && F.block == 64 && !counters;  // frame hints: the hard list's workgroups come first
    const bool order = !p.quad && !hint && F.order && p.fast && F.block == 64 && !counters;  // order table (else: the table is not read)
    with_bools(counters != nullptr, p.fast, [&](auto count, auto fast) {
        constexpr bool COUNT = decltype(count)::value, FAST = decltype(fast)::value;
        auto go = [&](auto kernel, unsigned grid) { launch(kernel, grid, p.block, stream, S, C, F, hits, normals, counters); };
        if constexpr (FAST) {
            if (p.quad) return go(k_trace_primary<COUNT, true, true>, p.grid);
            if constexpr (!COUNT) {
                if (hint) return go(k_trace_primary<false, true, false, true>, F.nblocks + F.hint_blocks);
                if (order) return go(k_trace_primary<false, true, false, false, false, false, true>, p.grid);
            }
        }
        go(k_trace_primary<COUNT, FAST>, p.grid);
    });
    return hipGetLastError();
}
// A profile frame (k_trace_primary's STAMP): the plain frame of single-wave workgroups on a scene with a fast tree, no table; ticks =
// ((nst_rank + 7) / 8) * 8 device words, zeroed here on the launch's stream.  false: the launch is not of that kind (nothing was issued).
bool can_profile_frame(const SceneDev& S, const FrameDev& F) {
    return F.nblocks != 0 && F.block == 64 && !F.hint && !F.packed && S.fast_root != REF_NONE && !plan_frame(S, F).quad;
}
hipError_t launch_trace_primary_profile(const SceneDev& S, const CameraDev& C, const FrameDev& F_in, CgrtHitDev* hits, float* normals,
                                        uint32_t* ticks, hipStream_t stream) {
    if (!can_profile_frame(S, F_in) || !ticks) return hipErrorInvalidValue;
    FrameDev F = F_in;
    F.order = nullptr;
    const hipError_t e = hipMemsetAsync(ticks, 0, sizeof(uint32_t) * (size_t)(F.nblocks / 64u), stream);
    if (e != hipSuccess) return e;
    launch(k_trace_primary<false, true, false, false, false, false, false, true>, F.nblocks, 64u, stream, S, C, F, hits, normals,
           reinterpret_cast<unsigned long long*>(ticks));
    return hipGetLastError();
}
hipError_t launch_build_frame_order(const uint32_t* ticks, uint32_t nst, uint32_t live, uint16_t* out, hipStream_t stream) {
    const uint32_t n_pad = (nst + 7u) / 8u * 8u;
    if (n_pad == 0) return hipSuccess;
    if (n_pad > CGRT_ORDER_MAX_POSITIONS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_build_frame_order, dim3(8), dim3(256), 0, stream, ticks, n_pad, nst, live, out);
    return hipGetLastError();
}
hipError_t launch_trace_batch(const SceneDev& S, const RayList& R, unsigned long long* counters, hipStream_t stream, ListGrid grid) {
    if (R.n == 0) return hipSuccess;
    if (grid == GRID_STRIDED && (counters || !R.dcount)) return hipErrorInvalidValue;
    const ListPlan p = plan_list(S, R.n, R.dcount, R.expected, grid);
    with_bools(counters != nullptr, p.fast, [&](auto count, auto fast) {
        constexpr bool COUNT = decltype(count)::value, FAST = decltype(fast)::value;
        auto go = [&](auto kernel) { launch(kernel, p, stream, S, R.rays, R.n, R.hits, R.normals, counters, R.dcount, p.qrpw, p.adapt); };
        if constexpr (FAST) {
            if (p.quad) return go(k_trace_batch<COUNT, true, true>);
        }
        if constexpr (!COUNT) {
            if (p.strided) return go(k_trace_batch<false, FAST, false, true>);
        }
        go(k_trace_batch<COUNT, FAST>);
    });
    return hipGetLastError();
}
hipError_t launch_trace_shadow(const SceneDev& S, const ShadowList& A, unsigned long long* counters, hipStream_t stream, ListGrid grid) {
    if (A.n == 0) return hipSuccess;
    if (grid == GRID_STRIDED && (counters || !A.dcount)) return hipErrorInvalidValue;
    const ListPlan p = plan_list(S, A.n, A.dcount, A.expected, grid);
    const unsigned dmul = A.dmul ? A.dmul : 1u;
    with_bools(counters != nullptr, p.fast, [&](auto count, auto fast) {
        constexpr bool COUNT = decltype(count)::value, FAST = decltype(fast)::value;
        auto go = [&](auto kernel) { launch(kernel, p, stream, S, A.rays, A.dist, A.n, A.hits, A.dcount, counters, p.qrpw, p.adapt, dmul); };
        if constexpr (FAST) {
            if (p.quad) return go(k_trace_shadow<COUNT, true, true>);
        }
        if constexpr (!COUNT) {
            if (p.strided) return go(k_trace_shadow<false, FAST, false, true>);
        }
        go(k_trace_shadow<COUNT, FAST>);
    });
    return hipGetLastError();
}
// The two lists of one level in one launch (k_trace_pair); false when the scene or the forced shape does not allow it -- the caller
// then launches them one by one.
bool can_trace_pair(const SceneDev& S) { return S.fast_root != REF_NONE && trace_block(S) == 64 && (shape_mode() == SHAPE_AUTO || shape_mode() == SHAPE_LANE64 || shape_mode() == SHAPE_LANE16); }
// GRID_FULL: a list of capacity 0 takes no workgroups.  GRID_STRIDED: the caller pairs two lists that both have a capacity, and each
// list gets the cap (the two share the chip).
hipError_t launch_trace_pair(const SceneDev& S, const ShadowList& A, const RayList& B, hipStream_t stream, ListGrid grid) {
    if (grid == GRID_STRIDED ? (A.n == 0 || B.n == 0) : (A.n == 0 && B.n == 0)) return grid == GRID_STRIDED ? hipErrorInvalidValue : hipSuccess;
    const ListPlan a = plan_list(S, A.n, A.dcount, A.expected, grid, true), b = plan_list(S, B.n, B.dcount, B.expected, grid, true);
    ListPairDev P{};
    P.rays_a = A.rays, P.dist_a = A.dist, P.hits_a = A.hits, P.dcount_a = A.dcount, P.n_a = A.n, P.dmul_a = A.dmul ? A.dmul : 1u;
    P.rpw_a = a.qrpw, P.adapt_a = a.adapt, P.blocks_a = a.grid;
    P.rays_b = B.rays, P.hits_b = B.hits, P.normals_b = B.normals, P.dcount_b = B.dcount, P.n_b = B.n;
    P.rpw_b = b.qrpw, P.adapt_b = b.adapt, P.blocks_b = b.grid;
    with_bool(grid == GRID_STRIDED, [&](auto strided) { launch(k_trace_pair<true, decltype(strided)::value>, P.blocks_a + P.blocks_b, 64u, stream, S, P); });
    return hipGetLastError();
}
hipError_t launch_trace_primary_compact(const SceneDev& S, const CameraDev& C, const FrameDev& F, float* rays, CgrtHitDev* hits, float* normals,
                                        int* pixels, uint32_t* count, hipStream_t stream, unsigned long long* counters, float* rgb,
                                        const SpawnDev* spawn) {  // (spawn: a DEVICE address)
    if (F.nblocks == 0) return hipSuccess;
    const FramePlan p = plan_frame(S, F);
    with_bools(counters != nullptr, p.fast, [&](auto c, auto fast) {
        constexpr bool COUNT = decltype(c)::value, FAST = decltype(fast)::value;
        auto go = [&](auto kernel) { launch(kernel, p.grid, p.block, stream, S, C, F, rays, hits, normals, pixels, count, counters, rgb, spawn); };
        if constexpr (FAST) {
            if (p.quad) return go(k_trace_primary_compact<COUNT, true, true>);
        }
        go(k_trace_primary_compact<COUNT, FAST>);
    });
    return hipGetLastError();
}
// Multi-view frames: the VIEWS instantiations (no counters, no hints), in the shape a single frame of the same workgroup size takes.
// raycams: F.raycams is set instead of F.views (the RAYCAM instantiations).
hipError_t launch_trace_primary_views(const SceneDev& S, const FrameDev& F, CgrtHitDev* hits, float* normals, hipStream_t stream, bool raycams) {
    if (F.nblocks == 0) return hipSuccess;
    const FramePlan p = plan_frame(S, F);
    const CameraDev C{};  // (unused: the cameras are in F.views)
    unsigned long long* const counters = nullptr;
    with_bools(raycams, p.fast, [&](auto raycam, auto fast) {
        constexpr bool RAYCAM = decltype(raycam)::value, FAST = decltype(fast)::value;
        auto go = [&](auto kernel) { launch(kernel, p.grid, p.block, stream, S, C, F, hits, normals, counters); };
        if constexpr (FAST) {
            if (p.quad) return go(k_trace_primary<false, true, true, false, true, RAYCAM>);
        }
        go(k_trace_primary<false, FAST, false, false, true, RAYCAM>);
    });
    return hipGetLastError();
}
hipError_t launch_trace_primary_views_compact(const SceneDev& S, const FrameDev& F, float* rays, CgrtHitDev* hits, float* normals, int* pixels,
                                              uint32_t* count, float* rgb, hipStream_t stream, bool raycams) {
    if (F.nblocks == 0) return hipSuccess;
    const FramePlan p = plan_frame(S, F);
    const CameraDev C{};
    unsigned long long* const counters = nullptr;
    const SpawnDev* const spawn = nullptr;
    with_bools(raycams, p.fast, [&](auto raycam, auto fast) {
        constexpr bool RAYCAM = decltype(raycam)::value, FAST = decltype(fast)::value;
        auto go = [&](auto kernel) { launch(kernel, p.grid, p.block, stream, S, C, F, rays, hits, normals, pixels, count, counters, rgb, spawn); };
        if constexpr (FAST) {
            if (p.quad) return go(k_trace_primary_compact<false, true, true, true, RAYCAM>);
        }
        go(k_trace_primary_compact<false, FAST, false, true, RAYCAM>);
    });
    return hipGetLastError();
}
hipError_t launch_trace_list_compact(const SceneDev& S, const float* in_rays, unsigned long long n, float* rays, CgrtHitDev* hits, float* normals,
                                     int* pixels, uint32_t* count, float* rgb, hipStream_t stream, unsigned long long* counters) {
    if (n == 0) return hipSuccess;
    const ListPlan p = plan_list(S, n, nullptr, 0, GRID_FULL);  // (the list's length is known to the host: laid out as any ray list)
    with_bools(counters != nullptr, p.fast, [&](auto c, auto fast) {
        constexpr bool COUNT = decltype(c)::value, FAST = decltype(fast)::value;
        auto go = [&](auto kernel) { launch(kernel, p, stream, S, in_rays, n, rays, hits, normals, pixels, count, counters, rgb, p.qrpw); };
        if constexpr (FAST) {
            if (p.quad) return go(k_trace_list_compact<COUNT, true, true>);
        }
        go(k_trace_list_compact<COUNT, FAST>);
    });
    return hipGetLastError();
}
hipError_t launch_clear_owned(const FrameDev& F, float* rgb, hipStream_t stream) {
    if (F.nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_clear_owned, dim3(F.nblocks), dim3((unsigned)F.block), 0, stream, F, rgb);
    return hipGetLastError();
}
// Soft shadows of a level's items: one thread per (item, light, sample).  Q.set_index: a light-set batch's distinct keys, Q.view_pixels:
// a multi-view frame's items.  GRID_STRIDED: the first *dcount (<= nitems) items, a capped grid (k_soft_shadow_strided; light sets:
// k_soft_shadow_sets_strided, whose items are always a multi-view frame's).
hipError_t launch_soft_shadow(const SceneDev& S, const SoftDev& Q, const float* rays, const CgrtHitDev* hits, const int* item_pixels,
                              unsigned long long nitems, uint32_t* lit, int anyhit, hipStream_t stream, const uint32_t* dcount, ListGrid grid) {
    const unsigned long long nthreads = nitems * Q.nlights * Q.samples;
    if (nthreads == 0) return hipSuccess;
    const unsigned block = (unsigned)trace_block(S);
    const unsigned long long full = (nthreads + block - 1) / block;
    const bool strided = grid == GRID_STRIDED, views = Q.view_pixels != 0, sets = Q.set_index != nullptr;
    if (strided ? (!dcount || (sets && !views)) : full > 0x7fffffffull) return hipErrorInvalidValue;
    const unsigned blocks = strided ? strided_blocks((unsigned)std::min<unsigned long long>(full, 0x7fffffffull), block) : (unsigned)full;
    with_bools(anyhit != 0, S.fast_root != REF_NONE, [&](auto a, auto f) {
        constexpr bool A = decltype(a)::value, F = decltype(f)::value;
        auto go = [&](auto kernel) { launch(kernel, blocks, block, stream, S, Q, rays, hits, item_pixels, nthreads, lit); };
        auto go_strided = [&](auto kernel) { launch(kernel, blocks, block, stream, S, Q, rays, hits, item_pixels, nitems, dcount, lit); };
        if (strided) {
            if (sets) return go_strided(k_soft_shadow_sets_strided<A, F>);
            return views ? go_strided(k_soft_shadow_strided<A, F, true>) : go_strided(k_soft_shadow_strided<A, F, false>);
        }
        if (sets) return views ? go(k_soft_shadow_views_sets<A, F>) : go(k_soft_shadow_sets<A, F>);
        return views ? go(k_soft_shadow<A, F, false, true>) : go(k_soft_shadow<A, F>);
    });
    return hipGetLastError();
}
hipError_t launch_soft_points(const SceneDev& S, const SoftDev& Q, const float* points, unsigned long long npoints, uint32_t* lit, int anyhit,
                              hipStream_t stream) {
    const unsigned long long nthreads = npoints * Q.nlights * Q.samples;
    if (nthreads == 0) return hipSuccess;
    const unsigned block = (unsigned)trace_block(S);
    const unsigned long long blocks = (nthreads + block - 1) / block;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    with_bools(anyhit != 0, S.fast_root != REF_NONE, [&](auto a, auto f) {
        launch(k_soft_shadow<decltype(a)::value, decltype(f)::value, true>, (unsigned)blocks, block, stream, S, Q, points, nullptr, nullptr, nthreads, lit);
    });
    return hipGetLastError();
}
// The visibility queries (k_visibility): n answers, laid out by the list's shape (as launch_trace_batch; forced by cgrt_set_kernel_shape).
// POINTS: src holds n / nlights points.
template <bool POINTS>
static hipError_t launch_visibility(const SceneDev& S, const float* src, const float* lights, unsigned nlights, unsigned long long n, uint8_t* out,
                                    hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const ListPlan p = plan_list(S, n, nullptr, 0, GRID_FULL);
    with_bool(p.fast, [&](auto fast) {
        constexpr bool FAST = decltype(fast)::value;
        auto go = [&](auto kernel) { launch(kernel, p, stream, S, src, lights, nlights, n, out, p.qrpw); };
        if constexpr (FAST) {
            if (p.quad) return go(k_visibility<POINTS, true, true>);
        }
        go(k_visibility<POINTS, FAST>);
    });
    return hipGetLastError();
}
hipError_t launch_occluded(const SceneDev& S, const float* rays, unsigned long long n, uint8_t* out, hipStream_t stream) {
    return launch_visibility<false>(S, rays, nullptr, 0u, n, out, stream);
}
hipError_t launch_in_shadow(const SceneDev& S, const float* points, unsigned long long npoints, const float* lights, unsigned nlights, uint8_t* out,
                            hipStream_t stream) {
    return launch_visibility<true>(S, points, lights, nlights, npoints * nlights, out, stream);
}
// One word into host-visible memory, behind whatever the stream holds: lets a host thread wait for a launch by looking at its own
// memory instead of sleeping in a runtime call (capi_combine.cpp combined_intersect).
__global__ void k_signal(uint32_t* __restrict__ flag, uint32_t value) {
    if (threadIdx.x == 0 && blockIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
hipError_t launch_signal(uint32_t* flag, uint32_t value, hipStream_t stream) {
    hipLaunchKernelGGL(k_signal, dim3(1), dim3(64), 0, stream, flag, value);
    return hipGetLastError();
}
hipError_t launch_generate_rays(const CameraDev& C, int W, int H, int x0, int y0, int x1, int y1, float* rays, hipStream_t stream) {
    const unsigned long long n = (unsigned long long)(x1 - x0) * (unsigned long long)(y1 - y0);
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_generate_rays, dim3(grid_for(n, CGRT_BLOCK)), dim3(CGRT_BLOCK), 0, stream, C, W, H, x0, y0, x1, y1, rays);
    return hipGetLastError();
}
hipError_t launch_generate_rays_raycam(const RayCameraDev& C, int W, int H, float* rays, hipStream_t stream) {
    const unsigned long long n = (unsigned long long)W * (unsigned long long)H;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_generate_rays_raycam, dim3(grid_for(n, CGRT_BLOCK)), dim3(CGRT_BLOCK), 0, stream, C, W, H, rays);
    return hipGetLastError();
}

}  // namespace cgrt
