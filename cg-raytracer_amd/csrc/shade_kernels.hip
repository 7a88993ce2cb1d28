// shade_kernels.hip -- the reference's shading / recursion driver (src/main.cpp:61-310) on the device, as a wavefront:
// per recursion level one kernel spawns the shadow rays of every hit (pointInShadow, :104-135), the batch traversal
// kernel answers them, one kernel evaluates the Phong terms (:61-98, :219-232) and spawns the mirror rays (shade,
// :241-264), and after the last level one kernel folds the levels back (color = direct + reflected * ks, :262).
// Every level is a COMPACT list of live paths: level 0 is the frame in the primary kernel's order (tiles, super-tiles),
// a hit appends its shadow rays to the level's shadow list and its mirror ray to the next level's list (one wave-level
// atomic per append site, lanes ranked by ballot), so that the traversal kernel only ever sees real rays, still roughly
// in tile order.  Links: an entry's level record holds the index of its child entry on the next level; sslot[entry * L + l]
// is the index of its shadow ray towards light l.  Spherical lights (:168-218) are sampled by k_soft_shadow (trace_kernels.hip), which
// leaves the number of unoccluded samples per (item, light); the draws of randomUnitVector() are a caller-supplied table.
// Arithmetic follows the reference's expression order (cgrt_math.h); pow(float, float) is powf (device libm: the last
// ulp may differ from glibc's -- the RGB parity bar is 1e-5 absolute).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cgrt_layout.h"
#include "cgrt_math.h"
#include "spawn_rays.h"
#include "trace_kernels.h"

namespace cgrt {

__device__ __forceinline__ F3 ldv(const float* p) { return f3(p[0], p[1], p[2]); }

// Block-aggregated append: threads with `want` get consecutive indices of the list behind `counter`, ONE atomic per
// workgroup (same-address atomics serialise at the L2, ~12 ns each: one per wave made these streaming kernels
// atomic-bound).  Every thread of the block must call it; s_tmp = blockDim.x / 64 + 1 LDS words.
__device__ __forceinline__ uint32_t block_append(uint32_t* counter, const bool want, uint32_t* s_tmp) {
    const unsigned long long m = __ballot(want);
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63u, nw = blockDim.x >> 6;
    if (lane == 0) s_tmp[w] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (unsigned k = 0; k < nw; k++) {
            const uint32_t c = s_tmp[k];
            s_tmp[k] = tot;
            tot += c;
        }
        s_tmp[nw] = tot ? atomicAdd(counter, tot) : 0u;
    }
    __syncthreads();
    const uint32_t idx = s_tmp[nw] + s_tmp[w] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();  // s_tmp is reused by the next call
    return idx;
}
#define CGRT_SHADE_BLOCK 1024

// entry i of k_spawn, for k_spawn_strided (n: the list's length; every thread of the workgroup calls it: the appends are per workgroup);
// returns whether entry i is a hit.  A copy of k_spawn's body (k_spawn keeps its own: calling this changed its SGPRs, measured
// with tools/enqueue_resource_usage.py): the two must stay in step.
__device__ __forceinline__ bool spawn_entry(const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits, const float* __restrict__ normals,
                                            const int* __restrict__ pixels, unsigned long long i, unsigned long long n, const float* __restrict__ materials,
                                            const float* __restrict__ lights, unsigned nlights, int spawn, float* __restrict__ srays,
                                            float* __restrict__ sdist, int* __restrict__ sslot, float4* __restrict__ lvl, float* __restrict__ next_rays,
                                            int* __restrict__ next_pixels, uint32_t* __restrict__ counters, uint32_t* s_tmp) {
    const bool in = i < n;
    const bool hit = in && hits[i].hit != 0;
    F3 pointOn = f3(0.f, 0.f, 0.f), d = f3(0.f, 0.f, 0.f), ks = f3(0.f, 0.f, 0.f);
    if (hit) {
        const float* r = rays + 7 * i;
        d = ldv(r + 3);
        pointOn = add(ldv(r), scale(d, hits[i].t));
        const int mid = hits[i].material_id;
        // a hit that never wrote hitInfo.material (sphere only) reads an indeterminate Material upstream; default Material here
        ks = mid >= 0 ? ldv(materials + 8 * mid + 3) : f3(0.f, 0.f, 0.f);
    }
    for (unsigned l = 0; l < nlights; l++) {
        const uint32_t idx = block_append(counters + 0, hit, s_tmp);
        if (in) sslot[i * nlights + l] = hit ? (int)idx : -1;
        if (hit) spawn_shadow_ray(lights, l, pointOn, idx, srays, sdist);
    }
    // :246 tests ks.z only (comma operator); `spawn` = level + 1 < maxLevel (:267)
    const bool wants_mirror = hit && !(ks.z <= 0.01f) && spawn;
    const uint32_t child = block_append(counters + 1, wants_mirror, s_tmp);
    if (wants_mirror) {
        spawn_mirror_ray(pointOn, d, ldv(normals + 3 * i), child, next_rays);
        next_pixels[child] = pixels[i];
    }
    if (in) lvl[2 * i + 1] = make_float4(ks.x, ks.y, ks.z, __int_as_float(wants_mirror ? (int)child : -1));
    return hit;
}
// hits of the level: one atomic per workgroup (h: the wave's count)
__device__ __forceinline__ void spawn_count_hits(uint32_t h, uint32_t* __restrict__ counters, uint32_t* s_tmp) {
    if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (unsigned k = 0; k < (blockDim.x >> 6); k++) tot += s_tmp[k];
        if (tot) atomicAdd(counters + 2, tot);
    }
}
// Everything a hit spawns, in one pass: pointInShadow's rays (main.cpp:104-111) for every light, appended to the level's
// shadow list, and shade's mirror ray (:246-258), appended to the next level's list -- the mirror ray does not depend on
// the shadow results, so its batch can be traversed on a second stream while this level's shadow batch runs.
// lvl[2 i + 1] = {ks.xyz, child}; child = index of the mirror ray's entry on the next level, -1 when none was spawned.
// counters[0] += shadow rays, counters[1] += mirror rays, counters[2] += hits.
__global__ __launch_bounds__(CGRT_SHADE_BLOCK) void k_spawn(const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                            const float* __restrict__ normals, const int* __restrict__ pixels,
                                                            unsigned long long n, const float* __restrict__ materials,
                                                            const float* __restrict__ lights, unsigned nlights, int spawn,
                                                            float* __restrict__ srays, float* __restrict__ sdist, int* __restrict__ sslot,
                                                            float4* __restrict__ lvl, float* __restrict__ next_rays,
                                                            int* __restrict__ next_pixels, uint32_t* __restrict__ counters,
                                                            const uint32_t* __restrict__ dcount) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (dcount) {  // the list's length is only known on the device (the grid covers its capacity n)
        const unsigned long long present = *dcount;
        n = present < n ? present : n;
    }
    const bool in = i < n;
    const bool hit = in && hits[i].hit != 0;
    F3 pointOn = f3(0.f, 0.f, 0.f), d = f3(0.f, 0.f, 0.f), ks = f3(0.f, 0.f, 0.f);
    if (hit) {
        const float* r = rays + 7 * i;
        d = ldv(r + 3);
        pointOn = add(ldv(r), scale(d, hits[i].t));
        const int mid = hits[i].material_id;
        // a hit that never wrote hitInfo.material (sphere only) reads an indeterminate Material upstream; default Material here
        ks = mid >= 0 ? ldv(materials + 8 * mid + 3) : f3(0.f, 0.f, 0.f);
    }
    __shared__ uint32_t s_tmp[CGRT_SHADE_BLOCK / 64 + 1];
    for (unsigned l = 0; l < nlights; l++) {
        const uint32_t idx = block_append(counters + 0, hit, s_tmp);
        if (in) sslot[i * nlights + l] = hit ? (int)idx : -1;
        if (hit) spawn_shadow_ray(lights, l, pointOn, idx, srays, sdist);
    }
    // :246 tests ks.z only (comma operator); `spawn` = level + 1 < maxLevel (:267)
    const bool wants_mirror = hit && !(ks.z <= 0.01f) && spawn;
    const uint32_t child = block_append(counters + 1, wants_mirror, s_tmp);
    if (wants_mirror) {
        spawn_mirror_ray(pointOn, d, ldv(normals + 3 * i), child, next_rays);
        next_pixels[child] = pixels[i];
    }
    if (in) lvl[2 * i + 1] = make_float4(ks.x, ks.y, ks.z, __int_as_float(wants_mirror ? (int)child : -1));
    // hits of the level: one atomic per workgroup
    const uint32_t h = (uint32_t)__popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (unsigned k = 0; k < (blockDim.x >> 6); k++) tot += s_tmp[k];
        if (tot) atomicAdd(counters + 2, tot);
    }
}
// The count-driven forms of this file's list kernels (enqueued frames, capi_frames.cpp enqueue_impl): dcount is required, n is the list's
// capacity, and a capped grid strides over the *dcount entries present, gridDim.x * blockDim.x at a time (the loops are uniform per
// workgroup, as block_append needs).  An entry is handled by the expressions of the one-pass kernel: the results are its results.
__global__ __launch_bounds__(CGRT_SHADE_BLOCK) void k_spawn_strided(const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                                    const float* __restrict__ normals, const int* __restrict__ pixels,
                                                                    unsigned long long n, const float* __restrict__ materials,
                                                                    const float* __restrict__ lights, unsigned nlights, int spawn,
                                                                    float* __restrict__ srays, float* __restrict__ sdist, int* __restrict__ sslot,
                                                                    float4* __restrict__ lvl, float* __restrict__ next_rays,
                                                                    int* __restrict__ next_pixels, uint32_t* __restrict__ counters,
                                                                    const uint32_t* __restrict__ dcount) {
    const unsigned long long present = *dcount;
    n = present < n ? present : n;
    __shared__ uint32_t s_tmp[CGRT_SHADE_BLOCK / 64 + 1];
    uint32_t h = 0;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < n; base += step) {
        const bool hit = spawn_entry(rays, hits, normals, pixels, base + threadIdx.x, n, materials, lights, nlights, spawn, srays, sdist, sslot, lvl,
                                     next_rays, next_pixels, counters, s_tmp);
        h += (uint32_t)__popcll(__ballot(hit));  // (block_append's last barrier has freed s_tmp for the next pass)
    }
    spawn_count_hits(h, counters, s_tmp);
}

// shading (main.cpp:160-235) for one level: lvl[2 i] = {direct light.xyz, flags}, flags bit0 = hit.
__device__ __forceinline__ void shade_entry(const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits, const float* __restrict__ normals,
                                            const CgrtHitDev* __restrict__ shits, const float* __restrict__ sdist, const int* __restrict__ sslot,
                                            unsigned long long i, const float* __restrict__ materials, const float* __restrict__ lights, unsigned nlights,
                                            const float* __restrict__ slights, unsigned nslights, const uint32_t* __restrict__ lit, unsigned samples,
                                            float4* __restrict__ lvl) {
    float4 out0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (hits[i].hit) {
        const float* r = rays + 7 * i;
        const F3 o = ldv(r), d = ldv(r + 3);
        const F3 nrm = ldv(normals + 3 * i);
        const F3 pointOn = add(o, scale(d, hits[i].t));
        const int mid = hits[i].material_id;
        const F3 kd = mid >= 0 ? ldv(materials + 8 * mid) : f3(0.f, 0.f, 0.f);
        const F3 ks = mid >= 0 ? ldv(materials + 8 * mid + 3) : f3(0.f, 0.f, 0.f);
        const float shininess = mid >= 0 ? materials[8 * mid + 6] : 1.0f;
        const float eps = 0.001f;
        F3 result = f3(0.f, 0.f, 0.f);
        const float dn = dot(nrm, d);  // glm::reflect(I, N) = I - N * dot(N, I) * 2
        const F3 refl = normalize(sub(d, scale(scale(nrm, dn), 2.0f)));
        for (unsigned l = 0; l < nslights; l++) {  // spherical lights first (main.cpp:168-218)
            const F3 lpos = ldv(slights + 7 * l), lcol = ldv(slights + 7 * l + 4);
            const F3 toLight = normalize(sub(lpos, pointOn));
            const float dc = dot(toLight, nrm);
            const F3 dif = dc <= 0 ? f3(0.f, 0.f, 0.f) : f3(lcol.x * kd.x * dc, lcol.y * kd.y * dc, lcol.z * kd.z * dc);
            const float sc = dot(refl, toLight);
            F3 spec = f3(0.f, 0.f, 0.f);
            if (!(sc <= 0)) {
                const float p = __builtin_powf(sc, shininess);
                spec = f3(lcol.x * ks.x * p, lcol.y * ks.y * p, lcol.z * ks.z * p);
            }
            // softShadowCounter: `samples` additions of 1.0f (exact), then / 200.0f (:200)
            const float counter = (float)lit[i * nslights + l] / (float)samples;
            result = add(result, scale(dif, counter));
            result = add(result, scale(spec, counter));
        }
        for (unsigned l = 0; l < nlights; l++) {
            const F3 lpos = ldv(lights + 6 * l), lcol = ldv(lights + 6 * l + 3);
            const F3 toLight = normalize(sub(lpos, pointOn));
            const int slot = sslot[i * nlights + l];
            const CgrtHitDev sh = shits[slot];
            const bool inShadow = sh.hit && !(sh.t + eps >= sdist[slot]);  // main.cpp:118-130
            if (inShadow) continue;
            const float dc = dot(toLight, nrm);  // diffuseOneLight :84-98
            const F3 dif = dc <= 0 ? f3(0.f, 0.f, 0.f) : f3(lcol.x * kd.x * dc, lcol.y * kd.y * dc, lcol.z * kd.z * dc);
            const float sc = dot(refl, toLight);  // specularOneLight :61-82
            F3 spec = f3(0.f, 0.f, 0.f);
            if (!(sc <= 0)) {
                const float p = __builtin_powf(sc, shininess);
                spec = f3(lcol.x * ks.x * p, lcol.y * ks.y * p, lcol.z * ks.z * p);
            }
            result = add(result, dif);
            result = add(result, spec);
        }
        out0 = make_float4(result.x, result.y, result.z, __uint_as_float(1u));
    }
    lvl[2 * i] = out0;
}
__global__ __launch_bounds__(CGRT_SHADE_BLOCK) void k_shade(const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                            const float* __restrict__ normals, const CgrtHitDev* __restrict__ shits,
                                                            const float* __restrict__ sdist, const int* __restrict__ sslot,
                                                            unsigned long long n, const float* __restrict__ materials,
                                                            const float* __restrict__ lights, unsigned nlights,
                                                            const float* __restrict__ slights, unsigned nslights,
                                                            const uint32_t* __restrict__ lit, unsigned samples, float4* __restrict__ lvl,
                                                            const uint32_t* __restrict__ dcount) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (dcount) {
        const unsigned long long present = *dcount;
        n = present < n ? present : n;
    }
    if (i >= n) return;
    shade_entry(rays, hits, normals, shits, sdist, sslot, i, materials, lights, nlights, slights, nslights, lit, samples, lvl);
}
__global__ __launch_bounds__(CGRT_SHADE_BLOCK) void k_shade_strided(const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                                    const float* __restrict__ normals, const CgrtHitDev* __restrict__ shits,
                                                                    const float* __restrict__ sdist, const int* __restrict__ sslot,
                                                                    unsigned long long n, const float* __restrict__ materials,
                                                                    const float* __restrict__ lights, unsigned nlights,
                                                                    const float* __restrict__ slights, unsigned nslights,
                                                                    const uint32_t* __restrict__ lit, unsigned samples, float4* __restrict__ lvl,
                                                                    const uint32_t* __restrict__ dcount) {
    const unsigned long long present = *dcount;
    n = present < n ? present : n;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        shade_entry(rays, hits, normals, shits, sdist, sslot, i, materials, lights, nlights, slights, nslights, lit, samples, lvl);
}

// colour = !hit ? 0 : (ks.z <= 0.01 ? direct : direct + childColour * ks)   (main.cpp:248, :262, :293); the child's
// record already holds its folded colour (levels are folded deepest first).
__device__ __forceinline__ void fold_entry(float4* __restrict__ lvl, const float4* __restrict__ child_lvl, unsigned long long i) {
    const float4 a = lvl[2 * i], b = lvl[2 * i + 1];
    const int child = __float_as_int(b.w);
    if (!(__float_as_uint(a.w) & 1u) || (b.z <= 0.01f) || child < 0) return;  // no child: colour + 0 * ks = colour
    const float4 c = child_lvl[2 * (unsigned long long)child];  // a child that missed holds colour 0
    lvl[2 * i] = make_float4(a.x + c.x * b.x, a.y + c.y * b.y, a.z + c.z * b.z, a.w);
}
__global__ void k_fold(float4* __restrict__ lvl, const float4* __restrict__ child_lvl, unsigned long long n,
                       const uint32_t* __restrict__ dcount) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (dcount) {  // (as k_spawn: the grid covers the list's capacity)
        const unsigned long long present = *dcount;
        n = present < n ? present : n;
    }
    if (i >= n) return;
    fold_entry(lvl, child_lvl, i);
}
__global__ void k_fold_strided(float4* __restrict__ lvl, const float4* __restrict__ child_lvl, unsigned long long n, const uint32_t* __restrict__ dcount) {
    const unsigned long long present = *dcount;
    n = present < n ? present : n;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) fold_entry(lvl, child_lvl, i);
}

// child_lvl (optional): the fold of level 0 with level 1 (k_fold's arithmetic) happens here, one launch less
__device__ __forceinline__ void write_rgb_entry(const float4* __restrict__ lvl0, const float4* __restrict__ child_lvl, unsigned long long i,
                                                const int* __restrict__ item_pixels, float* __restrict__ rgb) {
    const long long pix = item_pixels[i];
    if (pix < 0) return;  // item outside the frame
    float4 a = lvl0[2 * i];
    if (child_lvl) {
        const float4 b = lvl0[2 * i + 1];
        const int child = __float_as_int(b.w);
        if ((__float_as_uint(a.w) & 1u) && !(b.z <= 0.01f) && child >= 0) {
            const float4 c = child_lvl[2 * (unsigned long long)child];
            a = make_float4(a.x + c.x * b.x, a.y + c.y * b.y, a.z + c.z * b.z, a.w);
        }
    }
    rgb[3 * pix] = a.x;
    rgb[3 * pix + 1] = a.y;
    rgb[3 * pix + 2] = a.z;
}
__global__ void k_write_rgb(const float4* __restrict__ lvl0, const float4* __restrict__ child_lvl, unsigned long long n,
                            const int* __restrict__ item_pixels, float* __restrict__ rgb, const uint32_t* __restrict__ dcount) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (dcount) {
        const unsigned long long present = *dcount;
        n = present < n ? present : n;
    }
    if (i >= n) return;
    write_rgb_entry(lvl0, child_lvl, i, item_pixels, rgb);
}
__global__ void k_write_rgb_strided(const float4* __restrict__ lvl0, const float4* __restrict__ child_lvl, unsigned long long n,
                                    const int* __restrict__ item_pixels, float* __restrict__ rgb, const uint32_t* __restrict__ dcount) {
    const unsigned long long present = *dcount;
    n = present < n ? present : n;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) write_rgb_entry(lvl0, child_lvl, i, item_pixels, rgb);
}

// ---- Light sets (cgrt_render_light_sets*): one camera's ray tree shaded under T.nsets light sets ----
// The level lists, their link records lvl[2i+1] = {ks, child} and the shadow answers belong to the batch and are shared by every set:
// k_spawn traced one shadow ray per hit and DISTINCT point-light position p (sslot[i * npos + p]), k_soft_shadow_sets counted
// lit[i * nsph + k] per distinct spherical key k.  What depends on a set is its colours and which lights it holds: set b's direct colour of
// entry i is out[b * stride + i] = {colour, flags} (consecutive entries at consecutive addresses).  k_shade_sets computes what does not
// depend on the set once per entry, then every set's sum in shade_entry's expression order (spherical lights first, :168-218, then the
// point lights, :219-232), so that set b's colour is, bit for bit, what k_shade writes in set b's single frame.
// shade_sets_entry: entry i of k_shade_sets (and of k_shade_sets_strided, enqueued batches).
__device__ __forceinline__ void shade_sets_entry(const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits, const float* __restrict__ normals,
                                                 const CgrtHitDev* __restrict__ shits, const float* __restrict__ sdist, const int* __restrict__ sslot,
                                                 unsigned long long i, const float* __restrict__ materials, unsigned npos, unsigned nsph,
                                                 const uint32_t* __restrict__ lit, unsigned samples, const SetsDev& T, float4* __restrict__ out,
                                                 unsigned long long stride) {
    const bool hit = hits[i].hit != 0;
    F3 nrm = f3(0.f, 0.f, 0.f), pointOn = f3(0.f, 0.f, 0.f), kd = f3(0.f, 0.f, 0.f), ks = f3(0.f, 0.f, 0.f), refl = f3(0.f, 0.f, 0.f);
    float shininess = 1.0f;
    if (hit) {
        const float* r = rays + 7 * i;
        const F3 o = ldv(r), d = ldv(r + 3);
        nrm = ldv(normals + 3 * i);
        pointOn = add(o, scale(d, hits[i].t));
        const int mid = hits[i].material_id;
        kd = mid >= 0 ? ldv(materials + 8 * mid) : f3(0.f, 0.f, 0.f);
        ks = mid >= 0 ? ldv(materials + 8 * mid + 3) : f3(0.f, 0.f, 0.f);
        shininess = mid >= 0 ? materials[8 * mid + 6] : 1.0f;
        const float dn = dot(nrm, d);  // glm::reflect(I, N) = I - N * dot(N, I) * 2
        refl = normalize(sub(d, scale(scale(nrm, dn), 2.0f)));
    }
    const float eps = 0.001f;
    for (unsigned b = 0; b < T.nsets; b++) {
        float4 out0 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (hit) {
            F3 result = f3(0.f, 0.f, 0.f);
            for (uint32_t k = T.sph_off[b]; k < T.sph_off[b + 1]; k++) {  // spherical lights first (main.cpp:168-218)
                const float4 lp = T.sph[2 * k], lc = T.sph[2 * k + 1];
                const F3 lpos = f3(lp.x, lp.y, lp.z), lcol = f3(lc.x, lc.y, lc.z);
                const F3 toLight = normalize(sub(lpos, pointOn));
                const float dc = dot(toLight, nrm);
                const F3 dif = dc <= 0 ? f3(0.f, 0.f, 0.f) : f3(lcol.x * kd.x * dc, lcol.y * kd.y * dc, lcol.z * kd.z * dc);
                const float sc = dot(refl, toLight);
                F3 spec = f3(0.f, 0.f, 0.f);
                if (!(sc <= 0)) {
                    const float p = __builtin_powf(sc, shininess);
                    spec = f3(lcol.x * ks.x * p, lcol.y * ks.y * p, lcol.z * ks.z * p);
                }
                const float counter = (float)lit[i * nsph + __float_as_uint(lp.w)] / (float)samples;  // (:200)
                result = add(result, scale(dif, counter));
                result = add(result, scale(spec, counter));
            }
            for (uint32_t k = T.point_off[b]; k < T.point_off[b + 1]; k++) {
                const float4 lp = T.point[2 * k], lc = T.point[2 * k + 1];
                const F3 lpos = f3(lp.x, lp.y, lp.z), lcol = f3(lc.x, lc.y, lc.z);
                const F3 toLight = normalize(sub(lpos, pointOn));
                const int slot = sslot[i * npos + __float_as_uint(lp.w)];
                const CgrtHitDev sh = shits[slot];
                const bool inShadow = sh.hit && !(sh.t + eps >= sdist[slot]);  // main.cpp:118-130
                if (inShadow) continue;
                const float dc = dot(toLight, nrm);  // diffuseOneLight :84-98
                const F3 dif = dc <= 0 ? f3(0.f, 0.f, 0.f) : f3(lcol.x * kd.x * dc, lcol.y * kd.y * dc, lcol.z * kd.z * dc);
                const float sc = dot(refl, toLight);  // specularOneLight :61-82
                F3 spec = f3(0.f, 0.f, 0.f);
                if (!(sc <= 0)) {
                    const float p = __builtin_powf(sc, shininess);
                    spec = f3(lcol.x * ks.x * p, lcol.y * ks.y * p, lcol.z * ks.z * p);
                }
                result = add(result, dif);
                result = add(result, spec);
            }
            out0 = make_float4(result.x, result.y, result.z, __uint_as_float(1u));
        }
        out[(unsigned long long)b * stride + i] = out0;
    }
}
__global__ __launch_bounds__(CGRT_SHADE_BLOCK) void k_shade_sets(const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                                 const float* __restrict__ normals, const CgrtHitDev* __restrict__ shits,
                                                                 const float* __restrict__ sdist, const int* __restrict__ sslot,
                                                                 unsigned long long n, const float* __restrict__ materials, unsigned npos,
                                                                 unsigned nsph, const uint32_t* __restrict__ lit, unsigned samples, SetsDev T,
                                                                 float4* __restrict__ out, unsigned long long stride,
                                                                 const uint32_t* __restrict__ dcount) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (dcount) {  // (as k_shade: the grid covers the list's capacity)
        const unsigned long long present = *dcount;
        n = present < n ? present : n;
    }
    if (i >= n) return;
    shade_sets_entry(rays, hits, normals, shits, sdist, sslot, i, materials, npos, nsph, lit, samples, T, out, stride);
}
// fold_entry per set: the set's colours of this level (sets_lvl + o) += its colours of the next (child_sets + o) * ks, through the shared
// link records lvl[2i+1] (main.cpp:262)
__device__ __forceinline__ void fold_sets_entry(const float4* __restrict__ lvl, float4* __restrict__ sets_lvl, const float4* __restrict__ child_sets,
                                                unsigned long long i, unsigned long long o) {
    const float4 a = sets_lvl[o + i], b = lvl[2 * i + 1];
    const int child = __float_as_int(b.w);
    if (!(__float_as_uint(a.w) & 1u) || (b.z <= 0.01f) || child < 0) return;  // no child: colour + 0 * ks = colour
    const float4 c = child_sets[o + (unsigned long long)child];             // a child that missed holds colour 0
    sets_lvl[o + i] = make_float4(a.x + c.x * b.x, a.y + c.y * b.y, a.z + c.z * b.z, a.w);
}
// set blockIdx.y of every entry
__global__ void k_fold_sets(const float4* __restrict__ lvl, float4* __restrict__ sets_lvl, const float4* __restrict__ child_sets, unsigned long long n,
                            unsigned long long stride) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fold_sets_entry(lvl, sets_lvl, child_sets, i, (unsigned long long)blockIdx.y * stride);
}
// write_rgb_entry's colour per set: the set's level-0 colour of entry i (sets0 + o), folded with level 1 when child_sets is given
__device__ __forceinline__ float4 sets_colour0(const float4* __restrict__ lvl0, const float4* __restrict__ sets0, const float4* __restrict__ child_sets,
                                               unsigned long long i, unsigned long long o) {
    float4 a = sets0[o + i];
    if (child_sets) {
        const float4 b = lvl0[2 * i + 1];
        const int child = __float_as_int(b.w);
        if ((__float_as_uint(a.w) & 1u) && !(b.z <= 0.01f) && child >= 0) {
            const float4 c = child_sets[o + (unsigned long long)child];
            a = make_float4(a.x + c.x * b.x, a.y + c.y * b.y, a.z + c.z * b.z, a.w);
        }
    }
    return a;
}
__device__ __forceinline__ void store_rgb(float* __restrict__ p, const float4 a) {
    p[0] = a.x;
    p[1] = a.y;
    p[2] = a.z;
}
// write_rgb_entry per set: set blockIdx.y's level-0 colour (folded with level 1 when child_sets is given) goes to its own frame,
// rgb[3 * (set * frame_pixels + pixel)]
__global__ void k_write_rgb_sets(const float4* __restrict__ lvl0, const float4* __restrict__ sets0, const float4* __restrict__ child_sets,
                                 unsigned long long n, unsigned long long stride, const int* __restrict__ item_pixels, float* __restrict__ rgb,
                                 unsigned long long frame_pixels) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long pix = item_pixels[i];
    if (pix < 0) return;  // item outside the frame
    const float4 a = sets_colour0(lvl0, sets0, child_sets, i, (unsigned long long)blockIdx.y * stride);
    store_rgb(rgb + 3ull * ((unsigned long long)blockIdx.y * frame_pixels + (unsigned long long)pix), a);
}

// ---- Multi-view light sets (cgrt_render_views_light_sets*): nviews cameras' ray trees under T.nsets sets ----
// The lists are a multi-view frame's (pixel = view * view_pixels + in-view pixel); the shading, the folds and the shadow answers are the
// light sets' kernels above, unchanged.  Only the scatter differs: frame (view, set) is frame number view * nsets + set of the batch, so
// set s's colour of a pixel goes to rgb[3 * ((view * nsets + s) * view_pixels + in-view pixel)] -- the (V, S, H, W) order of the caller's
// output, which the export then writes as V * S frames back to back.
__device__ __forceinline__ unsigned long long views_sets_pixel(unsigned long long pix, unsigned set, unsigned nsets, unsigned long long view_pixels) {
    const unsigned long long v = pix / view_pixels;
    return (v * nsets + set) * view_pixels + (pix - v * view_pixels);
}
// k_write_rgb_sets for a multi-view batch: set blockIdx.y of every entry
__global__ void k_write_rgb_views_sets(const float4* __restrict__ lvl0, const float4* __restrict__ sets0, const float4* __restrict__ child_sets,
                                       unsigned long long n, unsigned long long stride, const int* __restrict__ item_pixels, float* __restrict__ rgb,
                                       unsigned long long view_pixels) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long pix = item_pixels[i];
    if (pix < 0) return;  // item outside the frame
    const float4 a = sets_colour0(lvl0, sets0, child_sets, i, (unsigned long long)blockIdx.y * stride);
    store_rgb(rgb + 3ull * views_sets_pixel((unsigned long long)pix, blockIdx.y, gridDim.y, view_pixels), a);
}
// The count-driven forms (enqueued batches; see k_spawn_strided): a capped grid strides over the *dcount entries present, and each entry
// handles every set, in the one-pass kernels' expressions.
__global__ __launch_bounds__(CGRT_SHADE_BLOCK) void k_shade_sets_strided(const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                                         const float* __restrict__ normals, const CgrtHitDev* __restrict__ shits,
                                                                         const float* __restrict__ sdist, const int* __restrict__ sslot,
                                                                         unsigned long long n, const float* __restrict__ materials, unsigned npos,
                                                                         unsigned nsph, const uint32_t* __restrict__ lit, unsigned samples, SetsDev T,
                                                                         float4* __restrict__ out, unsigned long long stride,
                                                                         const uint32_t* __restrict__ dcount) {
    const unsigned long long present = *dcount;
    n = present < n ? present : n;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        shade_sets_entry(rays, hits, normals, shits, sdist, sslot, i, materials, npos, nsph, lit, samples, T, out, stride);
}
__global__ void k_fold_sets_strided(const float4* __restrict__ lvl, float4* __restrict__ sets_lvl, const float4* __restrict__ child_sets,
                                    unsigned long long n, unsigned long long stride, unsigned nsets, const uint32_t* __restrict__ dcount) {
    const unsigned long long present = *dcount;
    n = present < n ? present : n;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        for (unsigned b = 0; b < nsets; b++) fold_sets_entry(lvl, sets_lvl, child_sets, i, (unsigned long long)b * stride);
}
__global__ void k_write_rgb_views_sets_strided(const float4* __restrict__ lvl0, const float4* __restrict__ sets0, const float4* __restrict__ child_sets,
                                               unsigned long long n, unsigned long long stride, unsigned nsets, const int* __restrict__ item_pixels,
                                               float* __restrict__ rgb, unsigned long long view_pixels, const uint32_t* __restrict__ dcount) {
    const unsigned long long present = *dcount;
    n = present < n ? present : n;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const long long pix = item_pixels[i];
        if (pix < 0) continue;  // item outside the frame
        for (unsigned b = 0; b < nsets; b++)
            store_rgb(rgb + 3ull * views_sets_pixel((unsigned long long)pix, b, nsets, view_pixels),
                      sets_colour0(lvl0, sets0, child_sets, i, (unsigned long long)b * stride));
    }
}

// The reference's antiAliasing branch (main.cpp:663-687): pixel (x, y) of the W x H frame is resolved from the sub-samples
// (2x + dx, 2y + dy) of the 2W x 2H frame `sub` the wavefront shaded -- summed channel by channel in the reference's loop order (yc
// outer, xc inner) onto a zero accumulator (upstream's `glm::vec3 color;` is uninitialised, DESIGN.md "Anti-aliasing" finding 1) and
// divided by level * 2.5f = 5.0f (:685; an IEEE division, not a product with 0.2f: -ffp-contract=off and correctly rounded division,
// csrc/Makefile).  F is the sub-sample frame: one thread per pixel of the 64x64 sub-sample super-tiles this rank owns (32x32 pixels
// each, so a pixel's four sub-samples always belong to one rank).  packed: pixel k of the rank's sl-th super-tile goes to
// out[sl * 1024 + k] (the rank's pixels back to back: one contiguous download), otherwise to out[y * W + x].
__global__ void k_resolve_aa(FrameDev F, const float* __restrict__ sub, float* __restrict__ out, int packed) {
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long sl = t >> 10;
    if (sl >= F.nst_rank) return;
    const unsigned k = (unsigned)(t & 1023u);
    const unsigned long long st = (unsigned long long)F.rank + (unsigned long long)F.nranks * sl;
    const int W = F.W / 2, H = F.H / 2;
    const int x = (int)(st % (unsigned long long)F.st_x) * 32 + (int)(k & 31u);
    const int y = (int)(st / (unsigned long long)F.st_x) * 32 + (int)(k >> 5);
    if (x >= W || y >= H) return;
    float r = 0.0f, g = 0.0f, b = 0.0f;  // :660, restated as zero
    for (int yc = 2 * y; yc < 2 * y + 2; yc++)      // :666
        for (int xc = 2 * x; xc < 2 * x + 2; xc++) {  // :668
            const float* p = sub + 3ull * ((unsigned long long)yc * (unsigned long long)F.W + (unsigned long long)xc);
            r = r + p[0];
            g = g + p[1];
            b = b + p[2];
        }
    const float level = 2.0f;
    const float d = level * 2.5f;  // :685
    const unsigned long long o = packed ? (sl << 10) + k : (unsigned long long)y * (unsigned long long)W + (unsigned long long)x;
    out[3 * o] = r / d;
    out[3 * o + 1] = g / d;
    out[3 * o + 2] = b / d;
}

// Screen::writeBitmapToFile's conversion of one channel (screen.cpp:38-49): clamp to [0, 1], * 255.0f, truncated to u8.  NaN (upstream:
// undefined behaviour of the cast) -> 0: both comparisons are false for it.
__device__ __forceinline__ unsigned to_u8(float v) {
    const float c = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
    return (unsigned)(c * 255.0f);  // (an f32 product, converted toward zero: v_cvt_u32_f32)
}
__device__ __forceinline__ unsigned rgba8(float r, float g, float b) { return to_u8(r) | (to_u8(g) << 8) | (to_u8(b) << 16) | 0xff000000u; }

// cgrt_render_device's export: one thread per 4 consecutive pixels of a row -- three float4 loads, then one 16-B store (RGBA8), one
// float4 store per plane (CHW) or three float4 stores (RGB_F32).  Row ends and bases that are not 16-B aligned (W % 4 != 0, pitches
// that are not multiples of 16) take the scalar path.  Tiles are multiples of 4 pixels wide, so the 4 pixels share an owner.
// VIEWS (ExportDev::views > 1, k_export_views): the threads of all views in one grid, view v's after view v - 1's.
template <bool VIEWS>
__device__ __forceinline__ void export_frame(ExportDev E) {
    unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long G = (unsigned long long)((E.W + 3) >> 2);  // 4-pixel groups per row
    if (VIEWS) {
        const unsigned long long per_view = G * (unsigned long long)E.H, v = t / per_view;
        if (v >= (unsigned long long)E.views) return;
        t -= v * per_view;
        E.src += 3ull * (unsigned long long)E.W * (unsigned long long)E.H * v;
        E.dst += E.view_bytes * v;
    }
    const unsigned long long yl = t / G;
    if (yl >= (unsigned long long)E.H) return;
    const int y = (int)yl, x0 = (int)(t - yl * G) * 4;
    const int n = E.W - x0 < 4 ? E.W - x0 : 4;
    unsigned long long sp = (unsigned long long)y * (unsigned long long)E.W + (unsigned long long)x0;  // source pixel of x0
    if (E.tile) {
        const unsigned long long k = (unsigned long long)(y / E.tile) * (unsigned long long)E.tiles_x + (unsigned long long)(x0 / E.tile);
        if (k % (unsigned long long)E.nranks != (unsigned long long)E.rank) return;
        if (E.packed) sp = ((k / (unsigned long long)E.nranks) << 10) + (unsigned long long)((y & 31) * 32 + (x0 & 31));
    }
    const float* s = E.src + 3ull * sp;
    float v[12];
    if (n == 4 && ((uintptr_t)s & 15u) == 0) {
        const float4 a = reinterpret_cast<const float4*>(s)[0], b = reinterpret_cast<const float4*>(s)[1], c = reinterpret_cast<const float4*>(s)[2];
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w, v[8] = c.x, v[9] = c.y, v[10] = c.z, v[11] = c.w;
    } else {
        for (int i = 0; i < 12; i++) v[i] = i < 3 * n ? s[i] : 0.0f;
    }
    if (E.format == 2) {  // RGBA8: row H-1-y (Screen::setPixel's flip)
        unsigned char* d = E.dst + (unsigned long long)(E.H - 1 - y) * E.pitch + 4ull * (unsigned long long)x0;
        const unsigned p0 = rgba8(v[0], v[1], v[2]), p1 = rgba8(v[3], v[4], v[5]), p2 = rgba8(v[6], v[7], v[8]), p3 = rgba8(v[9], v[10], v[11]);
        if (n == 4 && ((uintptr_t)d & 15u) == 0) {
            *reinterpret_cast<uint4*>(d) = make_uint4(p0, p1, p2, p3);
        } else {
            const unsigned p[4] = {p0, p1, p2, p3};
            for (int i = 0; i < n; i++) reinterpret_cast<unsigned*>(d)[i] = p[i];
        }
    } else if (E.format == 1) {  // CHW: plane c, row y
        for (int c = 0; c < 3; c++) {
            float* d = reinterpret_cast<float*>(E.dst + ((unsigned long long)c * (unsigned long long)E.H + (unsigned long long)y) * E.pitch) + x0;
            if (n == 4 && ((uintptr_t)d & 15u) == 0) {
                *reinterpret_cast<float4*>(d) = make_float4(v[c], v[3 + c], v[6 + c], v[9 + c]);
            } else {
                for (int i = 0; i < n; i++) d[i] = v[3 * i + c];
            }
        }
    } else {  // RGB_F32
        float* d = reinterpret_cast<float*>(E.dst + (unsigned long long)y * E.pitch) + 3 * x0;
        if (n == 4 && ((uintptr_t)d & 15u) == 0) {
            reinterpret_cast<float4*>(d)[0] = make_float4(v[0], v[1], v[2], v[3]);
            reinterpret_cast<float4*>(d)[1] = make_float4(v[4], v[5], v[6], v[7]);
            reinterpret_cast<float4*>(d)[2] = make_float4(v[8], v[9], v[10], v[11]);
        } else {
            for (int i = 0; i < 3 * n; i++) d[i] = v[i];
        }
    }
}
__global__ __launch_bounds__(256) void k_export_frame(ExportDev E) { export_frame<false>(E); }
__global__ __launch_bounds__(256) void k_export_views(ExportDev E) { export_frame<true>(E); }

static inline unsigned grid_for(unsigned long long n, unsigned block) { return (unsigned)((n + block - 1) / block); }

hipError_t launch_export_frame(const ExportDev& E, hipStream_t s) {
    const unsigned long long views = E.views > 1 ? (unsigned long long)E.views : 1ull;
    const unsigned long long n = (unsigned long long)((E.W + 3) / 4) * (unsigned long long)E.H * views;
    if (n == 0) return hipSuccess;
    if ((n + 255) / 256 > 0xffffffffull) return hipErrorInvalidValue;
    if (views > 1)
        hipLaunchKernelGGL(k_export_views, dim3(grid_for(n, 256)), dim3(256), 0, s, E);
    else
        hipLaunchKernelGGL(k_export_frame, dim3(grid_for(n, 256)), dim3(256), 0, s, E);
    return hipGetLastError();
}

// ---- Geometry buffers (AovDev, trace_kernels.h) ----
// k_aov_fill: one thread per 4 consecutive pixels of a row of a view, as k_export_frame (super-tiles are multiples of 4 pixels wide, so
// the 4 pixels share an owner): the miss values of every requested plane -- depth FLT_MAX, ids CGRT_NO_PRIM / -1, everything else 0 --
// as 16-B stores (the mask: one 4-B store) where the group is whole and its address aligned, element by element otherwise.
__device__ __forceinline__ void fill4(float* d, int n, float v) {
    if (n == 4 && ((uintptr_t)d & 15u) == 0) {
        *reinterpret_cast<float4*>(d) = make_float4(v, v, v, v);
    } else {
        for (int i = 0; i < n; i++) d[i] = v;
    }
}
__device__ __forceinline__ void fill3(float* plane, int chw, unsigned long long view, unsigned long long wh, unsigned long long p, int n) {
    if (chw) {
        for (int c = 0; c < 3; c++) fill4(plane + (3ull * view + (unsigned long long)c) * wh + p, n, 0.0f);
    } else {
        float* d = plane + 3ull * (view * wh + p);
        if (n == 4 && ((uintptr_t)d & 15u) == 0) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4*>(d)[0] = z;
            reinterpret_cast<float4*>(d)[1] = z;
            reinterpret_cast<float4*>(d)[2] = z;
        } else {
            for (int i = 0; i < 3 * n; i++) d[i] = 0.0f;
        }
    }
}
__global__ __launch_bounds__(256) void k_aov_fill(AovDev A) {
    unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long G = (unsigned long long)((A.W + 3) >> 2);  // 4-pixel groups per row
    const unsigned long long per_view = G * (unsigned long long)A.H, view = t / per_view;
    if (view >= (unsigned long long)A.views) return;
    t -= view * per_view;
    const unsigned long long yl = t / G;
    const int y = (int)yl, x0 = (int)(t - yl * G) * 4;
    const int n = A.W - x0 < 4 ? A.W - x0 : 4;
    if (A.nranks > 1) {
        const unsigned long long k = (unsigned long long)(y >> 6) * (unsigned long long)A.tiles_x + (unsigned long long)(x0 >> 6);
        if (k % (unsigned long long)A.nranks != (unsigned long long)A.rank) return;
    }
    const unsigned long long wh = (unsigned long long)A.W * (unsigned long long)A.H;
    const unsigned long long p = (unsigned long long)y * (unsigned long long)A.W + (unsigned long long)x0, q = view * wh + p;
    if (A.depth) fill4(A.depth + q, n, 3.402823466e+38f);  // FLT_MAX: the t a ray that misses keeps
    if (A.normal) fill3(A.normal, A.chw, view, wh, p, n);
    if (A.position) fill3(A.position, A.chw, view, wh, p, n);
    if (A.albedo) fill3(A.albedo, A.chw, view, wh, p, n);
    if (A.prim_id) fill4(reinterpret_cast<float*>(A.prim_id) + q, n, __uint_as_float(0xffffffffu));   // CGRT_NO_PRIM
    if (A.material_id) fill4(reinterpret_cast<float*>(A.material_id) + q, n, __uint_as_float(0xffffffffu));  // -1
    if (A.mask) {
        uint8_t* d = A.mask + q;
        if (n == 4 && ((uintptr_t)d & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(d) = 0u;
        } else {
            for (int i = 0; i < n; i++) d[i] = 0;
        }
    }
}
// k_aov_scatter: entry i of level 0 to its pixel.  The list is in the primary kernel's order (8 x 8 tiles), so a wave's 64 entries are
// row segments of up to 8 pixels: 32-B pieces of a 4-byte plane (measured: DESIGN.md section 5.17).
__device__ __forceinline__ void st3(float* plane, int chw, unsigned long long view, unsigned long long wh, unsigned long long p, F3 v) {
    if (chw) {
        float* d = plane + 3ull * view * wh + p;
        d[0] = v.x;
        d[wh] = v.y;
        d[2 * wh] = v.z;
    } else {
        float* d = plane + 3ull * (view * wh + p);
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
    }
}
__device__ __forceinline__ void aov_entry(const AovDev& A, const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                          const float* __restrict__ normals, const int* __restrict__ item_pixels,
                                          const float* __restrict__ materials, unsigned long long i) {
    const long long pix = item_pixels[i];
    const unsigned long long wh = (unsigned long long)A.W * (unsigned long long)A.H;
    if (pix < 0 || (unsigned long long)pix >= wh * (unsigned long long)A.views) return;  // item outside the frame
    const unsigned long long q = (unsigned long long)pix, view = q / wh, p = q - view * wh;
    const CgrtHitDev h = hits[i];
    if (A.depth) A.depth[q] = h.t;
    if (A.normal) st3(A.normal, A.chw, view, wh, p, ldv(normals + 3 * i));
    if (A.position) {
        const float* r = rays + 7 * i;
        st3(A.position, A.chw, view, wh, p, add(ldv(r), scale(ldv(r + 3), h.t)));  // pointOn (main.cpp:164), as k_shade's
    }
    if (A.albedo) st3(A.albedo, A.chw, view, wh, p, h.material_id >= 0 ? ldv(materials + 8 * h.material_id) : f3(0.f, 0.f, 0.f));
    if (A.prim_id) A.prim_id[q] = h.prim_id;
    if (A.material_id) A.material_id[q] = h.material_id;
    if (A.mask) A.mask[q] = (uint8_t)(h.hit != 0);
}
__global__ __launch_bounds__(256) void k_aov_scatter(AovDev A, const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                     const float* __restrict__ normals, const int* __restrict__ item_pixels,
                                                     const float* __restrict__ materials, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    aov_entry(A, rays, hits, normals, item_pixels, materials, i);
}
__global__ __launch_bounds__(256) void k_aov_scatter_strided(AovDev A, const float* __restrict__ rays, const CgrtHitDev* __restrict__ hits,
                                                             const float* __restrict__ normals, const int* __restrict__ item_pixels,
                                                             const float* __restrict__ materials, unsigned long long n,
                                                             const uint32_t* __restrict__ dcount) {
    const unsigned long long present = *dcount;
    n = present < n ? present : n;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
        aov_entry(A, rays, hits, normals, item_pixels, materials, i);
}
hipError_t launch_aov_fill(const AovDev& A, hipStream_t s) {
    const unsigned long long n = (unsigned long long)((A.W + 3) / 4) * (unsigned long long)A.H * (unsigned long long)A.views;
    if (n == 0) return hipSuccess;
    if ((n + 255) / 256 > 0xffffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_aov_fill, dim3(grid_for(n, 256)), dim3(256), 0, s, A);
    return hipGetLastError();
}
// KERNEL with one thread per entry of the list's n, or KERNEL_strided (the same parameters) with a capped grid (strided_blocks,
// trace_kernels.hip: at most strided_waves() waves, whatever the capacity n), as `grid` says
#define LAUNCH_LIST(KERNEL, block, ...)                                                                         \
    do {                                                                                                        \
        if (grid == GRID_STRIDED)                                                                               \
            hipLaunchKernelGGL(KERNEL##_strided, dim3(strided_blocks(grid_for(n, block), block)), dim3(block), 0, s, __VA_ARGS__); \
        else                                                                                                    \
            hipLaunchKernelGGL(KERNEL, dim3(grid_for(n, block)), dim3(block), 0, s, __VA_ARGS__);               \
    } while (0)
static inline const float4* f4(const float* p) { return reinterpret_cast<const float4*>(p); }
static inline float4* f4(float* p) { return reinterpret_cast<float4*>(p); }

hipError_t launch_aov_scatter(const AovDev& A, const LevelDev& V0, const float* materials, unsigned long long n, hipStream_t s, const uint32_t* dcount,
                              ListGrid grid) {
    if (n && grid == GRID_STRIDED)
        hipLaunchKernelGGL(k_aov_scatter_strided, dim3(strided_blocks(grid_for(n, 256), 256)), dim3(256), 0, s, A, V0.rays, V0.hits, V0.normals, V0.pixels, materials, n,
                           dcount);
    else if (n)
        hipLaunchKernelGGL(k_aov_scatter, dim3(grid_for(n, 256)), dim3(256), 0, s, A, V0.rays, V0.hits, V0.normals, V0.pixels, materials, n);
    return hipGetLastError();
}

hipError_t launch_spawn(const LevelDev& V, const FrameConst& K, unsigned long long n, hipStream_t s, const uint32_t* dcount, ListGrid grid) {
    if (n)
        LAUNCH_LIST(k_spawn, CGRT_SHADE_BLOCK, V.rays, V.hits, V.normals, V.pixels, n, K.materials, K.lights, K.nlights, V.spawn, V.srays, V.sdist,
                    V.sslot, f4(V.lvl), V.next_rays, V.next_pixels, V.counters, dcount);
    return hipGetLastError();
}
hipError_t launch_shade(const LevelDev& V, const FrameConst& K, unsigned long long n, hipStream_t s, const uint32_t* dcount, ListGrid grid) {
    if (n)
        LAUNCH_LIST(k_shade, CGRT_SHADE_BLOCK, V.rays, V.hits, V.normals, V.shits, V.sdist, V.sslot, n, K.materials, K.lights, K.nlights, K.slights,
                    K.nslights, K.lit, K.samples, f4(V.lvl), dcount);
    return hipGetLastError();
}
hipError_t launch_fold(const LevelDev& V, unsigned long long n, hipStream_t s, const uint32_t* dcount, ListGrid grid) {
    if (n) LAUNCH_LIST(k_fold, 256, f4(V.lvl), f4(V.child_lvl), n, dcount);
    return hipGetLastError();
}
hipError_t launch_write_rgb(const LevelDev& V0, const FrameConst& K, bool with_child, unsigned long long n, hipStream_t s, const uint32_t* dcount,
                            ListGrid grid) {
    if (n)
        LAUNCH_LIST(k_write_rgb, 256, f4(V0.lvl), with_child ? f4(V0.child_lvl) : nullptr, n, V0.pixels, K.rgb, dcount);
    return hipGetLastError();
}

hipError_t launch_shade_sets(const LevelDev& V, const FrameConst& K, const SetsDev& T, unsigned long long n, hipStream_t s, const uint32_t* dcount,
                             ListGrid grid) {
    if (n)
        LAUNCH_LIST(k_shade_sets, CGRT_SHADE_BLOCK, V.rays, V.hits, V.normals, V.shits, V.sdist, V.sslot, n, K.materials, K.nlights, K.nslights, K.lit,
                    K.samples, T, f4(V.sets), V.stride, dcount);
    return hipGetLastError();
}
// the sets' forms: one grid row for every set, or (GRID_STRIDED) one capped grid whose threads loop over the sets
hipError_t launch_fold_sets(const LevelDev& V, unsigned long long n, hipStream_t s, const uint32_t* dcount, ListGrid grid) {
    if (n && V.nsets && grid == GRID_STRIDED)
        hipLaunchKernelGGL(k_fold_sets_strided, dim3(strided_blocks(grid_for(n, 256), 256)), dim3(256), 0, s, f4(V.lvl), f4(V.sets), f4(V.child_sets), n, V.stride, V.nsets,
                           dcount);
    else if (n && V.nsets)
        hipLaunchKernelGGL(k_fold_sets, dim3(grid_for(n, 256), V.nsets), dim3(256), 0, s, f4(V.lvl), f4(V.sets), f4(V.child_sets), n, V.stride);
    return hipGetLastError();
}
hipError_t launch_write_rgb_sets(const LevelDev& V0, const FrameConst& K, bool views, bool with_child, unsigned long long n, hipStream_t s,
                                 const uint32_t* dcount, ListGrid grid) {
    if (grid == GRID_STRIDED && !views) return hipErrorInvalidValue;  // (no such kernel: an enqueued batch of sets is a multi-view one)
    if (n && V0.nsets) {
        const dim3 rows(grid_for(n, 256), V0.nsets);
        const float4* const child = with_child ? f4(V0.child_sets) : nullptr;
        if (grid == GRID_STRIDED)
            hipLaunchKernelGGL(k_write_rgb_views_sets_strided, dim3(strided_blocks(grid_for(n, 256), 256)), dim3(256), 0, s, f4(V0.lvl), f4(V0.sets), child, n, V0.stride,
                               V0.nsets, V0.pixels, K.rgb, K.frame_pixels, dcount);
        else if (views)
            hipLaunchKernelGGL(k_write_rgb_views_sets, rows, dim3(256), 0, s, f4(V0.lvl), f4(V0.sets), child, n, V0.stride, V0.pixels, K.rgb, K.frame_pixels);
        else
            hipLaunchKernelGGL(k_write_rgb_sets, rows, dim3(256), 0, s, f4(V0.lvl), f4(V0.sets), child, n, V0.stride, V0.pixels, K.rgb, K.frame_pixels);
    }
    return hipGetLastError();
}

hipError_t launch_resolve_aa(const FrameDev& F, const float* sub, float* out, int packed, hipStream_t s) {
    const unsigned long long n = (unsigned long long)F.nst_rank * 1024ull;
    if (n)
        hipLaunchKernelGGL(k_resolve_aa, dim3(grid_for(n, 256)), dim3(256), 0, s, F, sub, out, packed);
    return hipGetLastError();
}

}  // namespace cgrt
