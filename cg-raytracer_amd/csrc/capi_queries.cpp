// capi_queries.cpp -- the C-ABI's queries on a built scene (include/cgrt.h): visibility, surface attributes and their gradients,
// closest points, crossings, neighbours, signed distance, winding numbers, surface samples, Poisson-disk sets, point-set neighbours, point-set frames, iso-surfaces, grid fields.  None of them touches the scene's frame state (workspace, prediction, hints).
// Every family is ONE body for its host-pointer and its device-pointer entries, written with a QueryCall (capi_internal.h): the argument
// checks in the order include/cgrt.h states (`device`: the pointers' alignment too), the host-only scene, the empty call, then begin,
// in / out per array, the launch on the call's stream, finish.  The exported entries are one-line forwarders.
#include "capi_internal.h"

// The two pieces more than one family shares come first (templates over the kernels' argument records: C++ linkage).

// ---- the slots of the list entries (crossings and neighbours; DESIGN.md sections 5.21 and 5.26): query i's records go to
// [offsets[i], offsets[i + 1]) or [i k, (i + 1) k) of `out`, its full count to counts[i].  The one home of the slot rules, their
// messages and the three slot transfers.
namespace {
const uint64_t kSlotMaxCapacity = 1ull << 37;  // records of 8 bytes: 2^40 bytes, the bound of every output here
struct SlotList {
    bool list;  // false: a count entry, the fields below but counts unused
    const uint64_t* offsets;
    uint32_t k;
    void* out;
    uint64_t capacity;
    uint32_t* counts;
    // host offsets are read here; device offsets are the kernel's to clamp
    int rules(uint64_t n, bool device) const {
        if (!list) return CGRT_OK;
        if ((offsets != nullptr) == (k > 0)) return fail(CGRT_E_ARG, "exactly one of offsets and k > 0 must be given");
        if (capacity > kSlotMaxCapacity) return fail(CGRT_E_ARG, "capacity exceeds 2^37 records");
        if (k && n * (uint64_t)k > capacity) return fail(CGRT_E_ARG, "n * k records exceed capacity");
        if (!device && offsets && n) {
            if (offsets[0] != 0) return fail(CGRT_E_ARG, "offsets must start at 0");
            for (uint64_t i = 0; i < n; i++)
                if (offsets[i + 1] < offsets[i]) return fail(CGRT_E_ARG, "offsets must not decrease");
            if (offsets[n] > capacity) return fail(CGRT_E_ARG, "offsets end beyond capacity");
        }
        return CGRT_OK;
    }
    bool aligned() const { return !((uintptr_t)out % 4 || (uintptr_t)counts % 4 || (uintptr_t)offsets % 8); }
    // the records the call may write, [0, records): with device offsets any record below capacity, with host offsets those they cover
    uint64_t records(uint64_t n, bool device) const { return !list ? 0 : offsets ? (device ? capacity : offsets[n]) : n * (uint64_t)k; }
    bool want_counts() const { return !list || counts != nullptr; }
    // a host call whose every slot is empty and that asks for no count has nothing to write
    bool nothing(uint64_t n, bool device) const { return !device && records(n, false) == 0 && !want_counts(); }
    // slots 1 the offsets, 2 the records, 3 the counts, into the kernel's record (no record to write: the count search)
    template <class Args>
    int transfer(QueryCall& c, uint64_t n, Args* A) const {
        void *doff = nullptr, *dout = nullptr, *dcnt = nullptr;
        A->k = k;
        A->capacity = records(n, c.device);
        CGRT_TRY(c.in(1, offsets, offsets ? (n + 1) * 8 : 0, "d_offsets", &doff));
        CGRT_TRY(c.out(2, out, A->capacity * sizeof(*A->out), "d_out", &dout));
        CGRT_TRY(c.out(3, counts, want_counts() ? n * 4 : 0, "d_counts", &dcnt));
        A->offsets = static_cast<const unsigned long long*>(doff);
        A->out = static_cast<decltype(A->out)>(dout);
        A->counts = static_cast<uint32_t*>(dcnt);
        return CGRT_OK;
    }
};
}  // namespace

// ---- the points of the signed-distance and winding entries (DESIGN.md sections 5.24 and 5.25)
namespace {
// The points of a signed-distance or winding call, a list or a grid whose lanes make their own: the NULL rules, the sizes, and A's points /
// n / origin / spacing / dims (SdfArgs or WindingArgs).  kNoResult: neither output is asked for, which the family reports in its own words.
const int kNoResult = 1;
template <class Args>
int point_source(const float* points, const CgrtGrid* grid, bool is_grid, uint64_t n, bool have_result, Args* A) {
    if (is_grid ? !grid : (n && !points)) return fail(CGRT_E_ARG, is_grid ? "grid is NULL" : "NULL argument");
    if (!have_result) return kNoResult;
    if (is_grid) {
        n = 1;
        for (int c = 0; c < 3; c++) {
            if (grid->dims[c] < 1 || grid->dims[c] > (1u << 24)) return fail(CGRT_E_ARG, "grid dims must be in 1..2^24");
            n *= grid->dims[c];  // (below 2^55 before the test, which follows every factor)
            if (n > 0x7fffffffull) return fail(CGRT_E_ARG, "too many grid points: nx * ny * nz exceeds 0x7fffffff");
            if (!std::isfinite(grid->origin[c]) || !std::isfinite(grid->spacing[c])) return fail(CGRT_E_ARG, "grid origin and spacing must be finite");
            A->origin[c] = grid->origin[c];
            A->spacing[c] = grid->spacing[c];
            A->dims[c] = grid->dims[c];
        }
    } else if (n > 0x7fffffffull) {
        return fail(CGRT_E_ARG, "too many points: n exceeds 0x7fffffff");
    }
    A->points = points;
    A->n = (uint32_t)n;
    return CGRT_OK;
}
}  // namespace

extern "C" {

// ---- visibility queries (include/cgrt.h cgrt_occluded*, cgrt_in_shadow*, cgrt_soft_lit*): the reference's intersect() bool, pointInShadow
// and shading's soft-shadow counts for the caller's rays / points.  Arguments are checked in the order include/cgrt.h states, all before any
// device work; then a host-only scene is CGRT_E_NO_DEVICE.  None of them touches the scene's frame prediction or frame hints.
namespace {
const uint64_t kMaxAnswers = 0x7fffffffull;
// NULL pointers (the rays / points and the output with n > 0, lights missing), then n and n x per_point above 0x7fffffff
int query_args(const CgrtScene* s, const void* in, uint64_t n, const void* out, uint64_t per_point, bool lights_missing) {
    if (!s || (n && (!in || !out)) || lights_missing) return fail(CGRT_E_ARG, "NULL argument");
    if (n > kMaxAnswers || (per_point && n > kMaxAnswers / per_point)) return fail(CGRT_E_ARG, "too many answers: n (x lights) exceeds 0x7fffffff");
    return CGRT_OK;
}
// slots: 0 the rays, 1 the answers
int occluded_query(CgrtScene* s, bool device, const CgrtRay* rays, uint64_t n, uint8_t* hit, void* stream) {
    CGRT_TRY(query_args(s, rays, n, hit, 0, false));
    if (device && (uintptr_t)rays % 4) return fail(CGRT_E_ARG, "d_rays must be 4-byte aligned");
    NEED_DEVICE(s);
    if (n == 0) return CGRT_OK;
    QueryCall c(s, device, stream);
    void *dr = nullptr, *dh = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, rays, n * sizeof(CgrtRay), "d_rays", &dr));
    CGRT_TRY(c.out(1, hit, n, "d_hit", &dh));
    HIP_TRY(launch_occluded(s->dev, static_cast<const float*>(dr), n, static_cast<uint8_t*>(dh), c.stream()));
    return c.finish();
}
// n points x nlights lights (slots: 0 the points, 1 the answers, 3 the lights, host memory in both forms)
int in_shadow_query(CgrtScene* s, bool device, const float* points, uint64_t n, const float* lights, uint32_t nlights, uint8_t* out, void* stream) {
    CGRT_TRY(query_args(s, points, n, out, nlights, nlights && !lights));
    if (device && (uintptr_t)points % 4) return fail(CGRT_E_ARG, "d_points must be 4-byte aligned");
    NEED_DEVICE(s);
    if (n == 0 || nlights == 0) return CGRT_OK;
    QueryCall c(s, device, stream);
    void *dp = nullptr, *dout = nullptr, *dl = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, n * 12, "d_points", &dp));
    CGRT_TRY(c.out(1, out, n * nlights, "d_out", &dout));
    CGRT_TRY(c.host_in(3, lights, (size_t)nlights * 24, &dl));
    HIP_TRY(launch_in_shadow(s->dev, static_cast<const float*>(dp), n, static_cast<const float*>(dl), nlights, static_cast<uint8_t*>(dout), c.stream()));
    return c.finish();
}
// the soft-shadow counts of n points (slots: 0 the points, 1 the counts, zeroed here, 3 the spherical lights, 2 the unit vectors)
int soft_lit_query(CgrtScene* s, bool device, const float* points, uint64_t n, const CgrtSoftShadows* soft, uint32_t* lit, void* stream) {
    const uint64_t SL = soft ? soft->nspherical : 0u;
    CGRT_TRY(query_args(s, points, n, lit, SL, false));
    CGRT_TRY(soft_rules(soft));
    if (device && ((uintptr_t)points % 4 || (uintptr_t)lit % 4)) return fail(CGRT_E_ARG, "d_points and d_lit must be 4-byte aligned");
    NEED_DEVICE(s);
    if (n == 0 || SL == 0) return CGRT_OK;
    QueryCall c(s, device, stream);
    const uint64_t lit_bytes = n * SL * sizeof(uint32_t);
    void *dp = nullptr, *dlit = nullptr, *dl = nullptr, *du = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, n * 12, "d_points", &dp));
    CGRT_TRY(c.out(1, lit, lit_bytes, "d_lit", &dlit));
    CGRT_TRY(c.host_in(3, soft->spherical, SL * 28, &dl));
    CGRT_TRY(c.host_in(2, soft->unit_vectors, (size_t)soft->nunits * 12, &du));
    HIP_TRY(hipMemsetAsync(dlit, 0, lit_bytes, c.stream()));
    // (level stays 0, cgrt_shade_rays' convention: pixel = i, level 0)
    const SoftDev Q = soft_dev(*soft, (unsigned)SL, static_cast<const float*>(dl), static_cast<const float*>(du));
    HIP_TRY(launch_soft_points(s->dev, Q, static_cast<const float*>(dp), n, static_cast<uint32_t*>(dlit), soft->closest_hit ? 0 : 1, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_occluded_device(CgrtScene* s, const CgrtRay* d_rays, uint64_t n, uint8_t* d_hit, void* stream) {
    return occluded_query(s, true, d_rays, n, d_hit, stream);
}
int cgrt_occluded(CgrtScene* s, const CgrtRay* rays, uint64_t n, uint8_t* hit) { return occluded_query(s, false, rays, n, hit, nullptr); }
int cgrt_in_shadow_device(CgrtScene* s, const float* d_points, uint64_t n, const float* lights, uint32_t nlights, uint8_t* d_out, void* stream) {
    return in_shadow_query(s, true, d_points, n, lights, nlights, d_out, stream);
}
int cgrt_in_shadow(CgrtScene* s, const float* points, uint64_t n, const float* lights, uint32_t nlights, uint8_t* out) {
    return in_shadow_query(s, false, points, n, lights, nlights, out, nullptr);
}
int cgrt_soft_lit_device(CgrtScene* s, const float* d_points, uint64_t n, const CgrtSoftShadows* soft, uint32_t* d_lit, void* stream) {
    return soft_lit_query(s, true, d_points, n, soft, d_lit, stream);
}
int cgrt_soft_lit(CgrtScene* s, const float* points, uint64_t n, const CgrtSoftShadows* soft, uint32_t* lit) {
    return soft_lit_query(s, false, points, n, soft, lit, nullptr);
}

// ---- surface attributes (include/cgrt.h cgrt_hit_barycentrics*, cgrt_interpolate_hits*, cgrt_surface_*_device):
// where inside its triangle a hit lies, and a caller's per-vertex table carried there.  Nothing is traced and no scene state is read or
// written except the lookup table below; the checks come in the order include/cgrt.h states, all before any device work.
namespace {
const uint64_t kSurfaceMaxBytes = 1ull << 40;  // an output's size: items x channels x 4 bytes (the kernel indexes with 64 bits; a documented bound)
int surface_channels(uint32_t channels, uint64_t items) {
    if (channels < 1 || channels > 256) return fail(CGRT_E_ARG, "channels must be in 1..256");
    if (items * channels * 4ull > kSurfaceMaxBytes) return fail(CGRT_E_ARG, "output too large: items x channels x 4 exceeds 2^40 bytes");
    return CGRT_OK;
}
// prim_id -> {record, three vertex rows}, made once per scene by its first surface call (later calls: one atomic load)
int surface_lookup(CgrtScene* s, const SurfaceLookup** out) {
    void* p = s->d_surface_lookup.load(std::memory_order_acquire);
    if (!p) {
        std::lock_guard<std::mutex> lk(s->surface_mutex);
        p = s->d_surface_lookup.load(std::memory_order_acquire);
        if (!p) {
            std::vector<SurfaceLookup> T;
            try {
                T.resize(s->ntris);
            } catch (const std::bad_alloc&) {
                return fail(CGRT_E_ALLOC, "host allocation failed");
            }
            const std::vector<TriRecord>& R = s->bvh.tris;
            if (R.size() != s->ntris || s->tri_index.size() != 3 * (size_t)s->ntris) return fail(CGRT_E_ARG, "the scene's records do not cover its triangles");
            for (size_t k = 0; k < R.size(); k++) {
                const uint32_t prim = R[k].prim_id;
                if (prim >= s->ntris) return fail(CGRT_E_ARG, "a triangle record carries a primitive id out of range");
                T[prim].record = s->bvh.tri_base + (uint32_t)k;
                for (int c = 0; c < 3; c++) T[prim].v[c] = s->tri_index[3 * (size_t)prim + c];
            }
            const size_t bytes = T.size() * sizeof(SurfaceLookup);
            void* d = nullptr;
            HIP_TRY(hipMalloc(&d, bytes ? bytes : 16));
            if (bytes) {
                const hipError_t e = staged_h2d(d, T.data(), bytes);  // (complete when it returns: every later launch sees the table)
                if (e != hipSuccess) {
                    (void)hipFree(d);
                    return hip_fail(e, "uploading the surface lookup table");
                }
            }
            s->device_bytes += bytes;
            s->d_surface_lookup.store(d, std::memory_order_release);
            p = d;
        }
    }
    *out = static_cast<const SurfaceLookup*>(p);
    return CGRT_OK;
}
SurfaceDev surface_dev(const CgrtScene* s, const SurfaceLookup* lookup, uint64_t n, const float* d_attr, uint32_t channels, float* d_bary,
                       float* d_out, int chw) {
    SurfaceDev A{};
    A.tris = s->dev.tris;
    A.lookup = lookup;
    A.ntris = s->dev.ntris;
    A.n = (uint32_t)n;
    A.attr = d_out ? d_attr : nullptr;
    A.channels = d_out ? channels : 0;
    A.bary = d_bary;
    A.out = d_out;
    A.chw = chw ? 1 : 0;
    A.vec4 = d_out && channels % 4 == 0 && (uintptr_t)d_attr % 16 == 0 && (uintptr_t)d_out % 16 == 0;
    return A;
}
// the list forms' checks up to the host-only scene (attr: the call interpolates; device: the pointers' alignment is checked too)
int surface_list_args(const CgrtScene* s, const void* rays, const void* hits, uint64_t n, bool attr, const void* table, uint32_t channels,
                      const void* out, bool device) {
    if (!s || (n && (!rays || !hits || !out || (attr && !table)))) return fail(CGRT_E_ARG, "NULL argument");
    if (n > 0x7fffffffull) return fail(CGRT_E_ARG, "too many hits: n exceeds 0x7fffffff");
    if (attr) {
        const int rc = surface_channels(channels, n);
        if (rc) return rc;
    }
    if (device && ((uintptr_t)rays % 4 || (uintptr_t)hits % 4 || (uintptr_t)table % 4 || (uintptr_t)out % 4))
        return fail(CGRT_E_ARG, "device pointers must be 4-byte aligned");
    return CGRT_OK;
}
// d_bary or d_out (with d_attr, channels) of n hits on `st`; every pointer device memory
int surface_list_launch(CgrtScene* s, const void* d_rays, const void* d_hits, uint64_t n, const float* d_attr, uint32_t channels, float* d_bary,
                        float* d_out, hipStream_t st) {
    const SurfaceLookup* lookup = nullptr;
    const int rc = surface_lookup(s, &lookup);
    if (rc) return rc;
    SurfaceDev A = surface_dev(s, lookup, n, d_attr, channels, d_bary, d_out, 0);
    A.rays = static_cast<const float*>(d_rays);
    A.hits = static_cast<const CgrtHitDev*>(d_hits);
    HIP_TRY(launch_surface(A, SURFACE_LIST, st));
    return CGRT_OK;
}
// cgrt_hit_barycentrics* (attr false: res is bary) and cgrt_interpolate_hits* (res is out); slots: 0 rays, 1 hits, 2 the result, 3 the table
int surface_list(CgrtScene* s, bool device, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, bool attr, const float* table, uint32_t channels,
                 float* res, void* stream) {
    CGRT_TRY(surface_list_args(s, rays, hits, n, attr, table, channels, res, device));
    NEED_DEVICE(s);
    if (n == 0) return CGRT_OK;
    QueryCall c(s, device, stream);
    void *dr = nullptr, *dh = nullptr, *dt = nullptr, *dres = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, rays, n * sizeof(CgrtRay), "d_rays", &dr));
    CGRT_TRY(c.in(1, hits, n * sizeof(CgrtHit), "d_hits", &dh));
    CGRT_TRY(c.in(3, table, attr ? (uint64_t)s->nverts * channels * 4ull : 0, "d_attr", &dt));
    CGRT_TRY(c.out(2, res, n * (attr ? channels : 3u) * 4ull, attr ? "d_out" : "d_bary", &dres));
    CGRT_TRY(surface_list_launch(s, dr, dh, n, static_cast<const float*>(dt), channels, attr ? nullptr : static_cast<float*>(dres),
                                 attr ? static_cast<float*>(dres) : nullptr, c.stream()));
    return c.finish();
}
// cgrt_surface_views_device and its ray-camera twin (exactly one of cams, raycams)
int surface_frames_device(CgrtScene* s, const CgrtCamera* cams, const CgrtRayCamera* raycams, uint32_t nviews, int W, int H, const float* d_depth,
                          const uint32_t* d_prim_id, const float* d_attr, uint32_t channels, float* d_bary, float* d_out, int chw, void* stream) {
    if (!s || !d_depth || !d_prim_id || (!d_bary && !d_out) || (d_out && !d_attr)) return fail(CGRT_E_ARG, "NULL argument");
    int rc = views_args(raycams ? static_cast<const void*>(raycams) : cams, nviews, W, H, raycams);
    if (rc) return rc;
    const uint64_t npix = (uint64_t)nviews * (uint64_t)W * (uint64_t)H;
    if (d_out && (rc = surface_channels(channels, npix)) != CGRT_OK) return rc;
    if ((uintptr_t)d_depth % 4 || (uintptr_t)d_prim_id % 4 || (uintptr_t)d_attr % 4 || (uintptr_t)d_bary % 4 || (uintptr_t)d_out % 4)
        return fail(CGRT_E_ARG, "device pointers must be 4-byte aligned");
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = check_device_span(s, d_depth, npix * 4, "d_depth")) != CGRT_OK) return rc;
    if ((rc = check_device_span(s, d_prim_id, npix * 4, "d_prim_id")) != CGRT_OK) return rc;
    if (d_out && (rc = check_device_span(s, d_attr, (uint64_t)s->nverts * channels * 4ull, "d_attr")) != CGRT_OK) return rc;
    if (d_bary && (rc = check_device_span(s, d_bary, npix * 12, "d_bary")) != CGRT_OK) return rc;
    if (d_out && (rc = check_device_span(s, d_out, npix * channels * 4ull, "d_out")) != CGRT_OK) return rc;
    const SurfaceLookup* lookup = nullptr;
    if ((rc = surface_lookup(s, &lookup)) != CGRT_OK) return rc;
    SurfaceDev A = surface_dev(s, lookup, npix, d_attr, channels, d_bary, d_out, chw);
    A.depth = d_depth;
    A.prim = d_prim_id;
    A.W = W;
    A.H = H;
    A.plane = (uint32_t)((uint64_t)W * (uint64_t)H);
    hipStream_t const st = static_cast<hipStream_t>(stream);
    return launch_with_view_table(s, view_table(cams, raycams, nviews), st, [&](const void* d_table) {
        A.cams = d_table;
        return launch_surface(A, raycams ? SURFACE_RAYCAM : SURFACE_TRACKBALL, st);
    });
}

// ---- the adjoint with respect to the table (include/cgrt.h cgrt_interpolate_hits_grad*, cgrt_surface_*_grad_device; DESIGN.md section
// 5.23): twins of the entries above, grad_out in the place of out and grad_attr in the place of attr, the same checks in the same order.
SurfaceGradDev surface_grad_dev(const CgrtScene* s, const SurfaceLookup* lookup, uint64_t n, const float* d_grad_out, uint32_t channels,
                                float* d_grad_attr, int chw) {
    SurfaceGradDev A{};
    A.tris = s->dev.tris;
    A.lookup = lookup;
    A.ntris = s->dev.ntris;
    A.n = (uint32_t)n;
    A.grad_out = d_grad_out;
    A.channels = channels;
    A.grad_attr = d_grad_attr;
    A.chw = chw ? 1 : 0;
    surface_grad_policy(channels, A.chw, &A.by_item, &A.combine);
    return A;
}
// The reproducible form's workspace as the caller gave it (include/cgrt.h cgrt_*_grad_repro*); null: the float form.
struct ReproWorkspace {
    void* d;
    uint64_t bytes;
};
// d_workspace NULL (with the family's text for it), misaligned or below `need` bytes (what `entry`, the family's *_workspace entry,
// returns): the checks that follow the twin's, before the host-only scene
int repro_workspace_args(const ReproWorkspace* ws, uint64_t need, const char* null_text, const char* entry) {
    if (!ws) return CGRT_OK;
    if (!ws->d) return fail(CGRT_E_ARG, null_text);
    if ((uintptr_t)ws->d % 8) return fail(CGRT_E_ARG, "d_workspace must be 8-byte aligned");
    if (ws->bytes < need) return fail(CGRT_E_ARG, std::string("workspace_bytes is below ") + entry);
    return CGRT_OK;
}
// The device workspace of a call: the caller's `ws`, checked; else slot 4 of `lane` (the host form of a reproducible call); else none
int repro_workspace_device(const CgrtScene* s, const ReproWorkspace* ws, LaneCall* lane, uint64_t need, void** d) {
    *d = nullptr;
    if (ws) {
        *d = ws->d;
        return check_device_span(s, ws->d, need, "d_workspace");
    }
    if (lane) HIP_TRY(lane->scratch(4, need, d));
    return CGRT_OK;
}
int surface_repro_args(const CgrtScene* s, uint32_t channels, const ReproWorkspace* ws) {
    return repro_workspace_args(ws, repro_workspace_bytes((uint64_t)s->nverts * channels), "NULL argument", "cgrt_surface_grad_repro_workspace");
}
int surface_list_grad_launch(CgrtScene* s, const void* d_rays, const void* d_hits, uint64_t n, const float* d_grad_out, uint32_t channels,
                             float* d_grad_attr, void* d_workspace, hipStream_t st) {
    const SurfaceLookup* lookup = nullptr;
    const int rc = surface_lookup(s, &lookup);
    if (rc) return rc;
    SurfaceGradDev A = surface_grad_dev(s, lookup, n, d_grad_out, channels, d_grad_attr, 0);
    A.rays = static_cast<const float*>(d_rays);
    A.hits = static_cast<const CgrtHitDev*>(d_hits);
    if (d_workspace)
        HIP_TRY(launch_surface_grad_repro(A, SURFACE_LIST, (uint64_t)s->nverts * channels, d_workspace, st));
    else
        HIP_TRY(launch_surface_grad(A, SURFACE_LIST, st));
    return CGRT_OK;
}
// cgrt_interpolate_hits_grad*; slots: 0 rays, 1 hits, 2 grad_out, 3 grad_attr (host form: uploaded, accumulated into, downloaded).
// repro: the reproducible form, whose workspace is the caller's `ws` (device form) or the lane's slot 4 (host form)
int surface_list_grad(CgrtScene* s, bool device, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, const float* grad_out, uint32_t channels,
                      float* grad_attr, bool repro, const ReproWorkspace* ws, void* stream) {
    CGRT_TRY(surface_list_args(s, rays, hits, n, true, grad_attr, channels, grad_out, device));
    if (n) CGRT_TRY(surface_repro_args(s, channels, ws));
    NEED_DEVICE(s);
    if (n == 0) return CGRT_OK;
    QueryCall c(s, device, stream);
    void *dr = nullptr, *dh = nullptr, *dt = nullptr, *dgo = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, rays, n * sizeof(CgrtRay), "d_rays", &dr));
    CGRT_TRY(c.in(1, hits, n * sizeof(CgrtHit), "d_hits", &dh));
    CGRT_TRY(c.inout(3, grad_attr, (uint64_t)s->nverts * channels * 4ull, "d_grad_attr", &dt));
    CGRT_TRY(c.in(2, grad_out, n * channels * 4ull, "d_grad_out", &dgo));
    void* dws = nullptr;
    CGRT_TRY(repro_workspace_device(s, ws, repro ? &c.c : nullptr, repro_workspace_bytes((uint64_t)s->nverts * channels), &dws));
    CGRT_TRY(surface_list_grad_launch(s, dr, dh, n, static_cast<const float*>(dgo), channels, static_cast<float*>(dt), dws, c.stream()));
    return c.finish();
}
// cgrt_surface_views_grad_device and its ray-camera twin (exactly one of cams, raycams)
int surface_frames_grad_device(CgrtScene* s, const CgrtCamera* cams, const CgrtRayCamera* raycams, uint32_t nviews, int W, int H,
                               const float* d_depth, const uint32_t* d_prim_id, const float* d_grad_out, uint32_t channels, int chw,
                               float* d_grad_attr, const ReproWorkspace* ws, void* stream) {
    if (!s || !d_depth || !d_prim_id || !d_grad_out || !d_grad_attr) return fail(CGRT_E_ARG, "NULL argument");
    int rc = views_args(raycams ? static_cast<const void*>(raycams) : cams, nviews, W, H, raycams);
    if (rc) return rc;
    const uint64_t npix = (uint64_t)nviews * (uint64_t)W * (uint64_t)H;
    if ((rc = surface_channels(channels, npix)) != CGRT_OK) return rc;
    if ((uintptr_t)d_depth % 4 || (uintptr_t)d_prim_id % 4 || (uintptr_t)d_grad_attr % 4 || (uintptr_t)d_grad_out % 4)
        return fail(CGRT_E_ARG, "device pointers must be 4-byte aligned");
    if ((rc = surface_repro_args(s, channels, ws)) != CGRT_OK) return rc;
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = check_device_span(s, d_depth, npix * 4, "d_depth")) != CGRT_OK) return rc;
    if ((rc = check_device_span(s, d_prim_id, npix * 4, "d_prim_id")) != CGRT_OK) return rc;
    if ((rc = check_device_span(s, d_grad_attr, (uint64_t)s->nverts * channels * 4ull, "d_grad_attr")) != CGRT_OK) return rc;
    if ((rc = check_device_span(s, d_grad_out, npix * channels * 4ull, "d_grad_out")) != CGRT_OK) return rc;
    const uint64_t elements = (uint64_t)s->nverts * channels;
    void* dws = nullptr;
    if ((rc = repro_workspace_device(s, ws, nullptr, repro_workspace_bytes(elements), &dws)) != CGRT_OK) return rc;
    const SurfaceLookup* lookup = nullptr;
    if ((rc = surface_lookup(s, &lookup)) != CGRT_OK) return rc;
    SurfaceGradDev A = surface_grad_dev(s, lookup, npix, d_grad_out, channels, d_grad_attr, chw);
    A.depth = d_depth;
    A.prim = d_prim_id;
    A.W = W;
    A.H = H;
    A.plane = (uint32_t)((uint64_t)W * (uint64_t)H);
    hipStream_t const st = static_cast<hipStream_t>(stream);
    return launch_with_view_table(s, view_table(cams, raycams, nviews), st, [&](const void* d_table) {
        A.cams = d_table;
        if (dws) return launch_surface_grad_repro(A, raycams ? SURFACE_RAYCAM : SURFACE_TRACKBALL, elements, dws, st);
        return launch_surface_grad(A, raycams ? SURFACE_RAYCAM : SURFACE_TRACKBALL, st);
    });
}
}  // namespace

int cgrt_interpolate_hits_grad(CgrtScene* s, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, const float* grad_out, uint32_t channels,
                               float* grad_attr) {
    return surface_list_grad(s, false, rays, hits, n, grad_out, channels, grad_attr, false, nullptr, nullptr);
}
int cgrt_surface_grad_repro_workspace(CgrtScene* s, uint32_t channels, uint64_t* bytes) {
    if (!s || !bytes) return fail(CGRT_E_ARG, "NULL argument");
    if (channels < 1 || channels > 256) return fail(CGRT_E_ARG, "channels must be in 1..256");
    *bytes = repro_workspace_bytes((uint64_t)s->nverts * channels);
    return CGRT_OK;
}
int cgrt_interpolate_hits_grad_repro(CgrtScene* s, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, const float* grad_out,
                                     uint32_t channels, float* grad_attr) {
    return surface_list_grad(s, false, rays, hits, n, grad_out, channels, grad_attr, true, nullptr, nullptr);
}
int cgrt_interpolate_hits_grad_repro_device(CgrtScene* s, const CgrtRay* d_rays, const CgrtHit* d_hits, uint64_t n, const float* d_grad_out,
                                            uint32_t channels, float* d_grad_attr, void* d_workspace, uint64_t workspace_bytes, void* stream) {
    const ReproWorkspace ws{d_workspace, workspace_bytes};
    return surface_list_grad(s, true, d_rays, d_hits, n, d_grad_out, channels, d_grad_attr, true, &ws, stream);
}
int cgrt_surface_views_grad_repro_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                                         const uint32_t* d_prim_id, const float* d_grad_out, uint32_t channels, int chw, float* d_grad_attr,
                                         void* d_workspace, uint64_t workspace_bytes, void* stream) {
    const ReproWorkspace ws{d_workspace, workspace_bytes};
    return surface_frames_grad_device(s, cams, nullptr, nviews, W, H, d_depth, d_prim_id, d_grad_out, channels, chw, d_grad_attr, &ws, stream);
}
int cgrt_surface_raycams_grad_repro_device(CgrtScene* s, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                                           const uint32_t* d_prim_id, const float* d_grad_out, uint32_t channels, int chw, float* d_grad_attr,
                                           void* d_workspace, uint64_t workspace_bytes, void* stream) {
    const ReproWorkspace ws{d_workspace, workspace_bytes};
    return surface_frames_grad_device(s, nullptr, cams, nviews, W, H, d_depth, d_prim_id, d_grad_out, channels, chw, d_grad_attr, &ws, stream);
}
int cgrt_interpolate_hits_grad_device(CgrtScene* s, const CgrtRay* d_rays, const CgrtHit* d_hits, uint64_t n, const float* d_grad_out,
                                      uint32_t channels, float* d_grad_attr, void* stream) {
    return surface_list_grad(s, true, d_rays, d_hits, n, d_grad_out, channels, d_grad_attr, false, nullptr, stream);
}
int cgrt_hit_barycentrics(CgrtScene* s, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, float* bary) {
    return surface_list(s, false, rays, hits, n, false, nullptr, 0, bary, nullptr);
}
int cgrt_hit_barycentrics_device(CgrtScene* s, const CgrtRay* d_rays, const CgrtHit* d_hits, uint64_t n, float* d_bary, void* stream) {
    return surface_list(s, true, d_rays, d_hits, n, false, nullptr, 0, d_bary, stream);
}
int cgrt_interpolate_hits(CgrtScene* s, const CgrtRay* rays, const CgrtHit* hits, uint64_t n, const float* attr, uint32_t channels, float* out) {
    return surface_list(s, false, rays, hits, n, true, attr, channels, out, nullptr);
}
int cgrt_interpolate_hits_device(CgrtScene* s, const CgrtRay* d_rays, const CgrtHit* d_hits, uint64_t n, const float* d_attr, uint32_t channels,
                                 float* d_out, void* stream) {
    return surface_list(s, true, d_rays, d_hits, n, true, d_attr, channels, d_out, stream);
}
int cgrt_surface_views_grad_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                                   const uint32_t* d_prim_id, const float* d_grad_out, uint32_t channels, int chw, float* d_grad_attr,
                                   void* stream) {
    return surface_frames_grad_device(s, cams, nullptr, nviews, W, H, d_depth, d_prim_id, d_grad_out, channels, chw, d_grad_attr, nullptr, stream);
}
int cgrt_surface_raycams_grad_device(CgrtScene* s, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                                     const uint32_t* d_prim_id, const float* d_grad_out, uint32_t channels, int chw, float* d_grad_attr,
                                     void* stream) {
    return surface_frames_grad_device(s, nullptr, cams, nviews, W, H, d_depth, d_prim_id, d_grad_out, channels, chw, d_grad_attr, nullptr, stream);
}

int cgrt_surface_views_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* d_depth, const uint32_t* d_prim_id,
                              const float* d_attr, uint32_t channels, float* d_bary, float* d_out, int chw, void* stream) {
    return surface_frames_device(s, cams, nullptr, nviews, W, H, d_depth, d_prim_id, d_attr, channels, d_bary, d_out, chw, stream);
}
int cgrt_surface_raycams_device(CgrtScene* s, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const float* d_depth,
                                const uint32_t* d_prim_id, const float* d_attr, uint32_t channels, float* d_bary, float* d_out, int chw, void* stream) {
    return surface_frames_device(s, nullptr, cams, nviews, W, H, d_depth, d_prim_id, d_attr, channels, d_bary, d_out, chw, stream);
}

// ---- closest-point queries (include/cgrt.h cgrt_closest_points*): the nearest surface point of every query point.
// Nothing is traced and no scene state is read or written; the checks come in the order include/cgrt.h states, all before any device work.
namespace {
static_assert(sizeof(CgrtClosest) == sizeof(CgrtClosestDev), "CgrtClosest is what the kernels write");
// slots: 0 the points, 1 the records; how: 0 tree search, 1 brute force, 2 counted tree search (host form only: `work` in the place of out)
int closest_query(CgrtScene* s, bool device, const float* points, uint64_t n, float max_dist2, CgrtClosest* out, int how, uint64_t* work,
                  void* stream) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    if (n && (!points || (how == 2 ? !work : !out))) return fail(CGRT_E_ARG, "NULL argument");
    if (n > 0x7fffffffull) return fail(CGRT_E_ARG, "too many queries: n exceeds 0x7fffffff");
    if (!(max_dist2 >= 0.0f)) return fail(CGRT_E_ARG, "max_dist2 must be a number >= 0 (+inf: unbounded)");
    if (device && ((uintptr_t)points % 4 || (uintptr_t)out % 4)) return fail(CGRT_E_ARG, "device pointers must be 4-byte aligned");
    NEED_DEVICE(s);
    if (n == 0) return CGRT_OK;
    QueryCall c(s, device, stream);
    void *dp = nullptr, *dout = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, n * 12, "d_points", &dp));
    CGRT_TRY(c.out(1, out, n * sizeof(CgrtClosest), "d_out", &dout));
    const float* const P = static_cast<const float*>(dp);
    CgrtClosestDev* const R = static_cast<CgrtClosestDev*>(dout);
    if (how == 2) {
        CGRT_TRY(c.zero_counters(2));
        HIP_TRY(launch_closest(s->dev, P, n, max_dist2, R, c.counters(), c.stream()));
        return c.read_counters(work, 2);
    }
    if (how == 1)
        HIP_TRY(launch_closest_brute(s->dev, P, n, max_dist2, R, c.stream()));
    else
        HIP_TRY(launch_closest(s->dev, P, n, max_dist2, R, nullptr, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_closest_points(CgrtScene* s, const float* points, uint64_t n, float max_dist2, CgrtClosest* out) {
    return closest_query(s, false, points, n, max_dist2, out, 0, nullptr, nullptr);
}
int cgrt_closest_points_brute(CgrtScene* s, const float* points, uint64_t n, float max_dist2, CgrtClosest* out) {
    return closest_query(s, false, points, n, max_dist2, out, 1, nullptr, nullptr);
}
int cgrt_debug_closest_work(CgrtScene* s, const float* points, uint64_t n, float max_dist2, uint64_t* out2) {
    return closest_query(s, false, points, n, max_dist2, nullptr, 2, out2, nullptr);
}
int cgrt_closest_points_device(CgrtScene* s, const float* d_points, uint64_t n, float max_dist2, CgrtClosest* d_out, void* stream) {
    return closest_query(s, true, d_points, n, max_dist2, d_out, 0, nullptr, stream);
}

// ---- crossing queries (include/cgrt.h cgrt_count_crossings*, cgrt_list_crossings*): every triangle a ray passes
// through, counted or listed in (t, prim_id) order.  No scene state is read or written; the checks come in the order include/cgrt.h
// states, all before any device work.
namespace {
static_assert(sizeof(CgrtCrossing) == sizeof(CgrtCrossingDev), "CgrtCrossing is what the kernels write");
// where the conservative box test's argument does not hold the whole call tests every triangle: a wild triangle is accepted by every ray
// wherever its boxes are, and a non-finite vertex leaves its boxes meaningless
bool crossing_brute_scene(const CgrtScene* s) {
    if (!s->bvh.geometry_finite) return true;
    for (uint8_t w : s->bvh.leaf_wild)
        if (w) return true;
    return false;
}
// slots: 0 the rays, then the list's; how: 0 tree search, 1 brute force, 2 counted tree search (count mode; host form only: `work`)
int crossing_query(CgrtScene* s, bool device, const CgrtRay* rays, uint64_t n, const SlotList& L, int how, uint64_t* work, void* stream) {
    const void* const result = how == 2 ? static_cast<const void*>(work) : (L.list ? L.out : static_cast<const void*>(L.counts));
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    if (n && (!rays || !result)) return fail(CGRT_E_ARG, "NULL argument");
    if (n > 0x7fffffffull) return fail(CGRT_E_ARG, "too many rays: n exceeds 0x7fffffff");
    CGRT_TRY(L.rules(n, device));
    if (device && ((uintptr_t)rays % 4 || !L.aligned())) return fail(CGRT_E_ARG, "device pointers must be aligned to their elements");
    NEED_DEVICE(s);
    if (n == 0 || L.nothing(n, device)) return CGRT_OK;
    QueryCall c(s, device, stream);
    void* dr = nullptr;
    CrossingArgs A{};
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, rays, n * sizeof(CgrtRay), "d_rays", &dr));
    CGRT_TRY(L.transfer(c, n, &A));
    A.rays = static_cast<const float*>(dr);
    A.n = n;
    const bool brute = how == 1 || crossing_brute_scene(s);
    if (how == 2) {
        CGRT_TRY(c.zero_counters(2));
        HIP_TRY(launch_crossings(s->dev, A, brute, c.counters(), c.stream()));
        return c.read_counters(work, 2);
    }
    HIP_TRY(launch_crossings(s->dev, A, brute, nullptr, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_count_crossings(CgrtScene* s, const CgrtRay* rays, uint64_t n, uint32_t* counts) {
    return crossing_query(s, false, rays, n, {false, nullptr, 0, nullptr, 0, counts}, 0, nullptr, nullptr);
}
int cgrt_count_crossings_device(CgrtScene* s, const CgrtRay* d_rays, uint64_t n, uint32_t* d_counts, void* stream) {
    return crossing_query(s, true, d_rays, n, {false, nullptr, 0, nullptr, 0, d_counts}, 0, nullptr, stream);
}
int cgrt_list_crossings(CgrtScene* s, const CgrtRay* rays, uint64_t n, const uint64_t* offsets, uint32_t k, CgrtCrossing* out, uint64_t capacity,
                        uint32_t* counts) {
    return crossing_query(s, false, rays, n, {true, offsets, k, out, capacity, counts}, 0, nullptr, nullptr);
}
int cgrt_list_crossings_device(CgrtScene* s, const CgrtRay* d_rays, uint64_t n, const uint64_t* d_offsets, uint32_t k, CgrtCrossing* d_out,
                               uint64_t capacity, uint32_t* d_counts, void* stream) {
    return crossing_query(s, true, d_rays, n, {true, d_offsets, k, d_out, capacity, d_counts}, 0, nullptr, stream);
}
int cgrt_list_crossings_brute(CgrtScene* s, const CgrtRay* rays, uint64_t n, const uint64_t* offsets, uint32_t k, CgrtCrossing* out,
                              uint64_t capacity, uint32_t* counts) {
    return crossing_query(s, false, rays, n, {true, offsets, k, out, capacity, counts}, 1, nullptr, nullptr);
}
int cgrt_debug_crossing_work(CgrtScene* s, const CgrtRay* rays, uint64_t n, uint64_t* out2) {
    return crossing_query(s, false, rays, n, {false, nullptr, 0, nullptr, 0, nullptr}, 2, out2, nullptr);
}

// ---- neighbour queries (include/cgrt.h cgrt_count_neighbors*, cgrt_list_neighbors*): every triangle within a
// query point's squared radius, counted or listed in (dist2, prim_id) order.  No scene state is read or written; the checks come in the
// order include/cgrt.h states, all before any device work.
namespace {
static_assert(sizeof(CgrtNeighbor) == sizeof(CgrtNeighborDev), "CgrtNeighbor is what the kernels write");
// slots: 0 the points, 4 the radii, then the list's; how: 0 tree search, 1 brute force, 2 counted tree search (host form only: `work`;
// L is k records per query of the lane's own, or with k == 0 the count search)
int neighbor_query(CgrtScene* s, bool device, const float* points, uint64_t n, const float* radius2, float max_dist2, const SlotList& L, int how,
                   uint64_t* work, void* stream) {
    const void* const result = how == 2 ? static_cast<const void*>(work) : (L.list ? L.out : static_cast<const void*>(L.counts));
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    if (n && (!points || !result)) return fail(CGRT_E_ARG, "NULL argument");
    if (n > 0x7fffffffull) return fail(CGRT_E_ARG, "too many queries: n exceeds 0x7fffffff");
    if (!(max_dist2 >= 0.0f)) return fail(CGRT_E_ARG, "max_dist2 must be a number >= 0 (+inf: unbounded)");
    CGRT_TRY(L.rules(n, device));
    if (device && ((uintptr_t)points % 4 || (uintptr_t)radius2 % 4 || !L.aligned()))
        return fail(CGRT_E_ARG, "device pointers must be aligned to their elements");
    NEED_DEVICE(s);
    if (n == 0 || L.nothing(n, device)) return CGRT_OK;
    QueryCall c(s, device, stream);
    void *dp = nullptr, *drad = nullptr;
    NeighborArgs A{};
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, n * 12, "d_points", &dp));
    CGRT_TRY(c.in(4, radius2, radius2 ? n * 4 : 0, "d_radius2", &drad));
    CGRT_TRY(L.transfer(c, n, &A));
    A.points = static_cast<const float*>(dp);
    A.radius2 = static_cast<const float*>(drad);
    A.max_dist2 = max_dist2;
    A.n = n;
    if (how == 2) {
        CGRT_TRY(c.zero_counters(2));
        HIP_TRY(launch_neighbors(s->dev, A, false, c.counters(), c.stream()));
        return c.read_counters(work, 2);
    }
    HIP_TRY(launch_neighbors(s->dev, A, how == 1, nullptr, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_count_neighbors(CgrtScene* s, const float* points, uint64_t n, const float* radius2, float max_dist2, uint32_t* counts) {
    return neighbor_query(s, false, points, n, radius2, max_dist2, {false, nullptr, 0, nullptr, 0, counts}, 0, nullptr, nullptr);
}
int cgrt_count_neighbors_device(CgrtScene* s, const float* d_points, uint64_t n, const float* d_radius2, float max_dist2, uint32_t* d_counts,
                                void* stream) {
    return neighbor_query(s, true, d_points, n, d_radius2, max_dist2, {false, nullptr, 0, nullptr, 0, d_counts}, 0, nullptr, stream);
}
int cgrt_list_neighbors(CgrtScene* s, const float* points, uint64_t n, const float* radius2, float max_dist2, const uint64_t* offsets, uint32_t k,
                        CgrtNeighbor* out, uint64_t capacity, uint32_t* counts) {
    return neighbor_query(s, false, points, n, radius2, max_dist2, {true, offsets, k, out, capacity, counts}, 0, nullptr, nullptr);
}
int cgrt_list_neighbors_device(CgrtScene* s, const float* d_points, uint64_t n, const float* d_radius2, float max_dist2, const uint64_t* d_offsets,
                               uint32_t k, CgrtNeighbor* d_out, uint64_t capacity, uint32_t* d_counts, void* stream) {
    return neighbor_query(s, true, d_points, n, d_radius2, max_dist2, {true, d_offsets, k, d_out, capacity, d_counts}, 0, nullptr, stream);
}
int cgrt_list_neighbors_brute(CgrtScene* s, const float* points, uint64_t n, const float* radius2, float max_dist2, const uint64_t* offsets,
                              uint32_t k, CgrtNeighbor* out, uint64_t capacity, uint32_t* counts) {
    return neighbor_query(s, false, points, n, radius2, max_dist2, {true, offsets, k, out, capacity, counts}, 1, nullptr, nullptr);
}
int cgrt_debug_neighbor_work(CgrtScene* s, const float* points, uint64_t n, const float* radius2, float max_dist2, uint32_t k, uint64_t* out2) {
    // (n <= 0x7fffffff is checked before the capacity n k is looked at)
    return neighbor_query(s, false, points, n, radius2, max_dist2, {k > 0, nullptr, k, nullptr, n * (uint64_t)k, nullptr}, 2, out2, nullptr);
}

// ---- signed distance and occupancy (include/cgrt.h cgrt_signed_distance*): the closest-point search and the parity
// vote of a few count searches, fused per point.  No scene state is read or written; the checks come in the order include/cgrt.h states,
// all before any device work.
namespace {
std::atomic<int> g_sdf_grid_linear{0};  // cgrt_debug_set_sdf_grid_mapping
const float kSdfDefaultDirs[CGRT_SDF_DEFAULT_NDIRS][3] = CGRT_SDF_DEFAULT_DIRS;
static_assert(sizeof(SdfArgs{}.dirs) == sizeof(CgrtSdfParams{}.dirs) && CGRT_SDF_MAX_DIRS == 7, "the kernel's directions are the parameters'");
// slots: 0 the points, 1 sdf, 2 inside; work: the counted launch (host form only: out5 in the place of both outputs)
int sdf_query(CgrtScene* s, bool device, const float* points, const CgrtGrid* grid, bool is_grid, uint64_t n, const CgrtSdfParams* params,
              float* sdf, uint8_t* inside, int want_sdf, uint64_t* work, void* stream) {
    SdfArgs A{};
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    const int rc = point_source(points, grid, is_grid, n, sdf || inside || work, &A);
    if (rc) return rc == kNoResult ? fail(CGRT_E_ARG, "NULL argument: neither sdf nor inside is asked for") : rc;
    A.max_dist2 = params ? params->max_dist2 : INFINITY;
    if (!(A.max_dist2 >= 0.0f)) return fail(CGRT_E_ARG, "max_dist2 must be a number >= 0 (+inf: unbounded)");
    A.ndirs = params ? params->ndirs : 0u;
    if (A.ndirs > CGRT_SDF_MAX_DIRS || (A.ndirs && A.ndirs % 2 == 0)) return fail(CGRT_E_ARG, "ndirs must be 0 or odd, 1..7");
    const float(*dirs)[3] = A.ndirs ? params->dirs : kSdfDefaultDirs;
    if (!A.ndirs) A.ndirs = CGRT_SDF_DEFAULT_NDIRS;
    for (uint32_t j = 0; j < A.ndirs; j++) {
        const float* d = dirs[j];
        if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2])) return fail(CGRT_E_ARG, "a direction has a non-finite component");
        if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) return fail(CGRT_E_ARG, "a direction is all zero");
        memcpy(A.dirs[j], d, 12);
    }
    if (device && ((uintptr_t)points % 4 || (uintptr_t)sdf % 4)) return fail(CGRT_E_ARG, "d_points and d_sdf must be 4-byte aligned");
    NEED_DEVICE(s);
    if (A.n == 0) return CGRT_OK;
    QueryCall c(s, device, stream);
    void *dp = nullptr, *ds = nullptr, *di = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, is_grid ? 0 : (uint64_t)A.n * 12, "d_points", &dp));
    A.points = static_cast<const float*>(dp);
    const bool brute = crossing_brute_scene(s);
    if (work) {
        A.want_sdf = want_sdf ? 1u : 0u;
        CGRT_TRY(c.zero_counters(5));
        HIP_TRY(launch_sdf(s->dev, A, SDF_LIST, brute, c.counters(), c.stream()));
        return c.read_counters(work, 5);
    }
    CGRT_TRY(c.out(1, sdf, sdf ? (uint64_t)A.n * 4 : 0, "d_sdf", &ds));
    CGRT_TRY(c.out(2, inside, inside ? A.n : 0, "d_inside", &di));
    A.want_sdf = sdf ? 1u : 0u;
    A.sdf = static_cast<float*>(ds);
    A.inside = static_cast<uint8_t*>(di);
    const SdfPoints how = !is_grid ? SDF_LIST : (g_sdf_grid_linear.load() ? SDF_GRID_LINEAR : SDF_GRID_BRICK);
    HIP_TRY(launch_sdf(s->dev, A, how, brute, nullptr, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_signed_distance(CgrtScene* s, const float* points, uint64_t n, const CgrtSdfParams* params, float* sdf, uint8_t* inside) {
    return sdf_query(s, false, points, nullptr, false, n, params, sdf, inside, 0, nullptr, nullptr);
}
int cgrt_signed_distance_device(CgrtScene* s, const float* d_points, uint64_t n, const CgrtSdfParams* params, float* d_sdf, uint8_t* d_inside,
                                void* stream) {
    return sdf_query(s, true, d_points, nullptr, false, n, params, d_sdf, d_inside, 0, nullptr, stream);
}
int cgrt_signed_distance_grid(CgrtScene* s, const CgrtGrid* grid, const CgrtSdfParams* params, float* sdf, uint8_t* inside) {
    return sdf_query(s, false, nullptr, grid, true, 0, params, sdf, inside, 0, nullptr, nullptr);
}
int cgrt_signed_distance_grid_device(CgrtScene* s, const CgrtGrid* grid, const CgrtSdfParams* params, float* d_sdf, uint8_t* d_inside,
                                     void* stream) {
    return sdf_query(s, true, nullptr, grid, true, 0, params, d_sdf, d_inside, 0, nullptr, stream);
}
int cgrt_debug_sdf_work(CgrtScene* s, const float* points, uint64_t n, const CgrtSdfParams* params, int want_sdf, uint64_t* out5) {
    return sdf_query(s, false, points, nullptr, false, n, params, nullptr, nullptr, want_sdf, out5, nullptr);
}
int cgrt_debug_set_sdf_grid_mapping(int linear) {
    if (linear != 0 && linear != 1) return fail(CGRT_E_ARG, "linear must be 0 or 1");
    g_sdf_grid_linear.store(linear);
    return CGRT_OK;
}

// ---- winding numbers (include/cgrt.h cgrt_winding_numbers*): the signed solid angles of the triangles over 4 pi,
// every triangle (brute) or far clusters of the tree of winding_builder.h replaced by their dipoles.  No frame state is read or written;
// the checks come in the order include/cgrt.h states, all before any device work.
namespace {
// the scene's cluster tree on the host, built by the first caller (later calls: one atomic load); works on a host-only scene
int winding_host_tree(CgrtScene* s) {
    if (s->winding_built.load(std::memory_order_acquire)) return CGRT_OK;
    std::lock_guard<std::mutex> lk(s->surface_mutex);
    if (s->winding_built.load(std::memory_order_acquire)) return CGRT_OK;
    if (s->bvh.tris.size() != s->ntris || s->ntris > SUB_MAX_RECORDS) return fail(CGRT_E_ARG, "the scene's records do not cover its triangles");
    try {
        build_winding_tree(s->bvh.tris.data(), s->ntris, s->winding);
    } catch (const std::bad_alloc&) {
        return fail(CGRT_E_ALLOC, "host allocation failed");
    }
    s->winding_built.store(true, std::memory_order_release);
    return CGRT_OK;
}
// ... and on the device, uploaded once (complete when this returns: every later launch on any stream sees it); fills A's tree fields
int winding_device_tree(CgrtScene* s, WindingArgs* A) {
    int rc = winding_host_tree(s);
    if (rc) return rc;
    const WindingTree& T = s->winding;
    void* p = s->d_winding.load(std::memory_order_acquire);
    if (!p && !T.clusters.empty()) {
        std::lock_guard<std::mutex> lk(s->surface_mutex);
        p = s->d_winding.load(std::memory_order_acquire);
        if (!p) {
            const size_t bytes = T.clusters.size() * sizeof(WindingCluster);
            void* d = nullptr;
            HIP_TRY(hipMalloc(&d, bytes));
            const hipError_t e = staged_h2d(d, T.clusters.data(), bytes);
            if (e != hipSuccess) {
                (void)hipFree(d);
                return hip_fail(e, "uploading the winding cluster tree");
            }
            s->device_bytes += bytes;
            s->d_winding.store(d, std::memory_order_release);
            p = d;
        }
    }
    A->clusters = static_cast<const WindingCluster*>(p);
    A->nlevels = T.nlevels();
    A->top_base = A->nlevels ? T.level_offsets[A->nlevels - 1] : 0u;
    return CGRT_OK;
}
// slots: 0 the points, 1 w, 2 inside; brute: every triangle, beta is not read; work: the counted launch (both host form only: out3 in
// the place of both outputs)
int winding_query(CgrtScene* s, bool device, const float* points, const CgrtGrid* grid, bool is_grid, uint64_t n, const CgrtWindingParams* params,
                  float* w, uint8_t* inside, bool brute, uint64_t* work, void* stream) {
    WindingArgs A{};
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    const int rc = point_source(points, grid, is_grid, n, w || inside || work, &A);
    if (rc) return rc == kNoResult ? fail(CGRT_E_ARG, "NULL argument: neither w nor inside is asked for") : rc;
    float beta = params ? params->beta : 0.0f;
    if (beta == 0.0f || brute) beta = CGRT_WINDING_DEFAULT_BETA;
    if (!(beta >= 1.0f)) return fail(CGRT_E_ARG, "beta must be a number >= 1 (0: the default; +inf: no cluster is far)");
    A.beta2 = beta * beta;  // rounded once, here
    A.threshold = params ? params->threshold : CGRT_WINDING_DEFAULT_THRESHOLD;
    if (device && ((uintptr_t)points % 4 || (uintptr_t)w % 4)) return fail(CGRT_E_ARG, "d_points and d_w must be 4-byte aligned");
    NEED_DEVICE(s);
    if (A.n == 0) return CGRT_OK;
    QueryCall c(s, device, stream);
    void *dp = nullptr, *dw = nullptr, *di = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, is_grid ? 0 : (uint64_t)A.n * 12, "d_points", &dp));
    if (!work) {
        CGRT_TRY(c.out(1, w, w ? (uint64_t)A.n * 4 : 0, "d_w", &dw));
        CGRT_TRY(c.out(2, inside, inside ? A.n : 0, "d_inside", &di));
    }
    A.points = static_cast<const float*>(dp);
    A.w = static_cast<float*>(dw);
    A.inside = static_cast<uint8_t*>(di);
    A.recs = s->dev.tris + s->dev.tri_base;
    A.ntris = s->dev.ntris;
    if (!brute) CGRT_TRY(winding_device_tree(s, &A));
    if (work) {
        CGRT_TRY(c.zero_counters(3));
        HIP_TRY(launch_winding(A, WINDING_LIST, false, c.counters(), c.stream()));
        return c.read_counters(work, 3);
    }
    HIP_TRY(launch_winding(A, is_grid ? WINDING_GRID_BRICK : WINDING_LIST, brute, nullptr, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_winding_numbers(CgrtScene* s, const float* points, uint64_t n, const CgrtWindingParams* params, float* w, uint8_t* inside) {
    return winding_query(s, false, points, nullptr, false, n, params, w, inside, false, nullptr, nullptr);
}
int cgrt_winding_numbers_device(CgrtScene* s, const float* d_points, uint64_t n, const CgrtWindingParams* params, float* d_w, uint8_t* d_inside,
                                void* stream) {
    return winding_query(s, true, d_points, nullptr, false, n, params, d_w, d_inside, false, nullptr, stream);
}
int cgrt_winding_numbers_grid(CgrtScene* s, const CgrtGrid* grid, const CgrtWindingParams* params, float* w, uint8_t* inside) {
    return winding_query(s, false, nullptr, grid, true, 0, params, w, inside, false, nullptr, nullptr);
}
int cgrt_winding_numbers_grid_device(CgrtScene* s, const CgrtGrid* grid, const CgrtWindingParams* params, float* d_w, uint8_t* d_inside,
                                     void* stream) {
    return winding_query(s, true, nullptr, grid, true, 0, params, d_w, d_inside, false, nullptr, stream);
}
int cgrt_winding_numbers_brute(CgrtScene* s, const float* points, uint64_t n, const CgrtWindingParams* params, float* w, uint8_t* inside) {
    return winding_query(s, false, points, nullptr, false, n, params, w, inside, true, nullptr, nullptr);
}
int cgrt_debug_winding_work(CgrtScene* s, const float* points, uint64_t n, const CgrtWindingParams* params, uint64_t* out3) {
    return winding_query(s, false, points, nullptr, false, n, params, nullptr, nullptr, false, out3, nullptr);
}
int cgrt_debug_get_winding_tree(CgrtScene* s, float* clusters, uint32_t* level_offsets, uint32_t* nlevels, uint32_t* record_prims) {
    if (!s || !nlevels) return fail(CGRT_E_ARG, "NULL argument");
    const int rc = winding_host_tree(s);
    if (rc) return rc;
    const WindingTree& T = s->winding;
    *nlevels = T.nlevels();
    if (level_offsets) {
        if (T.level_offsets.empty())
            level_offsets[0] = 0;
        else
            memcpy(level_offsets, T.level_offsets.data(), T.level_offsets.size() * sizeof(uint32_t));
    }
    if (clusters && !T.clusters.empty()) memcpy(clusters, T.clusters.data(), T.clusters.size() * sizeof(WindingCluster));
    if (record_prims)
        for (size_t k = 0; k < s->bvh.tris.size(); k++) record_prims[k] = s->bvh.tris[k].prim_id;
    return CGRT_OK;
}

// ---- surface sampling (include/cgrt.h cgrt_sample_surface*): area-weighted points on the triangles, sample j a
// function of (scene, seed, j, strata) alone.  No frame state is read or written; the checks come in the order include/cgrt.h states, all
// before any device work.
namespace {
static_assert(sizeof(CgrtSurfaceSample) == sizeof(CgrtSurfaceSampleDev), "CgrtSurfaceSample is what the kernel writes");
// the scene's areas and thresholds on the host, built by the first caller (later calls: one atomic load); works on a host-only scene
int sample_host_table(CgrtScene* s) {
    if (s->sampling_built.load(std::memory_order_acquire)) return CGRT_OK;
    std::lock_guard<std::mutex> lk(s->surface_mutex);
    if (s->sampling_built.load(std::memory_order_acquire)) return CGRT_OK;
    if (s->bvh.tris.size() != s->ntris) return fail(CGRT_E_ARG, "the scene's records do not cover its triangles");
    try {
        if (!build_sample_table(s->bvh.tris.data(), s->ntris, s->sampling)) return fail(CGRT_E_ARG, "a triangle record carries a primitive id out of range");
    } catch (const std::bad_alloc&) {
        return fail(CGRT_E_ALLOC, "host allocation failed");
    }
    s->sampling_built.store(true, std::memory_order_release);
    return CGRT_OK;
}
// ... and the thresholds on the device, uploaded once (complete when this returns: every later launch on any stream sees them); fills
// A's table fields.  A scene that is empty for sampling uploads nothing.
int sample_device_table(CgrtScene* s, SampleArgs* A) {
    CGRT_TRY(sample_host_table(s));
    const SampleTable& T = s->sampling;
    A->last = T.last;
    A->steps = 0;
    A->thresholds = nullptr;
    if (T.last == SAMPLE_NO_PRIM) return CGRT_OK;
    while (A->steps < 32u && (1ull << A->steps) < (uint64_t)T.last + 1ull) A->steps++;  // ceil(log2(last + 1))
    void* p = s->d_sampling.load(std::memory_order_acquire);
    if (!p) {
        std::lock_guard<std::mutex> lk(s->surface_mutex);
        p = s->d_sampling.load(std::memory_order_acquire);
        if (!p) {
            const size_t bytes = T.thresholds.size() * sizeof(uint32_t);
            void* d = nullptr;
            HIP_TRY(hipMalloc(&d, bytes));
            const hipError_t e = staged_h2d(d, T.thresholds.data(), bytes);
            if (e != hipSuccess) {
                (void)hipFree(d);
                return hip_fail(e, "uploading the sampling thresholds");
            }
            s->device_bytes += bytes;
            s->d_sampling.store(d, std::memory_order_release);
            p = d;
        }
    }
    A->thresholds = static_cast<const uint32_t*>(p);
    return CGRT_OK;
}
// slots: 0 out, 1 attr, 2 out_attr
int sample_query(CgrtScene* s, bool device, uint64_t n, const CgrtSampleParams* params, CgrtSurfaceSample* out, const float* attr,
                 uint32_t channels, float* out_attr, void* stream) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    if (n && !out) return fail(CGRT_E_ARG, "NULL argument");
    if ((attr != nullptr) != (out_attr != nullptr)) return fail(CGRT_E_ARG, "attr and out_attr must be given together");
    if (n > 0x7fffffffull) return fail(CGRT_E_ARG, "too many samples: n exceeds 0x7fffffff");
    if (attr) CGRT_TRY(surface_channels(channels, n));
    const CgrtSampleParams P = params ? *params : CgrtSampleParams{0, 0, 0};
    if (P.strata > 0xffffffffull) return fail(CGRT_E_ARG, "strata exceeds 0xffffffff");
    if (P.strata && (P.first > P.strata || n > P.strata - P.first)) return fail(CGRT_E_ARG, "first + n exceeds strata");
    if (P.first + n < P.first) return fail(CGRT_E_ARG, "first + n overflows 64 bits");
    if (device && ((uintptr_t)out % 4 || (uintptr_t)attr % 4 || (uintptr_t)out_attr % 4))
        return fail(CGRT_E_ARG, "device pointers must be 4-byte aligned");
    NEED_DEVICE(s);
    if (n == 0) return CGRT_OK;
    QueryCall c(s, device, stream);
    void *dout = nullptr, *dattr = nullptr, *drows = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.out(0, out, n * sizeof(CgrtSurfaceSample), "d_out", &dout));
    CGRT_TRY(c.in(1, attr, attr ? (uint64_t)s->nverts * channels * 4ull : 0, "d_attr", &dattr));
    CGRT_TRY(c.out(2, out_attr, attr ? n * channels * 4ull : 0, "d_out_attr", &drows));
    SampleArgs A{};
    CGRT_TRY(sample_device_table(s, &A));
    const SurfaceLookup* lookup = nullptr;
    if (A.last != SAMPLE_NO_PRIM) CGRT_TRY(surface_lookup(s, &lookup));
    A.tris = s->dev.tris;
    A.lookup = lookup;
    A.n = (uint32_t)n;
    A.seed = P.seed;
    A.first = P.first;
    A.strata = P.strata;
    A.out = static_cast<CgrtSurfaceSampleDev*>(dout);
    A.attr = attr ? static_cast<const float*>(dattr) : nullptr;
    A.channels = attr ? channels : 0;
    A.out_attr = attr ? static_cast<float*>(drows) : nullptr;
    A.vec4 = attr && channels % 4 == 0 && (uintptr_t)dattr % 16 == 0 && (uintptr_t)drows % 16 == 0;
    HIP_TRY(launch_sample_surface(A, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_sample_surface(CgrtScene* s, uint64_t n, const CgrtSampleParams* params, CgrtSurfaceSample* out, const float* attr, uint32_t channels,
                        float* out_attr) {
    return sample_query(s, false, n, params, out, attr, channels, out_attr, nullptr);
}
int cgrt_sample_surface_device(CgrtScene* s, uint64_t n, const CgrtSampleParams* params, CgrtSurfaceSample* d_out, const float* d_attr,
                               uint32_t channels, float* d_out_attr, void* stream) {
    return sample_query(s, true, n, params, d_out, d_attr, channels, d_out_attr, stream);
}
int cgrt_triangle_areas(CgrtScene* s, float* areas, double* total) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    CGRT_TRY(sample_host_table(s));
    const SampleTable& T = s->sampling;
    if (areas && !T.areas.empty()) memcpy(areas, T.areas.data(), T.areas.size() * sizeof(float));
    if (total) *total = T.total;
    return CGRT_OK;
}
int cgrt_debug_get_sample_table(CgrtScene* s, uint32_t* thresholds, uint32_t* last) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    CGRT_TRY(sample_host_table(s));
    const SampleTable& T = s->sampling;
    if (thresholds && !T.thresholds.empty()) memcpy(thresholds, T.thresholds.data(), T.thresholds.size() * sizeof(uint32_t));
    if (last) *last = T.last;
    return CGRT_OK;
}

// ---- Poisson-disk sets (include/cgrt.h cgrt_poisson_disk*): the points of a list that keep a minimum spacing, the
// first maximal independent set in a seeded (or the caller's) order.  The scene only names the device and lends the call lane; no frame
// state is read or written; the checks come in the order include/cgrt.h states, all before any device work.
namespace {
// the device form's workspace as the caller gave it
struct PoissonWorkspace {
    void* d;
    uint64_t bytes;
};
// slots: 0 the points, 1 the flags, 2 the priorities, 3 the workspace (host form: the lane's) and the pinned header both forms read back.
// how: 0 hashed grid, 1 brute force, 2 counted grid (both host form only; 2: `work` in the place of keep and kept)
int poisson_query(CgrtScene* s, bool device, const float* points, uint64_t n, const CgrtPoissonParams* params, uint8_t* keep, uint64_t* kept,
                  const PoissonWorkspace* ws, int how, uint64_t* work, void* stream) {
    if (!s || !params) return fail(CGRT_E_ARG, "scene or params is NULL");
    if (n && (!points || (how == 2 ? !work : !keep))) return fail(CGRT_E_ARG, "NULL argument");
    if (n > 0x7fffffffull) return fail(CGRT_E_ARG, "too many points: n exceeds 0x7fffffff");
    if (params->min_dist2 == INFINITY) return fail(CGRT_E_ARG, "min_dist2 must not be +inf");
    if (device && ((uintptr_t)points % 4 || (uintptr_t)params->priority % 4)) return fail(CGRT_E_ARG, "device pointers must be 4-byte aligned");
    if (ws && n) {
        if (!ws->d) return fail(CGRT_E_ARG, "NULL argument");
        if ((uintptr_t)ws->d % 8) return fail(CGRT_E_ARG, "d_workspace must be 8-byte aligned");
        if (ws->bytes < poisson_workspace_bytes(n)) return fail(CGRT_E_ARG, "workspace_bytes is below cgrt_poisson_disk_workspace");
    }
    NEED_DEVICE(s);
    if (n == 0) {
        if (kept) *kept = 0;
        if (work) memset(work, 0, 6 * sizeof(uint64_t));
        return CGRT_OK;
    }
    QueryCall c(s, device, stream);
    void *dp = nullptr, *dk = nullptr, *dprio = nullptr, *dws = nullptr, *pin = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, n * 12, "d_points", &dp));
    CGRT_TRY(c.out(1, keep, how == 2 ? 0 : n, "d_keep", &dk));
    CGRT_TRY(c.in(2, params->priority, params->priority ? n * 4 : 0, "d_priority", &dprio));
    if (ws) {
        dws = ws->d;
        CGRT_TRY(check_device_span(s, dws, poisson_workspace_bytes(n), "d_workspace"));
    } else {
        HIP_TRY(c.c.scratch(3, poisson_workspace_bytes(n), &dws));
        if (how == 2) HIP_TRY(c.c.scratch(1, n, &dk));
    }
    if (device) CGRT_TRY(c.c.g.acquire());  // (a lane for its pinned words only: the work runs on the caller's stream)
    HIP_TRY(c.c.g.pin(3, 64, &pin));
    PoissonCall Q{};
    Q.points = static_cast<const float*>(dp);
    Q.n = (uint32_t)n;
    Q.min_dist2 = params->min_dist2;
    Q.seed = params->seed;
    Q.priority = params->priority ? static_cast<const uint32_t*>(dprio) : nullptr;
    Q.keep = static_cast<uint8_t*>(dk);
    Q.workspace = dws;
    PoissonWork W{};
    HIP_TRY(run_poisson_disk(Q, how == 1, static_cast<uint32_t*>(pin), c.stream(), kept, how == 2 ? &W : nullptr));
    if (how == 2) {
        const uint64_t out6[6] = {W.rounds, W.pair_tests, W.buckets_used, W.buckets, W.build_ns, W.rounds_ns};
        memcpy(work, out6, sizeof(out6));
        return CGRT_OK;
    }
    return c.finish();
}
}  // namespace

int cgrt_poisson_disk(CgrtScene* s, const float* points, uint64_t n, const CgrtPoissonParams* params, uint8_t* keep, uint64_t* kept) {
    return poisson_query(s, false, points, n, params, keep, kept, nullptr, 0, nullptr, nullptr);
}
int cgrt_poisson_disk_device(CgrtScene* s, const float* d_points, uint64_t n, const CgrtPoissonParams* params, uint8_t* d_keep, uint64_t* kept,
                             void* d_workspace, uint64_t workspace_bytes, void* stream) {
    const PoissonWorkspace ws{d_workspace, workspace_bytes};
    return poisson_query(s, true, d_points, n, params, d_keep, kept, &ws, 0, nullptr, stream);
}
int cgrt_poisson_disk_workspace(CgrtScene* s, uint64_t n, uint64_t* bytes) {
    if (!s || !bytes) return fail(CGRT_E_ARG, "NULL argument");
    if (n > 0x7fffffffull) return fail(CGRT_E_ARG, "too many points: n exceeds 0x7fffffff");
    *bytes = poisson_workspace_bytes(n);
    return CGRT_OK;
}
int cgrt_poisson_disk_brute(CgrtScene* s, const float* points, uint64_t n, const CgrtPoissonParams* params, uint8_t* keep, uint64_t* kept) {
    return poisson_query(s, false, points, n, params, keep, kept, nullptr, 1, nullptr, nullptr);
}
int cgrt_debug_poisson_work(CgrtScene* s, const float* points, uint64_t n, const CgrtPoissonParams* params, uint64_t* out6) {
    return poisson_query(s, false, points, n, params, nullptr, nullptr, nullptr, 2, out6, nullptr);
}

// ---- point-set neighbours (include/cgrt.h cgrt_point_grid_*, cgrt_count_point_neighbors*, cgrt_list_point_neighbors*; DESIGN.md section
// 5.30): every point of a cloud within a query point's squared radius, counted or listed in (d2, index) order, over a hashed grid that
// lives in the caller's device memory.  The scene only names the device and lends the call lane; no frame state is read or written; the
// checks come in the order include/cgrt.h states, all before any device work.
namespace {
static_assert(sizeof(CgrtPointNeighbor) == sizeof(CgrtPointNeighborDev), "CgrtPointNeighbor is what the kernels write");
const uint64_t kMaxCloud = 0x7fffffffull;
// the cloud of a call: the built grid (device forms), or the points themselves (host forms, which build a grid of their own or none)
struct PointCloud {
    const float* data;
    uint64_t m;
    float cell;
    const void* d_grid;
    uint64_t grid_bytes;
};
// a host form's own device memory, returned when the call ends (declared before the QueryCall: the lane has been waited for by then)
struct OwnedDevice {
    void* p = nullptr;
    ~OwnedDevice() {
        if (p) (void)hipFree(p);
    }
};
bool cell_ok(float cell) { return cell > 0.0f && cell <= 3.402823466e+38f; }
// slots: 0 the points, 4 the radii, then the list's; how: 0 the grid, 1 brute force, 2 the counted grid search (1 and 2 host form only;
// 2: `work`, L is k records per query of the lane's own, or with k == 0 the count search)
int point_neighbor_query(CgrtScene* s, bool device, const PointCloud& G, const float* points, uint64_t n, const CgrtPointQuery* q,
                         const SlotList& L, int how, uint64_t* work, void* stream) {
    const void* const result = how == 2 ? static_cast<const void*>(work) : (L.list ? L.out : static_cast<const void*>(L.counts));
    if (!s || !q) return fail(CGRT_E_ARG, "scene or query is NULL");
    if (n && (!points || !result || (device ? !G.d_grid : (G.m && !G.data)))) return fail(CGRT_E_ARG, "NULL argument");
    if (n > kMaxCloud) return fail(CGRT_E_ARG, "too many queries: n exceeds 0x7fffffff");
    if (!device && G.m > kMaxCloud) return fail(CGRT_E_ARG, "too many data points: m exceeds 0x7fffffff");
    if (!device && how != 1 && !cell_ok(G.cell)) return fail(CGRT_E_ARG, "cell must be finite and > 0");
    if (!(q->max_dist2 >= 0.0f)) return fail(CGRT_E_ARG, "max_dist2 must be a number >= 0 (+inf: unbounded)");
    if (q->flags & ~(uint32_t)CGRT_POINTS_SKIP_SAME_INDEX) return fail(CGRT_E_ARG, "unknown flags");
    CGRT_TRY(L.rules(n, device));
    if (device && ((uintptr_t)points % 4 || (uintptr_t)q->radius2 % 4 || !L.aligned() || (uintptr_t)G.d_grid % 8))
        return fail(CGRT_E_ARG, "device pointers must be aligned to their elements (d_grid: 8 bytes)");
    if (device && n && G.grid_bytes < point_grid_bytes(0)) return fail(CGRT_E_ARG, "grid_bytes is below cgrt_point_grid_workspace");
    NEED_DEVICE(s);
    if (n == 0 || L.nothing(n, device)) return CGRT_OK;
    OwnedDevice own;
    QueryCall c(s, device, stream);
    void *dp = nullptr, *drad = nullptr;
    PointNeighborArgs A{};
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, n * 12, "d_points", &dp));
    CGRT_TRY(c.in(4, q->radius2, q->radius2 ? n * 4 : 0, "d_radius2", &drad));
    CGRT_TRY(L.transfer(c, n, &A));
    if (device) {
        CGRT_TRY(check_device_span(s, G.d_grid, G.grid_bytes, "d_grid"));
        A.grid = G.d_grid;
        A.grid_bytes = G.grid_bytes;
    } else {  // the grid (none: brute force), then the cloud
        const uint64_t gbytes = how == 1 ? 0 : point_grid_bytes(G.m);
        HIP_TRY(hipMalloc(&own.p, gbytes + 12 * G.m + 16));
        float* const ddata = reinterpret_cast<float*>(static_cast<char*>(own.p) + gbytes);
        if (G.m) HIP_TRY(staged_h2d(ddata, G.data, 12 * G.m));  // (complete when it returns)
        if (how != 1) HIP_TRY(launch_point_grid_build(ddata, G.m, G.cell, own.p, c.stream()));
        A.grid = own.p;
        A.grid_bytes = gbytes;
        A.data = ddata;
        A.m = G.m;
    }
    A.points = static_cast<const float*>(dp);
    A.radius2 = static_cast<const float*>(drad);
    A.max_dist2 = q->max_dist2;
    A.flags = q->flags;
    A.n = n;
    if (how == 2) {
        CGRT_TRY(c.zero_counters(6));
        HIP_TRY(launch_point_neighbors(A, false, c.counters(), c.stream()));
        return c.read_counters(work, 6);
    }
    HIP_TRY(launch_point_neighbors(A, how == 1, nullptr, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_point_grid_workspace(CgrtScene* s, uint64_t m, uint64_t* bytes) {
    if (!s || !bytes) return fail(CGRT_E_ARG, "NULL argument");
    if (m > kMaxCloud) return fail(CGRT_E_ARG, "too many data points: m exceeds 0x7fffffff");
    *bytes = point_grid_bytes(m);
    return CGRT_OK;
}
int cgrt_point_grid_build_device(CgrtScene* s, const float* d_data, uint64_t m, float cell, void* d_grid, uint64_t grid_bytes, void* stream) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    if ((m && !d_data) || !d_grid) return fail(CGRT_E_ARG, "NULL argument");
    if (m > kMaxCloud) return fail(CGRT_E_ARG, "too many data points: m exceeds 0x7fffffff");
    if (!cell_ok(cell)) return fail(CGRT_E_ARG, "cell must be finite and > 0");
    if ((uintptr_t)d_data % 4 || (uintptr_t)d_grid % 8) return fail(CGRT_E_ARG, "d_data must be 4-byte and d_grid 8-byte aligned");
    if (grid_bytes < point_grid_bytes(m)) return fail(CGRT_E_ARG, "grid_bytes is below cgrt_point_grid_workspace");
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    CGRT_TRY(check_device_span(s, d_data, m * 12, "d_data"));
    CGRT_TRY(check_device_span(s, d_grid, point_grid_bytes(m), "d_grid"));
    HIP_TRY(launch_point_grid_build(d_data, m, cell, d_grid, static_cast<hipStream_t>(stream)));
    return CGRT_OK;
}
int cgrt_count_point_neighbors_device(CgrtScene* s, const void* d_grid, uint64_t grid_bytes, const float* d_points, uint64_t n,
                                      const CgrtPointQuery* query, uint32_t* d_counts, void* stream) {
    return point_neighbor_query(s, true, {nullptr, 0, 0.0f, d_grid, grid_bytes}, d_points, n, query, {false, nullptr, 0, nullptr, 0, d_counts}, 0,
                                nullptr, stream);
}
int cgrt_list_point_neighbors_device(CgrtScene* s, const void* d_grid, uint64_t grid_bytes, const float* d_points, uint64_t n,
                                     const CgrtPointQuery* query, const uint64_t* d_offsets, uint32_t k, CgrtPointNeighbor* d_out,
                                     uint64_t capacity, uint32_t* d_counts, void* stream) {
    return point_neighbor_query(s, true, {nullptr, 0, 0.0f, d_grid, grid_bytes}, d_points, n, query, {true, d_offsets, k, d_out, capacity, d_counts},
                                0, nullptr, stream);
}
int cgrt_count_point_neighbors(CgrtScene* s, const float* data, uint64_t m, float cell, const float* points, uint64_t n,
                               const CgrtPointQuery* query, uint32_t* counts) {
    return point_neighbor_query(s, false, {data, m, cell, nullptr, 0}, points, n, query, {false, nullptr, 0, nullptr, 0, counts}, 0, nullptr, nullptr);
}
int cgrt_list_point_neighbors(CgrtScene* s, const float* data, uint64_t m, float cell, const float* points, uint64_t n, const CgrtPointQuery* query,
                              const uint64_t* offsets, uint32_t k, CgrtPointNeighbor* out, uint64_t capacity, uint32_t* counts) {
    return point_neighbor_query(s, false, {data, m, cell, nullptr, 0}, points, n, query, {true, offsets, k, out, capacity, counts}, 0, nullptr,
                                nullptr);
}
int cgrt_list_point_neighbors_brute(CgrtScene* s, const float* data, uint64_t m, const float* points, uint64_t n, const CgrtPointQuery* query,
                                    const uint64_t* offsets, uint32_t k, CgrtPointNeighbor* out, uint64_t capacity, uint32_t* counts) {
    return point_neighbor_query(s, false, {data, m, 0.0f, nullptr, 0}, points, n, query, {true, offsets, k, out, capacity, counts}, 1, nullptr,
                                nullptr);
}
int cgrt_debug_point_neighbor_work(CgrtScene* s, const float* data, uint64_t m, float cell, const float* points, uint64_t n,
                                   const CgrtPointQuery* query, uint32_t k, uint64_t* out6) {
    // (n <= 0x7fffffff is checked before the capacity n k is looked at)
    return point_neighbor_query(s, false, {data, m, cell, nullptr, 0}, points, n, query, {k > 0, nullptr, k, nullptr, n * (uint64_t)k, nullptr}, 2,
                                out6, nullptr);
}

// ---- point-set frames (include/cgrt.h cgrt_point_frames*): centroid, covariance eigenvalues and a right-handed
// frame of every query's k nearest data points within its squared radius, search and solve in one kernel.  The checks are the point-set
// neighbour entries' in their order, with k, n * k and the frames' alignment added; all before any device work.
namespace {
static_assert(sizeof(CgrtPointFrame) == sizeof(CgrtPointFrameDev), "CgrtPointFrame is what the kernel writes");
// slots: 0 the points, 4 the radii, 1 the orientation vectors, 2 the neighbour records (the lane's own where the caller wants none), 3 the
// frames; how: 0 the grid, 1 brute force (host form only)
int point_frame_query(CgrtScene* s, bool device, const PointCloud& G, const float* points, uint64_t n, const CgrtPointQuery* q, uint32_t k,
                      const float* orient, CgrtPointNeighbor* neighbors, CgrtPointFrame* frames, int how, void* stream) {
    if (!s || !q) return fail(CGRT_E_ARG, "scene or query is NULL");
    if (n && (!points || !frames || (device && !neighbors) || (G.m && !G.data) || (device && !G.d_grid))) return fail(CGRT_E_ARG, "NULL argument");
    if (n > kMaxCloud) return fail(CGRT_E_ARG, "too many queries: n exceeds 0x7fffffff");
    if (G.m > kMaxCloud) return fail(CGRT_E_ARG, "too many data points: m exceeds 0x7fffffff");
    if (!device && how != 1 && !cell_ok(G.cell)) return fail(CGRT_E_ARG, "cell must be finite and > 0");
    if (!(q->max_dist2 >= 0.0f)) return fail(CGRT_E_ARG, "max_dist2 must be a number >= 0 (+inf: unbounded)");
    if (q->flags & ~(uint32_t)CGRT_POINTS_SKIP_SAME_INDEX) return fail(CGRT_E_ARG, "unknown flags");
    if (k == 0) return fail(CGRT_E_ARG, "k must be at least 1");
    if (n * (uint64_t)k > kSlotMaxCapacity) return fail(CGRT_E_ARG, "n * k exceeds 2^37 records");
    if (device && ((uintptr_t)points % 4 || (uintptr_t)q->radius2 % 4 || (uintptr_t)G.data % 4 || (uintptr_t)orient % 4 ||
                   (uintptr_t)neighbors % 4 || (uintptr_t)G.d_grid % 8))
        return fail(CGRT_E_ARG, "device pointers must be aligned to their elements (d_grid: 8 bytes)");
    if (device && (uintptr_t)frames % 16) return fail(CGRT_E_ARG, "d_frames must be 16-byte aligned");
    if (device && n && G.grid_bytes < point_grid_bytes(0)) return fail(CGRT_E_ARG, "grid_bytes is below cgrt_point_grid_workspace");
    NEED_DEVICE(s);
    if (n == 0) return CGRT_OK;
    OwnedDevice own;
    QueryCall c(s, device, stream);
    void *dp = nullptr, *drad = nullptr, *dorient = nullptr, *dnb = nullptr, *dfr = nullptr;
    PointFrameArgs A{};
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, n * 12, "d_points", &dp));
    CGRT_TRY(c.in(4, q->radius2, q->radius2 ? n * 4 : 0, "d_radius2", &drad));
    CGRT_TRY(c.in(1, orient, orient ? n * 12 : 0, "d_orient", &dorient));
    if (device || neighbors)
        CGRT_TRY(c.out(2, neighbors, n * k * sizeof(CgrtPointNeighbor), "d_neighbors", &dnb));
    else
        HIP_TRY(c.c.scratch(2, n * k * sizeof(CgrtPointNeighbor), &dnb));  // (the kernel's slots; nothing comes back)
    CGRT_TRY(c.out(3, frames, n * sizeof(CgrtPointFrame), "d_frames", &dfr));
    if (device) {
        CGRT_TRY(check_device_span(s, G.d_grid, G.grid_bytes, "d_grid"));
        CGRT_TRY(check_device_span(s, G.data, G.m * 12, "d_data"));
        A.grid = G.d_grid;
        A.grid_bytes = G.grid_bytes;
        A.data = G.data;
    } else {  // the grid (none: brute force), then the cloud
        const uint64_t gbytes = how == 1 ? 0 : point_grid_bytes(G.m);
        HIP_TRY(hipMalloc(&own.p, gbytes + 12 * G.m + 16));
        float* const ddata = reinterpret_cast<float*>(static_cast<char*>(own.p) + gbytes);
        if (G.m) HIP_TRY(staged_h2d(ddata, G.data, 12 * G.m));  // (complete when it returns)
        if (how != 1) HIP_TRY(launch_point_grid_build(ddata, G.m, G.cell, own.p, c.stream()));
        A.grid = own.p;
        A.grid_bytes = gbytes;
        A.data = ddata;
    }
    A.m = G.m;
    A.points = static_cast<const float*>(dp);
    A.radius2 = static_cast<const float*>(drad);
    A.max_dist2 = q->max_dist2;
    A.flags = q->flags;
    A.n = n;
    A.k = k;
    A.orient = orient ? static_cast<const float*>(dorient) : nullptr;
    A.neighbors = static_cast<CgrtPointNeighborDev*>(dnb);
    A.frames = static_cast<CgrtPointFrameDev*>(dfr);
    HIP_TRY(launch_point_frames(A, how == 1, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_point_frames_device(CgrtScene* s, const void* d_grid, uint64_t grid_bytes, const float* d_data, uint64_t m, const float* d_points,
                             uint64_t n, const CgrtPointQuery* query, uint32_t k, const float* d_orient, CgrtPointNeighbor* d_neighbors,
                             CgrtPointFrame* d_frames, void* stream) {
    return point_frame_query(s, true, {d_data, m, 0.0f, d_grid, grid_bytes}, d_points, n, query, k, d_orient, d_neighbors, d_frames, 0, stream);
}
int cgrt_point_frames(CgrtScene* s, const float* data, uint64_t m, float cell, const float* points, uint64_t n, const CgrtPointQuery* query,
                      uint32_t k, const float* orient, CgrtPointNeighbor* neighbors, CgrtPointFrame* frames) {
    return point_frame_query(s, false, {data, m, cell, nullptr, 0}, points, n, query, k, orient, neighbors, frames, 0, nullptr);
}
int cgrt_point_frames_brute(CgrtScene* s, const float* data, uint64_t m, const float* points, uint64_t n, const CgrtPointQuery* query, uint32_t k,
                            const float* orient, CgrtPointNeighbor* neighbors, CgrtPointFrame* frames) {
    return point_frame_query(s, false, {data, m, 0.0f, nullptr, 0}, points, n, query, k, orient, neighbors, frames, 1, nullptr);
}

// ---- iso-surfaces (include/cgrt.h cgrt_isosurface*): the triangle mesh of one level of a scalar grid, by marching
// tetrahedra, in a defined order.  The scene only names the device and lends the call lane; no frame state is read or written; the checks
// come in the order include/cgrt.h states, all before any device work.
namespace {
struct IsoWorkspace {
    void* d;
    uint64_t bytes;
};
// the output of a list entry (count entries: list false, the rest unused)
struct IsoMesh {
    bool list;
    float* verts;
    uint64_t vert_capacity;
    uint32_t* tris;
    uint64_t tri_capacity;
};
int iso_grid(const CgrtGrid* grid, uint64_t* points) {
    uint64_t n = 1;
    for (int c = 0; c < 3; c++) {
        if (grid->dims[c] < 1 || grid->dims[c] > (1u << 24)) return fail(CGRT_E_ARG, "grid dims must be in 1..2^24");
        n *= grid->dims[c];  // (below 2^52 before the test, which follows every factor)
        if (n > kIsoMaxPoints) return fail(CGRT_E_ARG, "too many grid points: nx * ny * nz exceeds 2^28");
        if (!std::isfinite(grid->origin[c]) || !std::isfinite(grid->spacing[c])) return fail(CGRT_E_ARG, "grid origin and spacing must be finite");
    }
    *points = n;
    return CGRT_OK;
}
// slots: 0 the values, 1 the vertices, 2 the triangles, 3 the two counts, 4 the workspace (host form: the lane's).  work: the counted
// classify pass (host form only: out4 in the place of counts2)
int iso_query(CgrtScene* s, bool device, const CgrtGrid* grid, const float* values, const CgrtIsoParams* params, const IsoMesh& M,
              uint64_t* counts2, const IsoWorkspace* ws, bool counted, uint64_t* work, void* stream) {
    if (!s || !grid || !params) return fail(CGRT_E_ARG, "scene, grid or params is NULL");
    uint64_t N = 0;
    CGRT_TRY(iso_grid(grid, &N));
    if (!std::isfinite(params->iso)) return fail(CGRT_E_ARG, "iso must be finite");
    if (params->flags & ~(uint32_t)CGRT_ISO_INSIDE_ABOVE) return fail(CGRT_E_ARG, "unknown flags");
    if (!values) return fail(CGRT_E_ARG, "NULL argument: values");
    if (counted ? !work : !counts2) return fail(CGRT_E_ARG, counted ? "NULL argument: out4" : "NULL argument: counts2");
    if (M.list && ((M.vert_capacity && !M.verts) || (M.tri_capacity && !M.tris))) return fail(CGRT_E_ARG, "NULL output with a non-zero capacity");
    if (device && ((uintptr_t)values % 4 || (uintptr_t)M.verts % 4 || (uintptr_t)M.tris % 4 || (uintptr_t)counts2 % 8))
        return fail(CGRT_E_ARG, "device pointers must be aligned to their elements (d_counts2: 8 bytes)");
    if (ws) {
        if (!ws->d) return fail(CGRT_E_ARG, "NULL argument: d_workspace");
        if ((uintptr_t)ws->d % 8) return fail(CGRT_E_ARG, "d_workspace must be 8-byte aligned");
        if (ws->bytes < iso_workspace_bytes(N)) return fail(CGRT_E_ARG, "workspace_bytes is below cgrt_isosurface_workspace");
    }
    NEED_DEVICE(s);
    QueryCall c(s, device, stream);
    void *dv = nullptr, *dverts = nullptr, *dtris = nullptr, *dcounts = nullptr, *dws = nullptr;
    IsoCall Q{};
    memcpy(Q.origin, grid->origin, 12);
    memcpy(Q.spacing, grid->spacing, 12);
    memcpy(Q.dims, grid->dims, 12);
    Q.iso = params->iso;
    Q.above = (params->flags & CGRT_ISO_INSIDE_ABOVE) ? 1u : 0u;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, values, N * 4, "d_values", &dv));
    Q.values = static_cast<const float*>(dv);
    if (device) {  // in place on the caller's stream: no slot holds more than the grid can give
        const uint64_t vmax = std::min<uint64_t>(M.vert_capacity, 7 * N), tmax = std::min<uint64_t>(M.tri_capacity, 12 * N);
        CGRT_TRY(c.out(1, M.verts, M.list ? vmax * 12 : 0, "d_verts", &dverts));
        CGRT_TRY(c.out(2, M.tris, M.list ? tmax * 12 : 0, "d_tris", &dtris));
        CGRT_TRY(c.out(3, counts2, 16, "d_counts2", &dcounts));
        CGRT_TRY(check_device_span(s, ws->d, iso_workspace_bytes(N), "d_workspace"));
        Q.list = M.list;
        Q.verts = static_cast<float*>(dverts);
        Q.vert_capacity = M.vert_capacity;
        Q.tris = static_cast<uint32_t*>(dtris);
        Q.tri_capacity = M.tri_capacity;
        Q.counts2 = static_cast<unsigned long long*>(dcounts);
        Q.workspace = ws->d;
        HIP_TRY(launch_isosurface(Q, nullptr, c.stream()));
        return c.finish();
    }
    HIP_TRY(c.c.scratch(4, iso_workspace_bytes(N), &dws));
    Q.workspace = dws;
    if (counted) {
        CGRT_TRY(c.zero_counters(4));
        Q.counts2 = c.counters() + 2;
        HIP_TRY(launch_isosurface(Q, c.counters(), c.stream()));
        return c.read_counters(work, 4);
    }
    // the count, read back; then the list into buffers no larger than what will be written (a caller may over-allocate freely), so that
    // nothing beyond the written records reaches the caller's arrays
    HIP_TRY(c.c.scratch(3, 16, &dcounts));
    Q.counts2 = static_cast<unsigned long long*>(dcounts);
    HIP_TRY(launch_isosurface(Q, nullptr, c.stream()));
    unsigned long long h[2];
    HIP_TRY(hipMemcpyAsync(h, dcounts, 16, hipMemcpyDeviceToHost, c.stream()));
    HIP_TRY(hipStreamSynchronize(c.stream()));
    const uint64_t nv = M.list ? std::min<uint64_t>(M.vert_capacity, h[0]) : 0, nt = M.list ? std::min<uint64_t>(M.tri_capacity, h[1]) : 0;
    if (nv || nt) {
        CGRT_TRY(c.out(1, M.verts, nv * 12, "verts", &dverts));
        CGRT_TRY(c.out(2, M.tris, nt * 12, "tris", &dtris));
        Q.list = true;
        Q.verts = static_cast<float*>(dverts);
        Q.vert_capacity = nv;
        Q.tris = static_cast<uint32_t*>(dtris);
        Q.tri_capacity = nt;
        HIP_TRY(launch_isosurface(Q, nullptr, c.stream()));
    }
    counts2[0] = h[0];
    counts2[1] = h[1];
    return c.finish();
}
}  // namespace

int cgrt_isosurface_workspace(CgrtScene* s, const CgrtGrid* grid, uint64_t* bytes) {
    if (!s || !grid || !bytes) return fail(CGRT_E_ARG, "NULL argument");
    uint64_t N = 0;
    CGRT_TRY(iso_grid(grid, &N));
    *bytes = iso_workspace_bytes(N);
    return CGRT_OK;
}
int cgrt_isosurface_count_device(CgrtScene* s, const CgrtGrid* grid, const float* d_values, const CgrtIsoParams* params, uint64_t* d_counts2,
                                 void* d_workspace, uint64_t workspace_bytes, void* stream) {
    const IsoWorkspace ws{d_workspace, workspace_bytes};
    return iso_query(s, true, grid, d_values, params, {false, nullptr, 0, nullptr, 0}, d_counts2, &ws, false, nullptr, stream);
}
int cgrt_isosurface_device(CgrtScene* s, const CgrtGrid* grid, const float* d_values, const CgrtIsoParams* params, float* d_verts,
                           uint64_t vert_capacity, uint32_t* d_tris, uint64_t tri_capacity, uint64_t* d_counts2, void* d_workspace,
                           uint64_t workspace_bytes, void* stream) {
    const IsoWorkspace ws{d_workspace, workspace_bytes};
    return iso_query(s, true, grid, d_values, params, {true, d_verts, vert_capacity, d_tris, tri_capacity}, d_counts2, &ws, false, nullptr, stream);
}
int cgrt_isosurface(CgrtScene* s, const CgrtGrid* grid, const float* values, const CgrtIsoParams* params, float* verts, uint64_t vert_capacity,
                    uint32_t* tris, uint64_t tri_capacity, uint64_t* counts2) {
    return iso_query(s, false, grid, values, params, {true, verts, vert_capacity, tris, tri_capacity}, counts2, nullptr, false, nullptr, nullptr);
}
int cgrt_debug_isosurface_work(CgrtScene* s, const CgrtGrid* grid, const float* values, const CgrtIsoParams* params, uint64_t* out4) {
    return iso_query(s, false, grid, values, params, {false, nullptr, 0, nullptr, 0}, nullptr, nullptr, true, out4, nullptr);
}

// ---- grid fields (include/cgrt.h "Grid fields"): the trilinear sample of a scalar grid with its gradient, and the
// march of rays to a level of it.  The scene only names the device and lends the call lane; no frame state is read or written; the checks
// come in the order include/cgrt.h states, all before any device work.
namespace {
static_assert(sizeof(CgrtGridHit) == 32 && sizeof(CgrtMarchParams) == 28 && sizeof(CgrtFieldParams) == 8, "the records of include/cgrt.h");
static_assert(CGRT_FIELD_CLAMP == kFieldClamp && CGRT_ISO_INSIDE_ABOVE == kMarchInsideAbove && CGRT_MARCH_MISS == kMarchMiss &&
                  CGRT_MARCH_HIT == kMarchHit && CGRT_MARCH_EXHAUSTED == kMarchExhausted && CGRT_MARCH_NONFINITE == kMarchNonfinite,
              "the kernels' constants are the header's");
int field_grid(const CgrtGrid* grid, GridField* G, uint64_t* points) {
    uint64_t n = 1;
    for (int c = 0; c < 3; c++) {
        if (grid->dims[c] < 2 || grid->dims[c] > (1u << 24)) return fail(CGRT_E_ARG, "grid dims must be in 2..2^24");
        n *= grid->dims[c];  // (below 2^55 before the test, which follows every factor)
        if (n > kFieldMaxPoints) return fail(CGRT_E_ARG, "too many grid points: nx * ny * nz exceeds 0x7fffffff");
        if (!std::isfinite(grid->origin[c]) || !std::isfinite(grid->spacing[c])) return fail(CGRT_E_ARG, "grid origin and spacing must be finite");
        if (grid->spacing[c] == 0.0f) return fail(CGRT_E_ARG, "grid spacing must not be zero");
        G->origin[c] = grid->origin[c];
        G->spacing[c] = grid->spacing[c];
        G->top[c] = (float)(grid->dims[c] - 1u);
    }
    G->nx = grid->dims[0], G->ny = grid->dims[1], G->nz = grid->dims[2];
    *points = n;
    return CGRT_OK;
}
// slots: 0 the values, 1 the points, 2 value, 3 gradient, 4 inside
int field_sample_query(CgrtScene* s, bool device, const CgrtGrid* grid, const float* values, const float* points, uint64_t n,
                       const CgrtFieldParams* params, float* value, float* gradient, uint8_t* inside, void* stream) {
    if (!s || !grid) return fail(CGRT_E_ARG, "scene or grid is NULL");
    FieldSampleCall Q{};
    uint64_t N = 0;
    CGRT_TRY(field_grid(grid, &Q.grid, &N));
    if (params && (params->flags & ~(uint32_t)CGRT_FIELD_CLAMP)) return fail(CGRT_E_ARG, "unknown flags");
    if (!values) return fail(CGRT_E_ARG, "NULL argument: values");
    if (n && !points) return fail(CGRT_E_ARG, "NULL argument: points");
    if (!value && !gradient && !inside) return fail(CGRT_E_ARG, "NULL argument: none of value, gradient and inside is asked for");
    if (n > kFieldMaxPoints) return fail(CGRT_E_ARG, "too many points: n exceeds 0x7fffffff");
    if (device && ((uintptr_t)values % 4 || (uintptr_t)points % 4 || (uintptr_t)value % 4 || (uintptr_t)gradient % 4))
        return fail(CGRT_E_ARG, "d_values, d_points, d_value and d_gradient must be 4-byte aligned");
    NEED_DEVICE(s);
    if (n == 0) return CGRT_OK;
    Q.outside_bits = kCanonicalNan;
    if (params) memcpy(&Q.outside_bits, &params->outside, 4);
    Q.clamp = params && (params->flags & CGRT_FIELD_CLAMP) ? 1u : 0u;
    Q.n = (uint32_t)n;
    QueryCall c(s, device, stream);
    void *dv = nullptr, *dp = nullptr, *dval = nullptr, *dg = nullptr, *di = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, values, N * 4, "d_values", &dv));
    CGRT_TRY(c.in(1, points, n * 12, "d_points", &dp));
    CGRT_TRY(c.out(2, value, value ? n * 4 : 0, "d_value", &dval));
    CGRT_TRY(c.out(3, gradient, gradient ? n * 12 : 0, "d_gradient", &dg));
    CGRT_TRY(c.out(4, inside, inside ? n : 0, "d_inside", &di));
    Q.grid.values = static_cast<const float*>(dv);
    Q.points = static_cast<const float*>(dp);
    Q.value = static_cast<float*>(dval);
    Q.gradient = static_cast<float*>(dg);
    Q.inside = static_cast<uint8_t*>(di);
    HIP_TRY(launch_sample_grid(Q, c.stream()));
    return c.finish();
}
// slots: 0 the values, 1 the rays, 2 the records; work: the counting launch (host form only: out3 in the place of hits)
int field_march_query(CgrtScene* s, bool device, const CgrtGrid* grid, const float* values, const CgrtRay* rays, uint64_t n,
                      const CgrtMarchParams* params, CgrtGridHit* hits, bool counted, uint64_t* work, void* stream) {
    if (!s || !grid) return fail(CGRT_E_ARG, "scene or grid is NULL");
    FieldMarchCall Q{};
    uint64_t N = 0;
    CGRT_TRY(field_grid(grid, &Q.grid, &N));
    if (!params) return fail(CGRT_E_ARG, "NULL argument: params");
    if (!std::isfinite(params->iso)) return fail(CGRT_E_ARG, "iso must be finite");
    if (!std::isfinite(params->relax) || !(params->relax >= 0.0f)) return fail(CGRT_E_ARG, "relax must be finite and >= 0");
    if (!std::isfinite(params->min_step) || !(params->min_step > 0.0f)) return fail(CGRT_E_ARG, "min_step must be finite and > 0");
    if (!std::isfinite(params->hit_eps) || !(params->hit_eps >= 0.0f)) return fail(CGRT_E_ARG, "hit_eps must be finite and >= 0");
    if (params->max_steps < 1 || params->max_steps > 65536) return fail(CGRT_E_ARG, "max_steps must be in 1..65536");
    if (params->refine > 32) return fail(CGRT_E_ARG, "refine must be in 0..32");
    if (params->flags & ~(uint32_t)CGRT_ISO_INSIDE_ABOVE) return fail(CGRT_E_ARG, "unknown flags");
    if (!values) return fail(CGRT_E_ARG, "NULL argument: values");
    if (n && !rays) return fail(CGRT_E_ARG, "NULL argument: rays");
    if (counted ? !work : !hits) return fail(CGRT_E_ARG, counted ? "NULL argument: out3" : "NULL argument: hits");
    if (n > kFieldMaxPoints) return fail(CGRT_E_ARG, "too many rays: n exceeds 0x7fffffff");
    if (device && ((uintptr_t)values % 4 || (uintptr_t)rays % 4 || (uintptr_t)hits % 4))
        return fail(CGRT_E_ARG, "d_values, d_rays and d_hits must be 4-byte aligned");
    NEED_DEVICE(s);
    if (n == 0) {
        if (counted) work[0] = work[1] = work[2] = 0;
        return CGRT_OK;
    }
    Q.rules = {params->iso, params->relax, params->min_step, params->hit_eps, params->max_steps, params->refine,
               (params->flags & CGRT_ISO_INSIDE_ABOVE) ? 1u : 0u};
    Q.n = (uint32_t)n;
    QueryCall c(s, device, stream);
    void *dv = nullptr, *dr = nullptr, *dh = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, values, N * 4, "d_values", &dv));
    CGRT_TRY(c.in(1, rays, n * sizeof(CgrtRay), "d_rays", &dr));
    Q.grid.values = static_cast<const float*>(dv);
    Q.rays = static_cast<const float*>(dr);
    if (counted) {
        CGRT_TRY(c.zero_counters(3));
        HIP_TRY(launch_march_grid(Q, c.counters(), c.stream()));
        return c.read_counters(work, 3);
    }
    CGRT_TRY(c.out(2, hits, n * sizeof(CgrtGridHit), "d_hits", &dh));
    Q.hits = static_cast<uint32_t*>(dh);
    HIP_TRY(launch_march_grid(Q, nullptr, c.stream()));
    return c.finish();
}
// the sampler's adjoint (include/cgrt.h "Grid fields, the adjoint").  slots: 0 the points, 1 grad_value,
// 2 grad_gradient, 3 grad_values (host form: uploaded, added into, downloaded).  repro: the bitwise-reproducible form (DESIGN.md section
// 5.36), whose workspace is the caller's `ws` (device form) or the lane's slot 4 (host form)
int field_grad_query(CgrtScene* s, bool device, const CgrtGrid* grid, const float* points, uint64_t n, const CgrtFieldParams* params,
                     const float* grad_value, const float* grad_gradient, float* grad_values, bool repro, const ReproWorkspace* ws,
                     void* stream) {
    if (!s || !grid) return fail(CGRT_E_ARG, "scene or grid is NULL");
    FieldGradCall Q{};
    uint64_t N = 0;
    CGRT_TRY(field_grid(grid, &Q.grid, &N));
    if (params && (params->flags & ~(uint32_t)CGRT_FIELD_CLAMP)) return fail(CGRT_E_ARG, "unknown flags");
    if (n && !points) return fail(CGRT_E_ARG, "NULL argument: points");
    if (!grad_value && !grad_gradient) return fail(CGRT_E_ARG, "NULL argument: neither grad_value nor grad_gradient is given");
    if (!grad_values) return fail(CGRT_E_ARG, "NULL argument: grad_values");
    if (n > kFieldMaxPoints) return fail(CGRT_E_ARG, "too many points: n exceeds 0x7fffffff");
    if (device && ((uintptr_t)points % 4 || (uintptr_t)grad_value % 4 || (uintptr_t)grad_gradient % 4 || (uintptr_t)grad_values % 4))
        return fail(CGRT_E_ARG, "d_points, d_grad_value, d_grad_gradient and d_grad_values must be 4-byte aligned");
    if (n)
        CGRT_TRY(repro_workspace_args(ws, repro_workspace_bytes(N), "NULL argument: d_workspace", "cgrt_sample_grid_grad_repro_workspace"));
    NEED_DEVICE(s);
    if (n == 0) return CGRT_OK;
    Q.clamp = params && (params->flags & CGRT_FIELD_CLAMP) ? 1u : 0u;
    Q.n = (uint32_t)n;
    QueryCall c(s, device, stream);
    void *dp = nullptr, *dgv = nullptr, *dgg = nullptr, *dout = nullptr;
    CGRT_TRY(c.begin());
    CGRT_TRY(c.in(0, points, n * 12, "d_points", &dp));
    CGRT_TRY(c.in(1, grad_value, grad_value ? n * 4 : 0, "d_grad_value", &dgv));
    CGRT_TRY(c.in(2, grad_gradient, grad_gradient ? n * 12 : 0, "d_grad_gradient", &dgg));
    CGRT_TRY(c.inout(3, grad_values, N * 4, "d_grad_values", &dout));
    Q.points = static_cast<const float*>(dp);
    Q.grad_value = grad_value ? static_cast<const float*>(dgv) : nullptr;
    Q.grad_gradient = grad_gradient ? static_cast<const float*>(dgg) : nullptr;
    Q.grad_values = static_cast<float*>(dout);
    void* dws = nullptr;
    CGRT_TRY(repro_workspace_device(s, ws, repro ? &c.c : nullptr, repro_workspace_bytes(N), &dws));
    if (repro)
        HIP_TRY(launch_sample_grid_grad_repro(Q, N, dws, c.stream()));
    else
        HIP_TRY(launch_sample_grid_grad(Q, c.stream()));
    return c.finish();
}
}  // namespace

int cgrt_sample_grid(CgrtScene* s, const CgrtGrid* grid, const float* values, const float* points, uint64_t n, const CgrtFieldParams* params,
                     float* value, float* gradient, uint8_t* inside) {
    return field_sample_query(s, false, grid, values, points, n, params, value, gradient, inside, nullptr);
}
int cgrt_sample_grid_device(CgrtScene* s, const CgrtGrid* grid, const float* d_values, const float* d_points, uint64_t n,
                            const CgrtFieldParams* params, float* d_value, float* d_gradient, uint8_t* d_inside, void* stream) {
    return field_sample_query(s, true, grid, d_values, d_points, n, params, d_value, d_gradient, d_inside, stream);
}
int cgrt_sample_grid_grad(CgrtScene* s, const CgrtGrid* grid, const float* points, uint64_t n, const CgrtFieldParams* params,
                          const float* grad_value, const float* grad_gradient, float* grad_values) {
    return field_grad_query(s, false, grid, points, n, params, grad_value, grad_gradient, grad_values, false, nullptr, nullptr);
}
int cgrt_sample_grid_grad_device(CgrtScene* s, const CgrtGrid* grid, const float* d_points, uint64_t n, const CgrtFieldParams* params,
                                 const float* d_grad_value, const float* d_grad_gradient, float* d_grad_values, void* stream) {
    return field_grad_query(s, true, grid, d_points, n, params, d_grad_value, d_grad_gradient, d_grad_values, false, nullptr, stream);
}
int cgrt_sample_grid_grad_repro_workspace(CgrtScene* s, const CgrtGrid* grid, uint64_t* bytes) {
    if (!s || !grid || !bytes) return fail(CGRT_E_ARG, "NULL argument");
    GridField G{};
    uint64_t N = 0;
    CGRT_TRY(field_grid(grid, &G, &N));
    *bytes = repro_workspace_bytes(N);
    return CGRT_OK;
}
int cgrt_sample_grid_grad_repro(CgrtScene* s, const CgrtGrid* grid, const float* points, uint64_t n, const CgrtFieldParams* params,
                                const float* grad_value, const float* grad_gradient, float* grad_values) {
    return field_grad_query(s, false, grid, points, n, params, grad_value, grad_gradient, grad_values, true, nullptr, nullptr);
}
int cgrt_sample_grid_grad_repro_device(CgrtScene* s, const CgrtGrid* grid, const float* d_points, uint64_t n, const CgrtFieldParams* params,
                                       const float* d_grad_value, const float* d_grad_gradient, float* d_grad_values, void* d_workspace,
                                       uint64_t workspace_bytes, void* stream) {
    const ReproWorkspace ws{d_workspace, workspace_bytes};
    return field_grad_query(s, true, grid, d_points, n, params, d_grad_value, d_grad_gradient, d_grad_values, true, &ws, stream);
}
int cgrt_march_grid(CgrtScene* s, const CgrtGrid* grid, const float* values, const CgrtRay* rays, uint64_t n, const CgrtMarchParams* params,
                    CgrtGridHit* hits) {
    return field_march_query(s, false, grid, values, rays, n, params, hits, false, nullptr, nullptr);
}
int cgrt_march_grid_device(CgrtScene* s, const CgrtGrid* grid, const float* d_values, const CgrtRay* d_rays, uint64_t n,
                           const CgrtMarchParams* params, CgrtGridHit* d_hits, void* stream) {
    return field_march_query(s, true, grid, d_values, d_rays, n, params, d_hits, false, nullptr, stream);
}
int cgrt_debug_march_work(CgrtScene* s, const CgrtGrid* grid, const float* values, const CgrtRay* rays, uint64_t n, const CgrtMarchParams* params,
                          uint64_t* out3) {
    return field_march_query(s, false, grid, values, rays, n, params, nullptr, true, out3, nullptr);
}

}  // extern "C"
