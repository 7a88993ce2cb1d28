// capi_frame_entries.cpp -- the C entries of the shaded frame (cgrt_render*, cgrt_shade_rays*, cgrt_enqueue_render*,
// cgrt_enqueue_shade_rays_device): each checks its arguments in include/cgrt.h's order, builds a FrameRequest (capi_frames.h) and hands
// it to one of capi_frames.cpp's drivers.
#include "capi_internal.h"
#include "capi_frames.h"

// cgrt_shade_rays' rules for the spherical lights, which every frame entry shares; NULL = no spherical lights
int cgrt::soft_rules(const CgrtSoftShadows* soft) {
    if (soft && soft->nspherical &&
        (!soft->spherical || !soft->unit_vectors || soft->nunits == 0 || soft->samples == 0 || soft->samples > (1u << 24)))
        return fail(CGRT_E_ARG, "soft shadows need lights, a unit-vector table and 1..2^24 samples");
    return CGRT_OK;
}

// a request with where its driver reports: a blocking frame's stats, an enqueued frame's ticket
static int render_frame(CgrtScene* s, FrameRequest R, CgrtRenderStats* stats) {
    R.stats = stats;
    return render_impl(s, R);
}
static int enqueue_frame(CgrtScene* s, FrameRequest R, uint64_t* ticket) {
    R.ticket = ticket;
    return enqueue_impl(s, R);
}

extern "C" {

int cgrt_render(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, int max_level, float* rgb,
                CgrtRenderStats* stats) {
    return cgrt_render_rank(s, cam, W, H, lights, nlights, nullptr, max_level, 0, 1, rgb, stats);
}
int cgrt_render_counted(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, int max_level, float* rgb,
                        CgrtRenderStats* stats, CgrtCounters* work3) {
    if (!work3) return fail(CGRT_E_ARG, "work3 is NULL");
    FrameRequest R;
    R.cam = cam, R.W = W, R.H = H, R.lights = lights, R.nlights = nlights, R.max_level = max_level, R.rgb = rgb, R.stats = stats, R.counted = work3;
    return render_impl(s, R);
}
int cgrt_render_soft(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                     int max_level, float* rgb, CgrtRenderStats* stats) {
    return cgrt_render_rank(s, cam, W, H, lights, nlights, soft, max_level, 0, 1, rgb, stats);
}
int cgrt_render_mapped(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                       int max_level, const float** rgb, CgrtRenderStats* stats) {
    if (!rgb) return fail(CGRT_E_ARG, "rgb is NULL");
    FrameRequest R;
    R.cam = cam, R.W = W, R.H = H, R.lights = lights, R.nlights = nlights, R.soft = soft, R.max_level = max_level, R.mapped = rgb, R.stats = stats;
    return render_impl(s, R);
}
int cgrt_render_rank(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                     int max_level, int rank, int nranks, float* rgb, CgrtRenderStats* stats) {
    FrameRequest R;
    R.cam = cam, R.W = W, R.H = H, R.lights = lights, R.nlights = nlights, R.soft = soft, R.max_level = max_level, R.rank = rank, R.nranks = nranks;
    R.rgb = rgb, R.stats = stats;
    return render_impl(s, R);
}

// The anti-aliased entries check every argument before any device work (a host-only scene: CGRT_E_NO_DEVICE after the rest).
extern "C++" int cgrt::aa_args(const CgrtCamera* cam, const void* out, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                   int max_level, int rank, int nranks) {
    if (!cam || !out) return fail(CGRT_E_ARG, "NULL argument");
    if (nlights && !lights) return fail(CGRT_E_ARG, "nlights > 0 but lights is NULL");
    if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
    if (4ull * (unsigned long long)W * (unsigned long long)H > 0x7fffffffull) return fail(CGRT_E_ARG, "frame too large: 4*W*H sub-samples exceed 0x7fffffff");
    if (max_level < 0 || max_level > 16) return fail(CGRT_E_ARG, "bad recursion depth");
    if (nranks <= 0 || rank < 0 || rank >= nranks) return fail(CGRT_E_ARG, "bad rank / nranks");
    return soft_rules(soft);
}
int cgrt_render_aa(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                   int max_level, int rank, int nranks, float* rgb, CgrtRenderStats* stats) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    const int rc = aa_args(cam, rgb, W, H, lights, nlights, soft, max_level, rank, nranks);
    if (rc) return rc;
    NEED_DEVICE(s);
    FrameRequest R;
    R.cam = cam, R.W = W, R.H = H, R.lights = lights, R.nlights = nlights, R.soft = soft, R.max_level = max_level, R.rank = rank, R.nranks = nranks;
    R.aa = true, R.rgb = rgb, R.stats = stats;
    return render_impl(s, R);
}
int cgrt_render_aa_mapped(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                          int max_level, const float** rgb, CgrtRenderStats* stats) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    const int rc = aa_args(cam, rgb, W, H, lights, nlights, soft, max_level, 0, 1);
    if (rc) return rc;
    NEED_DEVICE(s);
    FrameRequest R;
    R.cam = cam, R.W = W, R.H = H, R.lights = lights, R.nlights = nlights, R.soft = soft, R.max_level = max_level, R.aa = true, R.mapped = rgb;
    R.stats = stats;
    return render_impl(s, R);
}

// The frame export's own arguments (cgrt_render_device, cgrt_debug_export_frame; W, H > 0 already checked): *pitch = the row pitch,
// *extent = bytes from out to one past the last byte the export may write.
extern "C++" int cgrt::export_args(const void* out, int W, int H, int format, uint64_t row_bytes, uint64_t* pitch, uint64_t* extent) {
    const uint64_t row = format == CGRT_FRAME_RGB_F32 ? 12ull * (uint64_t)W
                         : (format == CGRT_FRAME_CHW_F32 || format == CGRT_FRAME_RGBA8) ? 4ull * (uint64_t)W : 0;
    if (!row) return fail(CGRT_E_ARG, "unknown frame format");
    if (row_bytes && (row_bytes < row || row_bytes % 4)) return fail(CGRT_E_ARG, "row_bytes must be 0 or a multiple of 4 of at least the packed row");
    if ((uintptr_t)out % 4) return fail(CGRT_E_ARG, "the output buffer is not 4-byte aligned");
    const uint64_t p = row_bytes ? row_bytes : row, rows = (format == CGRT_FRAME_CHW_F32 ? 3ull : 1ull) * (uint64_t)H;
    if ((unsigned __int128)p * rows > ((unsigned __int128)1 << 62)) return fail(CGRT_E_ARG, "row_bytes too large");
    *pitch = p;
    *extent = p * (rows - 1) + row;
    return CGRT_OK;
}

// p .. p + bytes must be device memory of the scene's device (the current device is the scene's): one allocation, or several that follow
// one another in the address space (a caching allocator that maps its pool in pieces through the virtual-memory API, e.g. torch's
// expandable segments), each checked.  A pointer this HIP runtime does not know (another copy of the runtime in the process, host memory)
// is refused here, before any work.  Used by every entry that takes a caller's device buffer (cgrt_render_device, cgrt_shade_rays_device).
extern "C++" int cgrt::check_device_span(const CgrtScene* s, const void* p, uint64_t bytes, const char* name) {
    uintptr_t at = (uintptr_t)p;
    const uintptr_t end = at + bytes;
    for (int piece = 0; at < end; piece++) {
        if (piece == 65536) return fail(CGRT_E_ARG, std::string(name) + " spans too many separate allocations");
        hipPointerAttribute_t pa{};
        if (hipPointerGetAttributes(&pa, reinterpret_cast<void*>(at)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(CGRT_E_ARG, std::string(name) + (piece ? "'s allocation is smaller than the data" : " is not memory of this process's HIP runtime"));
        }
        if (pa.type != hipMemoryTypeDevice || pa.device != s->device) return fail(CGRT_E_ARG, std::string(name) + " is not device memory of the scene's device");
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, reinterpret_cast<hipDeviceptr_t>(at)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(CGRT_E_ARG, std::string(name) + ": no device allocation found");
        }
        if ((uintptr_t)base + size <= at) return fail(CGRT_E_ARG, std::string(name) + ": no device allocation found");
        at = (uintptr_t)base + size;
    }
    return CGRT_OK;
}

// The geometry buffers' own checks (include/cgrt.h CgrtAovOut), behind the counterpart's: aov_args before the host-only check, aov_spans
// (px pixels per plane) behind d_out's.
static int aov_args(const CgrtAovOut* aov, int max_level, int aa, int nranks) {
    if (!aov) return fail(CGRT_E_ARG, "aov is NULL");
    if (!aov->depth && !aov->normal && !aov->position && !aov->albedo && !aov->prim_id && !aov->material_id && !aov->mask)
        return fail(CGRT_E_ARG, "aov requests no plane");
    if (max_level == 0) return fail(CGRT_E_ARG, "max_level 0 traces no primary rays: there are no geometry buffers to export");
    if (aa && nranks > 1) return fail(CGRT_E_ARG, "anti-aliased geometry buffers are for nranks == 1 only");
    if ((uintptr_t)aov->depth % 4 || (uintptr_t)aov->normal % 4 || (uintptr_t)aov->position % 4 || (uintptr_t)aov->albedo % 4 ||
        (uintptr_t)aov->prim_id % 4 || (uintptr_t)aov->material_id % 4)
        return fail(CGRT_E_ARG, "a geometry-buffer plane is not aligned to its element size");
    return CGRT_OK;
}
static int aov_spans(const CgrtScene* s, const CgrtAovOut* aov, uint64_t px) {
    const struct {
        const void* p;
        uint64_t bytes;
        const char* name;
    } planes[7] = {{aov->depth, 4, "aov.depth"},     {aov->normal, 12, "aov.normal"},          {aov->position, 12, "aov.position"}, {aov->albedo, 12, "aov.albedo"},
                   {aov->prim_id, 4, "aov.prim_id"}, {aov->material_id, 4, "aov.material_id"}, {aov->mask, 1, "aov.mask"}};
    for (const auto& pl : planes) {
        if (!pl.p) continue;
        const int rc = check_device_span(s, pl.p, pl.bytes * px, pl.name);
        if (rc) return rc;
    }
    return CGRT_OK;
}
// cgrt_render_device's checks, in include/cgrt.h's order, all before any device work (cgrt_enqueue_render_device: the same); *pitch = the row pitch
// with_aov: cgrt_render_aov_device's, which adds the planes' checks
static int render_device_args(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                              int max_level, int aa, int rank, int nranks, void* d_out, int format, uint64_t row_bytes, uint64_t* pitch,
                              bool with_aov = false, const CgrtAovOut* aov = nullptr) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    if (aa) {
        const int rc = aa_args(cam, d_out, W, H, lights, nlights, soft, max_level, rank, nranks);
        if (rc) return rc;
    } else {
        if (!cam || !d_out) return fail(CGRT_E_ARG, "NULL argument");
        if (nlights && !lights) return fail(CGRT_E_ARG, "nlights > 0 but lights is NULL");
        if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
        if (max_level < 0 || max_level > 16) return fail(CGRT_E_ARG, "bad recursion depth");
        if (nranks <= 0 || rank < 0 || rank >= nranks) return fail(CGRT_E_ARG, "bad rank / nranks");
        if (const int rc = soft_rules(soft)) return rc;
        if (soft && soft->nspherical && (unsigned long long)W * H > 0x7fffffffull) return fail(CGRT_E_ARG, "frame too large");
    }
    uint64_t extent = 0;
    int rc = export_args(d_out, W, H, format, row_bytes, pitch, &extent);
    if (rc) return rc;
    if (with_aov && (rc = aov_args(aov, max_level, aa, nranks))) return rc;
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = check_device_span(s, d_out, extent, "d_out"))) return rc;
    return with_aov ? aov_spans(s, aov, (uint64_t)W * (uint64_t)H * (aa ? 4u : 1u)) : CGRT_OK;
}
// the request of the single-camera device entries, blocking and enqueued (D: filled by render_device_args)
static FrameRequest device_request(const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft, int max_level,
                                   int aa, int rank, int nranks, const DeviceOut* D, const CgrtAovOut* aov = nullptr) {
    FrameRequest R;
    R.cam = cam, R.W = W, R.H = H, R.lights = lights, R.nlights = nlights, R.soft = soft, R.max_level = max_level, R.rank = rank, R.nranks = nranks;
    R.aa = aa != 0, R.dout = D, R.aov = aov, R.stream = D->stream;
    return R;
}
int cgrt_render_device(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                       int max_level, int aa, int rank, int nranks, void* d_out, int format, uint64_t row_bytes, void* stream,
                       CgrtRenderStats* stats) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream)};
    const int rc = render_device_args(s, cam, W, H, lights, nlights, soft, max_level, aa, rank, nranks, d_out, format, row_bytes, &D.pitch);
    if (rc) return rc;
    return render_frame(s, device_request(cam, W, H, lights, nlights, soft, max_level, aa, rank, nranks, &D), stats);
}
int cgrt_render_aov_device(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                           int max_level, int aa, int rank, int nranks, void* d_out, int format, uint64_t row_bytes, void* stream,
                           CgrtRenderStats* stats, const CgrtAovOut* aov) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream)};
    const int rc = render_device_args(s, cam, W, H, lights, nlights, soft, max_level, aa, rank, nranks, d_out, format, row_bytes, &D.pitch, true, aov);
    if (rc) return rc;
    return render_frame(s, device_request(cam, W, H, lights, nlights, soft, max_level, aa, rank, nranks, &D, aov), stats);
}

// ---- renderRayTracing's per-pixel loop for a batch of cameras (render_impl, ViewSrc; include/cgrt.h cgrt_render_views*) ----
// cgrt_render_device's checks without aa / rank / row_bytes, with the batch's own (views_args) in place of the frame size check.
static int render_views_args(const CgrtScene* s, const void* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                             const CgrtSoftShadows* soft, int max_level, const void* out, const CgrtRayCamera* ray = nullptr) {
    if (!s || !out) return fail(CGRT_E_ARG, "NULL argument");
    if (nlights && !lights) return fail(CGRT_E_ARG, "nlights > 0 but lights is NULL");
    const int rc = views_args(cams, nviews, W, H, ray);
    if (rc) return rc;
    if (max_level < 0 || max_level > 16) return fail(CGRT_E_ARG, "bad recursion depth");
    return soft_rules(soft);
}
// the request of the views entries, blocking and enqueued (V: the batch; D: NULL, or filled by render_views_device_args)
static FrameRequest views_request(const ViewSrc* V, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft, int max_level,
                                  const DeviceOut* D = nullptr, const CgrtAovOut* aov = nullptr) {
    FrameRequest R;
    R.views = V, R.W = W, R.H = H, R.lights = lights, R.nlights = nlights, R.soft = soft, R.max_level = max_level, R.dout = D, R.aov = aov;
    if (D) R.stream = D->stream;
    return R;
}
int cgrt_render_views(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                      const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats) {
    const int rc = render_views_args(s, cams, nviews, W, H, lights, nlights, soft, max_level, rgb);
    if (rc) return rc;
    NEED_DEVICE(s);
    const ViewSrc V{cams, nviews};
    FrameRequest R = views_request(&V, W, H, lights, nlights, soft, max_level);
    R.rgb = rgb, R.stats = stats;
    return render_impl(s, R);
}
// cgrt_render_views_device's checks (cgrt_enqueue_render_views_device: the same); D->pitch and D->view_bytes are set
// (ray: the cameras are ray cameras, `cams` the same pointer)
static int render_views_device_args(CgrtScene* s, const void* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                                    const CgrtSoftShadows* soft, int max_level, void* d_out, int format, DeviceOut* D, bool with_aov = false,
                                    const CgrtAovOut* aov = nullptr, const CgrtRayCamera* ray = nullptr) {
    int rc = render_views_args(s, cams, nviews, W, H, lights, nlights, soft, max_level, d_out, ray);
    if (rc) return rc;
    uint64_t extent = 0;
    if ((rc = export_args(d_out, W, H, format, 0, &D->pitch, &extent))) return rc;
    D->view_bytes = extent;  // (packed rows: one view's frame is exactly its extent)
    if (with_aov && (rc = aov_args(aov, max_level, 0, 1))) return rc;
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = check_device_span(s, d_out, extent * nviews, "d_out"))) return rc;
    return with_aov ? aov_spans(s, aov, (uint64_t)W * (uint64_t)H * nviews) : CGRT_OK;
}
int cgrt_render_views_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                             const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, CgrtRenderStats* stats) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    const int rc = render_views_device_args(s, cams, nviews, W, H, lights, nlights, soft, max_level, d_out, format, &D);
    if (rc) return rc;
    const ViewSrc V{cams, nviews};
    return render_frame(s, views_request(&V, W, H, lights, nlights, soft, max_level, &D), stats);
}
int cgrt_render_views_aov_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                                 const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, CgrtRenderStats* stats,
                                 const CgrtAovOut* aov) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    const int rc = render_views_device_args(s, cams, nviews, W, H, lights, nlights, soft, max_level, d_out, format, &D, true, aov);
    if (rc) return rc;
    const ViewSrc V{cams, nviews};
    return render_frame(s, views_request(&V, W, H, lights, nlights, soft, max_level, &D, aov), stats);
}

// ---- one camera under a batch of light sets (render_impl, LightSetSrc; include/cgrt.h cgrt_render_light_sets*) ----
// The sets' own rules (light_sets_args, views_light_sets_args): nsets, the offsets, the light arrays and the sampling parameters.
static int sets_rules(const CgrtLightSets* sets, const CgrtSoftShadows* soft) {
    const uint32_t B = sets->nsets;
    if (B == 0 || B > 1024) return fail(CGRT_E_ARG, "nsets must be 1 .. 1024");
    const uint32_t* lo = sets->light_offsets;
    const uint32_t* so = sets->spherical_offsets;
    if (!lo) return fail(CGRT_E_ARG, "light_offsets is NULL");
    if (lo[0] != 0 || (so && so[0] != 0)) return fail(CGRT_E_ARG, "light set offsets must start at 0");
    for (uint32_t b = 0; b < B; b++)
        if (lo[b + 1] < lo[b] || (so && so[b + 1] < so[b])) return fail(CGRT_E_ARG, "light set offsets must not decrease");
    const uint32_t np = lo[B], ns = so ? so[B] : 0u;
    if (np && !sets->lights) return fail(CGRT_E_ARG, "point lights in the sets but lights is NULL");
    if (ns && !sets->spherical) return fail(CGRT_E_ARG, "spherical lights in the sets but spherical is NULL");
    if (soft && (soft->spherical || soft->nspherical)) return fail(CGRT_E_ARG, "soft carries the sampling parameters only: its spherical lights must be NULL and 0");
    if (ns && (!soft || !soft->unit_vectors || soft->nunits == 0 || soft->samples == 0 || soft->samples > (1u << 24)))
        return fail(CGRT_E_ARG, "spherical lights need soft: a unit-vector table and 1..2^24 samples");
    return CGRT_OK;
}
// The plan's bounds for px items per level (W*H, or nviews*W*H): a level's shadow list holds up to px x (distinct positions) rays, its
// soft-shadow counters px x (distinct keys), with 32-bit indices; the samples of a level stay below 2^37.
static int sets_bounds(unsigned long long px, const LightSetSrc& P, const CgrtSoftShadows* soft) {
    if (px * (P.points.size() / 6) > 0x7fffffffull) return fail(CGRT_E_ARG, "too many distinct point-light positions for the frame's 32-bit shadow list");
    if (px * P.sph_index.size() > 0x7fffffffull || (!P.sph_index.empty() && px * P.sph_index.size() * soft->samples > 0x7fffffffull * 64))
        return fail(CGRT_E_ARG, "too many distinct spherical lights for the frame's 32-bit soft-shadow lists");
    return CGRT_OK;
}
// Every check of include/cgrt.h's list, all CGRT_E_ARG and before any device work; then *P holds the batch's plan.
static int light_sets_args(const CgrtScene* s, const CgrtCamera* cam, int W, int H, const CgrtLightSets* sets, const CgrtSoftShadows* soft,
                           int max_level, const void* out, LightSetSrc* P) {
    if (!s || !cam || !sets || !out) return fail(CGRT_E_ARG, "NULL argument");
    const int rc = sets_rules(sets, soft);
    if (rc) return rc;
    if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
    if (max_level < 0 || max_level > 16) return fail(CGRT_E_ARG, "bad recursion depth");
    const unsigned long long px = (unsigned long long)W * (unsigned long long)H;
    if (px > 0x7fffffffull) return fail(CGRT_E_ARG, "frame too large: W*H exceeds 0x7fffffff");
    plan_light_sets(*sets, *P);
    return sets_bounds(px, *P, soft);
}
// the request of the light-set entries, blocking and enqueued (V: NULL or the batch of views; P: the checked plan; D: NULL or filled)
static FrameRequest sets_request(const CgrtCamera* cam, const ViewSrc* V, int W, int H, const LightSetSrc& P, const CgrtSoftShadows* soft, int max_level,
                                 const DeviceOut* D = nullptr) {
    FrameRequest R;
    R.cam = cam, R.views = V, R.W = W, R.H = H, R.soft = soft, R.max_level = max_level, R.dout = D;
    R.use_sets(P);
    if (D) R.stream = D->stream;
    return R;
}
int cgrt_render_light_sets(CgrtScene* s, const CgrtCamera* cam, int W, int H, const CgrtLightSets* sets, const CgrtSoftShadows* soft, int max_level,
                           float* rgb, CgrtRenderStats* stats) {
    LightSetSrc P;
    const int rc = light_sets_args(s, cam, W, H, sets, soft, max_level, rgb, &P);
    if (rc) return rc;
    NEED_DEVICE(s);
    FrameRequest R = sets_request(cam, nullptr, W, H, P, soft, max_level);
    R.rgb = rgb, R.stats = stats;
    return render_impl(s, R);
}
int cgrt_render_light_sets_device(CgrtScene* s, const CgrtCamera* cam, int W, int H, const CgrtLightSets* sets, const CgrtSoftShadows* soft,
                                  int max_level, void* d_out, int format, void* stream, CgrtRenderStats* stats) {
    LightSetSrc P;
    int rc = light_sets_args(s, cam, W, H, sets, soft, max_level, d_out, &P);
    if (rc) return rc;
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    uint64_t extent = 0;
    if ((rc = export_args(d_out, W, H, format, 0, &D.pitch, &extent))) return rc;
    D.view_bytes = extent;  // (packed rows: one set's frame is exactly its extent)
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = check_device_span(s, d_out, extent * P.nsets, "d_out"))) return rc;
    return render_frame(s, sets_request(cam, nullptr, W, H, P, soft, max_level, &D), stats);
}

// ---- nviews cameras under a batch of light sets (render_impl / enqueue_impl with a ViewSrc and a LightSetSrc; include/cgrt.h
// cgrt_render_views_light_sets*) ----
// Every check of include/cgrt.h's list, in its order, all CGRT_E_ARG and before any device work; then *P holds the batch's plan.
// (ray: the cameras are ray cameras, `cams` the same pointer, checked where cams is)
static int views_light_sets_args(const CgrtScene* s, const void* cams, uint32_t nviews, int W, int H, const CgrtLightSets* sets,
                                 const CgrtSoftShadows* soft, int max_level, const void* out, LightSetSrc* P, const CgrtRayCamera* ray = nullptr) {
    if (!s || !cams || !sets || !out) return fail(CGRT_E_ARG, "NULL argument");
    int rc = ray ? raycams_check(ray, nviews, W, H) : CGRT_OK;
    if (rc) return rc;
    if (nviews == 0) return fail(CGRT_E_ARG, "nviews must be at least 1");
    if ((rc = sets_rules(sets, soft))) return rc;
    if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
    if (max_level < 0 || max_level > 16) return fail(CGRT_E_ARG, "bad recursion depth");
    if ((rc = views_extent_args(nviews, W, H))) return rc;
    const unsigned long long px = (unsigned long long)nviews * (unsigned long long)W * (unsigned long long)H;
    plan_light_sets(*sets, *P);
    if ((rc = sets_bounds(px, *P, soft))) return rc;
    if (px * sets->nsets > 0x7fffffffull) return fail(CGRT_E_ARG, "batch too large: nviews*nsets*W*H exceeds 0x7fffffff");
    return CGRT_OK;
}
// the device forms' checks (blocking and enqueued): D->pitch and D->view_bytes are set
static int views_light_sets_device_args(CgrtScene* s, const void* cams, uint32_t nviews, int W, int H, const CgrtLightSets* sets,
                                        const CgrtSoftShadows* soft, int max_level, void* d_out, int format, LightSetSrc* P, DeviceOut* D,
                                        const CgrtRayCamera* ray = nullptr) {
    int rc = views_light_sets_args(s, cams, nviews, W, H, sets, soft, max_level, d_out, P, ray);
    if (rc) return rc;
    uint64_t extent = 0;
    if ((rc = export_args(d_out, W, H, format, 0, &D->pitch, &extent))) return rc;
    D->view_bytes = extent;  // (packed rows: one frame is exactly its extent; frame (v, s) is frame v * nsets + s)
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    return check_device_span(s, d_out, extent * nviews * P->nsets, "d_out");
}
int cgrt_render_views_light_sets(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const CgrtLightSets* sets,
                                 const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats) {
    LightSetSrc P;
    const int rc = views_light_sets_args(s, cams, nviews, W, H, sets, soft, max_level, rgb, &P);
    if (rc) return rc;
    NEED_DEVICE(s);
    const ViewSrc V{cams, nviews};
    FrameRequest R = sets_request(nullptr, &V, W, H, P, soft, max_level);
    R.rgb = rgb, R.stats = stats;
    return render_impl(s, R);
}
int cgrt_render_views_light_sets_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const CgrtLightSets* sets,
                                        const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, CgrtRenderStats* stats) {
    LightSetSrc P;
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    const int rc = views_light_sets_device_args(s, cams, nviews, W, H, sets, soft, max_level, d_out, format, &P, &D);
    if (rc) return rc;
    const ViewSrc V{cams, nviews};
    return render_frame(s, sets_request(nullptr, &V, W, H, P, soft, max_level, &D), stats);
}

// ---- ray cameras (include/cgrt.h CgrtRayCamera): the views entries with a ViewSrc that carries ray cameras ----
int cgrt_render_raycams_device(CgrtScene* s, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                               const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, CgrtRenderStats* stats,
                               const CgrtAovOut* aov) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    const int rc = render_views_device_args(s, cams, nviews, W, H, lights, nlights, soft, max_level, d_out, format, &D, aov != nullptr, aov, cams);
    if (rc) return rc;
    const ViewSrc V{nullptr, nviews, cams};
    return render_frame(s, views_request(&V, W, H, lights, nlights, soft, max_level, &D, aov), stats);
}
int cgrt_render_raycams_light_sets_device(CgrtScene* s, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const CgrtLightSets* sets,
                                          const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, CgrtRenderStats* stats) {
    LightSetSrc P;
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    const int rc = views_light_sets_device_args(s, cams, nviews, W, H, sets, soft, max_level, d_out, format, &P, &D, cams);
    if (rc) return rc;
    const ViewSrc V{nullptr, nviews, cams};
    return render_frame(s, sets_request(nullptr, &V, W, H, P, soft, max_level, &D), stats);
}

// ---- getFinalColor of the caller's rays (main.cpp:298-310): level 0 of the wavefront from a ray list (render_impl, ListSrc) ----
// Every argument is checked before any device work, in the order include/cgrt.h states; a host-only scene is CGRT_E_NO_DEVICE after that.
static int shade_rays_args(const CgrtScene* s, const void* rays, uint64_t n, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                           int max_level, const void* rgb) {
    if (!s || !rgb || (n > 0 && !rays) || (nlights && !lights)) return fail(CGRT_E_ARG, "NULL argument");
    if (n > 0x7fffffffull) return fail(CGRT_E_ARG, "too many rays: n exceeds 0x7fffffff");
    if (max_level < 0 || max_level > 16) return fail(CGRT_E_ARG, "bad recursion depth");
    if (const int rc = soft_rules(soft)) return rc;
    NEED_DEVICE(s);
    return CGRT_OK;
}
// the request of the ray-list entries, blocking and enqueued (stream: where the ticket of an enqueued list goes)
static FrameRequest list_request(const ListSrc* src, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft, int max_level) {
    FrameRequest R;
    R.list = src, R.lights = lights, R.nlights = nlights, R.soft = soft, R.max_level = max_level, R.stream = src->stream;
    return R;
}
// cgrt_shade_rays_device's checks (cgrt_enqueue_shade_rays_device: the same); n == 0 needs no buffers
static int shade_rays_device_args(CgrtScene* s, const CgrtRay* d_rays, uint64_t n, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                                  int max_level, float* d_rgb) {
    int rc = shade_rays_args(s, d_rays, n, lights, nlights, soft, max_level, d_rgb);
    if (rc || n == 0) return rc;
    if ((uintptr_t)d_rays % 4 || (uintptr_t)d_rgb % 4) return fail(CGRT_E_ARG, "d_rays and d_rgb must be 4-byte aligned");
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = check_device_span(s, d_rays, n * sizeof(CgrtRay), "d_rays")) != CGRT_OK) return rc;
    return check_device_span(s, d_rgb, n * 12, "d_rgb");
}
int cgrt_shade_rays_device(CgrtScene* s, const CgrtRay* d_rays, uint64_t n, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                           int max_level, float* d_rgb, void* stream, CgrtRenderStats* stats) {
    const int rc = shade_rays_device_args(s, d_rays, n, lights, nlights, soft, max_level, d_rgb);
    if (rc) return rc;
    if (n == 0) {
        if (stats) *stats = CgrtRenderStats{};
        return CGRT_OK;
    }
    const ListSrc src{reinterpret_cast<const float*>(d_rays), n, d_rgb, static_cast<hipStream_t>(stream)};
    return render_frame(s, list_request(&src, lights, nlights, soft, max_level), stats);
}
int cgrt_shade_rays(CgrtScene* s, const CgrtRay* rays, uint64_t n, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                    int max_level, float* rgb, CgrtRenderStats* stats) {
    int rc = shade_rays_args(s, rays, n, lights, nlights, soft, max_level, rgb);
    if (rc) return rc;
    if (n == 0) {
        if (stats) *stats = CgrtRenderStats{};
        return CGRT_OK;
    }
    // the rays go up and the colours come down through a call lane's pinned staging, on the lane's stream
    LaneCall c(s);
    if ((rc = c.begin()) != CGRT_OK) return rc;
    void *dr = nullptr, *dc = nullptr;
    HIP_TRY(c.input(0, rays, n * sizeof(CgrtRay), &dr));
    HIP_TRY(c.scratch(1, n * 12, &dc));
    const ListSrc src{static_cast<const float*>(dr), n, static_cast<float*>(dc), c.stream()};
    rc = render_frame(s, list_request(&src, lights, nlights, soft, max_level), stats);
    if (rc) return rc;
    HIP_TRY(c.output(1, rgb, dc, n * 12));
    HIP_TRY(c.finish());
    return CGRT_OK;
}
int cgrt_enqueue_render_device(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                               int max_level, int aa, int rank, int nranks, void* d_out, int format, uint64_t row_bytes, void* stream,
                               uint64_t* ticket) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream)};
    const int rc = render_device_args(s, cam, W, H, lights, nlights, soft, max_level, aa, rank, nranks, d_out, format, row_bytes, &D.pitch);
    if (rc) return rc;
    return enqueue_frame(s, device_request(cam, W, H, lights, nlights, soft, max_level, aa, rank, nranks, &D), ticket);
}
int cgrt_enqueue_render_views_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                                     const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, uint64_t* ticket) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    const int rc = render_views_device_args(s, cams, nviews, W, H, lights, nlights, soft, max_level, d_out, format, &D);
    if (rc) return rc;
    const ViewSrc V{cams, nviews};
    return enqueue_frame(s, views_request(&V, W, H, lights, nlights, soft, max_level, &D), ticket);
}
int cgrt_enqueue_render_aov_device(CgrtScene* s, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                                   int max_level, int aa, int rank, int nranks, void* d_out, int format, uint64_t row_bytes, void* stream,
                                   uint64_t* ticket, const CgrtAovOut* aov) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream)};
    const int rc = render_device_args(s, cam, W, H, lights, nlights, soft, max_level, aa, rank, nranks, d_out, format, row_bytes, &D.pitch, true, aov);
    if (rc) return rc;
    return enqueue_frame(s, device_request(cam, W, H, lights, nlights, soft, max_level, aa, rank, nranks, &D, aov), ticket);
}
int cgrt_enqueue_render_views_aov_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                                         const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, uint64_t* ticket,
                                         const CgrtAovOut* aov) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    const int rc = render_views_device_args(s, cams, nviews, W, H, lights, nlights, soft, max_level, d_out, format, &D, true, aov);
    if (rc) return rc;
    const ViewSrc V{cams, nviews};
    return enqueue_frame(s, views_request(&V, W, H, lights, nlights, soft, max_level, &D, aov), ticket);
}
int cgrt_enqueue_render_raycams_device(CgrtScene* s, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, const float* lights, uint32_t nlights,
                                       const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, uint64_t* ticket,
                                       const CgrtAovOut* aov) {
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    const int rc = render_views_device_args(s, cams, nviews, W, H, lights, nlights, soft, max_level, d_out, format, &D, aov != nullptr, aov, cams);
    if (rc) return rc;
    const ViewSrc V{nullptr, nviews, cams};
    return enqueue_frame(s, views_request(&V, W, H, lights, nlights, soft, max_level, &D, aov), ticket);
}
int cgrt_enqueue_render_views_light_sets_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, const CgrtLightSets* sets,
                                                const CgrtSoftShadows* soft, int max_level, void* d_out, int format, void* stream, uint64_t* ticket) {
    LightSetSrc P;
    DeviceOut D{d_out, format, 0, static_cast<hipStream_t>(stream), 0};
    const int rc = views_light_sets_device_args(s, cams, nviews, W, H, sets, soft, max_level, d_out, format, &P, &D);
    if (rc) return rc;
    const ViewSrc V{cams, nviews};
    return enqueue_frame(s, sets_request(nullptr, &V, W, H, P, soft, max_level, &D), ticket);
}
int cgrt_enqueue_shade_rays_device(CgrtScene* s, const CgrtRay* d_rays, uint64_t n, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
                                   int max_level, float* d_rgb, void* stream, uint64_t* ticket) {
    const int rc = shade_rays_device_args(s, d_rays, n, lights, nlights, soft, max_level, d_rgb);
    if (rc) return rc;
    const ListSrc src{reinterpret_cast<const float*>(d_rays), n, d_rgb, static_cast<hipStream_t>(stream)};
    return enqueue_frame(s, list_request(&src, lights, nlights, soft, max_level), ticket);
}

int cgrt_debug_export_frame(int device, const float* rgb, int W, int H, int format, uint64_t row_bytes, void* out) {
    if (!rgb || !out) return fail(CGRT_E_ARG, "NULL argument");
    if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
    uint64_t pitch = 0, extent = 0;
    int rc = export_args(out, W, H, format, row_bytes, &pitch, &extent);
    if (rc) return rc;
    if ((rc = select_device(device)) != CGRT_OK) return rc;
    DevBuf src, dst;
    HIP_TRY(src.alloc((size_t)W * H * 12));
    HIP_TRY(dst.alloc(extent));
    HIP_TRY(hipMemcpy(src.p, rgb, (size_t)W * H * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dst.p, out, extent, hipMemcpyHostToDevice));  // (bytes the export must not touch come back as they were)
    ExportDev E{};
    E.src = src.as<float>();
    E.dst = dst.as<unsigned char>();
    E.pitch = pitch;
    E.W = W;
    E.H = H;
    E.format = format;
    HIP_TRY(launch_export_frame(E, nullptr));
    HIP_TRY(hipMemcpy(out, dst.p, extent, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

}  // extern "C"
