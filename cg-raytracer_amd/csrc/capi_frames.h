// capi_frames.h -- what the shaded frame's units share (capi_frames.cpp: the two drivers; capi_frame_entries.cpp: the C entries that
// build their requests; capi_multi.cpp: the replicas' frames): the request and its sources, the drivers, the workspace's buffers.
// Host code only, hidden visibility, like capi_internal.h.
#pragma once
#include "capi_internal.h"

struct WsBuf {  // a slot of the scene's workspace, with DevBuf's interface
    CgrtScene* sc;
    int slot;
    void* p = nullptr;
    hipError_t alloc(size_t bytes) {
        CgrtScene::WorkSlot& w = sc->work[slot];
        if (w.cap < bytes || !w.p) {
            // enqueued frames (and a blocking frame's export) may still use the buffer: they finish before it is released
            if (w.p && sc->enq_pending) {
                const hipError_t e = hipEventSynchronize(sc->enq_done);
                if (e != hipSuccess) return e;
                sc->enq_pending = false;
            }
            if (w.p && sc->export_pending) {
                const hipError_t e = hipEventSynchronize(sc->export_done);
                if (e != hipSuccess) return e;
            }
            if (w.p) (void)hipFree(w.p);
            w.p = nullptr;
            w.cap = 0;
            const hipError_t e = hipMalloc(&w.p, bytes ? bytes : 1);
            if (e != hipSuccess) return e;
            w.cap = bytes ? bytes : 1;
        }
        p = w.p;
        return hipSuccess;
    }
    size_t cap() const { return sc->work[slot].cap; }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

struct DeviceOut {
    void* p;
    int format;        // CGRT_FRAME_*
    uint64_t pitch;    // bytes from row to row (never 0 here)
    hipStream_t stream;
    uint64_t view_bytes;  // (a batch of views) bytes from one view's frame to the next
};
// Level 0 from a caller's ray list instead of the camera's frame (cgrt_shade_rays*): n > 0 rays in device memory of the scene's device,
// colours into rgb (n x 3 floats, device memory), both ordered on `stream`: the frame's work starts behind everything queued there
// before the call, and the stream waits for the frame's end.  The rest of the frame -- the level loop, the fold, k_write_rgb and the
// soft shadows -- is the camera frame's own; the list always takes the exactly sized path, and neither reads nor writes the scene's
// prediction record or its frame hints.
struct ListSrc {
    const float* rays;
    unsigned long long n;
    float* rgb;
    hipStream_t stream;
};
// Level 0 from nviews cameras instead of one (cgrt_render_views*): every view a whole W x H frame, their super-tiles ONE primary launch
// (the VIEWS kernels) and one set of wavefront lists; pixel = view * W * H + y * W + x, so the frame buffer holds the views back to back
// and the soft-shadow samples are drawn with pixel % (W * H).  Whole frames, one rank, no aa.  Like a ray list, the batch always takes
// the exactly sized path and neither reads nor writes the scene's prediction record or its frame hints.
struct ViewSrc {
    const CgrtCamera* cams;
    uint32_t n;
    const CgrtRayCamera* raycams = nullptr;  // the batch's cameras are ray cameras (cgrt_*_raycams*; cams is NULL): the RAYCAM kernels
    size_t table_bytes() const { return (size_t)n * (raycams ? sizeof(RayCameraDev) : sizeof(CameraDev)); }
};
// One camera under nsets light sets instead of one light list (cgrt_render_light_sets*): the batch's plan, built on
// the host from the caller's CSR arrays (plan_light_sets).  A pixel's ray tree does not depend on the lights, so level 0, every level's
// spawn and every mirror list run once.  A point light's shadow ray depends on its position alone, so each level's shadow list holds one ray
// per hit and DISTINCT position, compared by bit pattern: `points` is k_spawn's light list.  A spherical light's sample count depends on
// its position, its radius and its index within its set (the draws' `l`): the soft-shadow keys are the distinct (position, radius, index)
// triples, `spherical`, drawn as light `sph_index`.  `table` is SetsDev's memory: point_off[nsets + 1] | sph_off[nsets + 1] |
// sph_index[nsph] | (to 16 B) | every point light, then every spherical light, as {position, slot}, {colour, 0}.  Set b's frame is pixels
// b * W * H .. of the frame buffer.  Whole frames, one rank, no aa; like views, the batch always takes the exactly sized path and neither
// reads nor writes the scene's prediction record or its frame hints.
struct LightSetSrc {
    uint32_t nsets = 0;
    std::vector<float> points;        // npos x 6 {position, 0}
    std::vector<float> spherical;     // nsph x 7 {position, radius, 0}
    std::vector<uint32_t> sph_index;  // nsph: the in-set index each key draws with
    std::vector<uint32_t> table;
    size_t point_at = 0, sph_at = 0;  // words of `table` before the point / spherical light records
};

// ---- The shaded frame as both of its drivers see it (render_impl: blocking; enqueue_impl: without a host round trip) ----
// What a frame entry asks for.  Each C entry runs its own argument check and fills the fields it means; the others keep their defaults.
// rgb (optional): the caller's frame; mapped (optional): receives the scene's pinned staging frame (valid until the next
// cgrt_render* call on this scene).  With nranks > 1 only the pixels this rank owns are meaningful in the staging frame, and only
// those are copied into rgb (pixels of other ranks keep the caller's contents).
// aa: the reference's antiAliasing branch (main.cpp:663-687): the wavefront shades the 2W x 2H sub-sample frame, ranks own its
// 64x64 super-tiles (32x32 pixel blocks of the W x H frame), k_resolve_aa writes the W x H frame on the device and only that comes
// down (nranks > 1: only this rank's pixels, packed).  The caller has checked the arguments (aa_args).
// dout (cgrt_render_device, instead of rgb / mapped): nothing comes down; k_export_frame writes this rank's pixels of the W x H frame
// into the caller's device buffer on the caller's stream (behind the frame, and behind whatever the caller queued there before).
struct FrameRequest {
    const CgrtCamera* cam = nullptr;  // level 0: one camera's W x H frame, or a caller's ray list, or a batch of views of W x H each
    const ListSrc* list = nullptr;
    const ViewSrc* views = nullptr;
    int W = 1, H = 1;
    const float* lights = nullptr;  // point lights, nlights x 6
    uint32_t nlights = 0;
    const LightSetSrc* sets = nullptr;      // a batch of light sets instead (use_sets)
    const CgrtSoftShadows* soft = nullptr;  // spherical lights and their sampling (light sets: the sampling parameters only)
    int max_level = 0;
    int rank = 0, nranks = 1;
    bool aa = false;
    float* rgb = nullptr;  // (a ray list's colours go to list->rgb instead of these three)
    const float** mapped = nullptr;
    const DeviceOut* dout = nullptr;
    const CgrtAovOut* aov = nullptr;
    CgrtCounters* counted = nullptr;   // (blocking frames) 3 blocks of work counters
    CgrtRenderStats* stats = nullptr;  // (blocking frames)
    hipStream_t stream = nullptr;      // (enqueued frames) the caller's stream
    uint64_t* ticket = nullptr;        // (enqueued frames) receives the frame's number
    void use_sets(const LightSetSrc& P) {  // (k_spawn's light list is the batch's distinct positions)
        sets = &P;
        lights = P.points.data();
        nlights = (uint32_t)(P.points.size() / 6);
    }
    // (light sets: the batch's distinct spherical keys, with the caller's sampling parameters; light_sets_args has checked them)
    unsigned spherical() const { return sets ? (unsigned)sets->sph_index.size() : soft ? soft->nspherical : 0; }
};

#pragma GCC visibility push(hidden)
namespace cgrt {
// ---- capi_frames.cpp
void plan_light_sets(const CgrtLightSets& L, LightSetSrc& P);
int render_impl(CgrtScene* s, const FrameRequest& R);
int enqueue_impl(CgrtScene* s, const FrameRequest& R);
}  // namespace cgrt
#pragma GCC visibility pop
