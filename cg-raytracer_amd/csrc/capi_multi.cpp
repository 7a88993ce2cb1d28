// capi_multi.cpp -- one caller, several replicas of a scene on their own devices, one frame: cgrt_trace_primary_multi, cgrt_render_multi*.
#include "capi_internal.h"
#include "capi_frames.h"

// ------------------------------------------------------------------------------------------------
// One caller, N devices, one framebuffer (main.cpp:648-720 yields ONE Screen).  scenes[i] is a
// replica of the scene on its own device (the same device may appear several times); replica i traces the super-tiles
// i % nscenes.  All launches are issued first, each on a private stream of its replica; every device then downloads its
// pixels with ONE asynchronous copy (the kernel writes them back to back, FrameDev::packed) and a host thread per replica
// scatters them into the caller's frame.
namespace {
// pixel of lane (r, c) = row r, column c of the 8x8 tile of wave w of workgroup b: the host mirror of tile_pixel_of()
inline bool tile_origin(const FrameDev& F, uint32_t b, uint32_t w, int& x, int& y) {
    const uint32_t lane8 = b & 7u, j = b >> 3;
    const uint32_t wpb = (uint32_t)F.block / 64u, bps = 64u / wpb;
    const uint32_t sl = (j / bps) * 8u + lane8;
    if (sl >= F.nst_rank) return false;
    const uint32_t st = (uint32_t)F.rank + (uint32_t)F.nranks * sl;
    const int stx = (int)(st % (uint32_t)F.st_x), sty = (int)(st / (uint32_t)F.st_x);
    const int idx = (int)((j % bps) * wpb + w);
    x = F.x0 + (stx * ST_TILES + (idx & 7)) * 8;
    y = F.y0 + (sty * ST_TILES + (idx >> 3)) * 8;
    return x < F.x1 && y < F.y1;
}
}  // namespace

// cgrt_render_multi*: one host thread per replica (arguments checked by the caller)
static int render_replicas(CgrtScene* const* scenes, int nscenes, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                           const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats, bool aa) {
    // every replica renders its super-tiles (shading included: a pixel's secondary rays stay on the device that owns it) into a
    // frame of its own on a host thread of its own; the owned pixels are then merged into the caller's frame
    std::vector<CgrtRenderStats> st(nscenes);
    std::vector<int> status(nscenes, CGRT_OK);
    std::vector<std::string> errs(nscenes);
    auto work = [&](int i) {
        // render_impl downloads the replica's frame into its scene's pinned staging and copies ONLY the super-tiles rank i owns
        // into the caller's frame: disjoint regions, so the replicas' threads write rgb concurrently without a merge pass
        FrameRequest R;
        R.cam = cam, R.W = W, R.H = H, R.lights = lights, R.nlights = nlights, R.soft = soft, R.max_level = max_level, R.rank = i, R.nranks = nscenes;
        R.aa = aa, R.rgb = rgb, R.stats = &st[i];
        status[i] = render_impl(scenes[i], R);
        if (status[i]) errs[i] = g_err;  // (thread-local: carried over to the caller's thread below)
    };
    {
        std::vector<std::thread> pool;
        for (int i = 1; i < nscenes; i++) pool.emplace_back(work, i);
        work(0);
        for (std::thread& t : pool) t.join();
    }
    for (int i = 0; i < nscenes; i++)
        if (status[i]) return fail(status[i], errs[i]);
    CgrtRenderStats tot{};
    for (int i = 0; i < nscenes; i++) {
        tot.primary_rays += st[i].primary_rays;
        tot.shadow_rays += st[i].shadow_rays;
        tot.reflection_rays += st[i].reflection_rays;
        tot.soft_shadow_rays += st[i].soft_shadow_rays;
        tot.levels = std::max(tot.levels, st[i].levels);
        tot.device_ms = std::max(tot.device_ms, st[i].device_ms);
    }
    if (stats) *stats = tot;
    return CGRT_OK;
}

extern "C" {

int cgrt_trace_primary_multi(CgrtScene* const* scenes, int nscenes, const CgrtCamera* cam, int W, int H, CgrtHit* hits, float* normals,
                             CgrtMultiStats* stats) {
    if (!scenes || nscenes <= 0 || nscenes > 64 || !cam || !hits) return fail(CGRT_E_ARG, "NULL argument or bad replica count");
    for (int i = 0; i < nscenes; i++) {
        if (!scenes[i]) return fail(CGRT_E_ARG, "NULL scene");
        NEED_DEVICE(scenes[i]);
        for (int k = 0; k < i; k++)
            if (scenes[k] == scenes[i]) return fail(CGRT_E_ARG, "the same replica twice: create one scene per rank (the same device may repeat)");
    }
    if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
    const CameraDev C = make_camera(*cam);
    struct Part {
        FrameDev F;
        LaneCall* c = nullptr;
        void *dh = nullptr, *dn = nullptr, *ph = nullptr, *pn = nullptr;
        size_t n = 0;
        hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
        ~Part() {
            for (hipEvent_t e : {e0, e1, e2})
                if (e) (void)hipEventDestroy(e);
            delete c;
        }
    };
    std::vector<Part> part(nscenes);
    const auto t_begin = std::chrono::steady_clock::now();
    for (int i = 0; i < nscenes; i++) {  // issue everything, wait for nothing
        Part& P = part[i];
        if (!make_frame(W, H, 0, 0, W, H, i, nscenes, trace_block(scenes[i]->dev), P.F)) return fail(CGRT_E_ARG, "bad frame");
        P.F.packed = 1;
        apply_frame_gate(scenes[i], C, P.F);
        P.n = (size_t)P.F.nblocks * (size_t)P.F.block;
        if (P.n == 0) continue;
        P.c = new LaneCall(scenes[i]);
        int rc = P.c->begin();
        if (rc) return rc;
        HIP_TRY(P.c->scratch(1, P.n * sizeof(CgrtHit), &P.dh));
        HIP_TRY(P.c->g.pin(1, P.n * sizeof(CgrtHit), &P.ph));
        if (normals) {
            HIP_TRY(P.c->scratch(2, P.n * 12, &P.dn));
            HIP_TRY(P.c->g.pin(2, P.n * 12, &P.pn));
        }
        HIP_TRY(hipEventCreate(&P.e0));
        HIP_TRY(hipEventCreate(&P.e1));
        HIP_TRY(hipEventCreate(&P.e2));
        hipStream_t st = P.c->stream();
        HIP_TRY(hipEventRecord(P.e0, st));
        HIP_TRY(launch_trace_primary(scenes[i]->dev, C, P.F, static_cast<CgrtHitDev*>(P.dh), static_cast<float*>(P.dn), nullptr, st));
        HIP_TRY(hipEventRecord(P.e1, st));
        HIP_TRY(hipMemcpyAsync(P.ph, P.dh, P.n * sizeof(CgrtHit), hipMemcpyDeviceToHost, st));
        if (normals) HIP_TRY(hipMemcpyAsync(P.pn, P.dn, P.n * 12, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(P.e2, st));
    }
    // one host thread per replica: wait for its stream, scatter its tiles (rows of 8 pixels) into the frame
    std::vector<int> status(nscenes, CGRT_OK);
    std::vector<std::string> errs(nscenes);
    auto finish = [&](int i) {
        Part& P = part[i];
        if (P.n == 0) return;
        if (hipSetDevice(scenes[i]->device) != hipSuccess || hipStreamSynchronize(P.c->stream()) != hipSuccess) {
            status[i] = CGRT_E_HIP;
            errs[i] = "waiting for a replica's stream failed";
            return;
        }
        const CgrtHit* ph = static_cast<const CgrtHit*>(P.ph);
        const float* pn = static_cast<const float*>(P.pn);
        for (uint32_t b = 0; b < P.F.nblocks; b++)
            for (uint32_t w = 0; w < (uint32_t)P.F.block / 64u; w++) {
                int x, y;
                if (!tile_origin(P.F, b, w, x, y)) continue;
                const int cw = std::min(8, P.F.x1 - x), ch = std::min(8, P.F.y1 - y);
                const size_t base = (size_t)b * (size_t)P.F.block + w * 64u;
                for (int r = 0; r < ch; r++) {
                    std::memcpy(hits + (size_t)(y + r) * W + x, ph + base + 8 * r, (size_t)cw * sizeof(CgrtHit));
                    if (normals) {
                        // hitInfo.normal is only written for rays that hit (HitInfo stays untouched on a miss)
                        for (int c = 0; c < cw; c++)
                            if (ph[base + 8 * r + c].hit) std::memcpy(normals + 3 * ((size_t)(y + r) * W + x + c), pn + 3 * (base + 8 * r + c), 12);
                    }
                }
            }
    };
    {
        std::vector<std::thread> pool;
        for (int i = 1; i < nscenes; i++) pool.emplace_back(finish, i);
        finish(0);
        for (std::thread& t : pool) t.join();
    }
    for (int i = 0; i < nscenes; i++)
        if (status[i]) return fail(status[i], errs[i]);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->replicas = nscenes;
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        for (int i = 0; i < nscenes; i++) {
            Part& P = part[i];
            if (P.n == 0) continue;
            float k = 0, c = 0;
            (void)hipSetDevice(scenes[i]->device);
            if (hipEventElapsedTime(&k, P.e0, P.e1) == hipSuccess) stats->kernel_ms_max = std::max(stats->kernel_ms_max, k);
            if (hipEventElapsedTime(&c, P.e1, P.e2) == hipSuccess) stats->download_ms_max = std::max(stats->download_ms_max, c);
            stats->rays[i] = owned_pixels(P.F);
        }
    }
    return CGRT_OK;
}

int cgrt_render_multi(CgrtScene* const* scenes, int nscenes, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                      const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats) {
    if (!scenes || nscenes <= 0 || nscenes > 64 || !cam || !rgb) return fail(CGRT_E_ARG, "NULL argument or bad replica count");
    for (int i = 0; i < nscenes; i++) {
        if (!scenes[i]) return fail(CGRT_E_ARG, "NULL scene");
        for (int k = 0; k < i; k++)
            if (scenes[k] == scenes[i]) return fail(CGRT_E_ARG, "the same replica twice: create one scene per rank (the same device may repeat)");
    }
    if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
    return render_replicas(scenes, nscenes, cam, W, H, lights, nlights, soft, max_level, rgb, stats, false);
}

// The replicas of cgrt_render_multi_aa each shade the sub-sample super-tiles i % nscenes, resolve them on their device and download
// only their own pixels (render_impl, packed); the host threads scatter disjoint 32x32 blocks into rgb.
int cgrt_render_multi_aa(CgrtScene* const* scenes, int nscenes, const CgrtCamera* cam, int W, int H, const float* lights, uint32_t nlights,
                         const CgrtSoftShadows* soft, int max_level, float* rgb, CgrtRenderStats* stats) {
    if (!scenes || nscenes <= 0 || nscenes > 64) return fail(CGRT_E_ARG, "NULL argument or bad replica count");
    for (int i = 0; i < nscenes; i++) {
        if (!scenes[i]) return fail(CGRT_E_ARG, "NULL scene");
        for (int k = 0; k < i; k++)
            if (scenes[k] == scenes[i]) return fail(CGRT_E_ARG, "the same replica twice: create one scene per rank (the same device may repeat)");
    }
    const int rc = aa_args(cam, rgb, W, H, lights, nlights, soft, max_level, 0, nscenes);
    if (rc) return rc;
    for (int i = 0; i < nscenes; i++) NEED_DEVICE(scenes[i]);
    return render_replicas(scenes, nscenes, cam, W, H, lights, nlights, soft, max_level, rgb, stats, true);
}

}  // extern "C"
