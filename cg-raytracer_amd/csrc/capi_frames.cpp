// capi_frames.cpp -- the shaded frame's two drivers, render_impl (blocking) and enqueue_impl (without a host round trip), and what only
// they use: the frame's shape, its part of the scene's workspace, the tables of its kernels.  The C entries that build their requests
// are capi_frame_entries.cpp's.
#include "capi_internal.h"
#include "capi_frames.h"

// ------------------------------------------------------------------------------------------------
// renderRayTracing / getFinalColor (src/main.cpp:298-310, :648-720) as a device wavefront
// counted (optional, 3 blocks): the frame is rendered with the instrumented kernels (never timed) and the work of its primary,
// shadow and mirror traversals is returned separately

// Which of the wavefront's buffer sets a level's hits / normals / rays / pixels live in: level % 3, or -- a frame with geometry buffers
// that is deep enough to reuse set 0 -- level 0 in set 0 for good and levels 1.. through sets 1, 2, 3 (applied by Wavefront::level alone).
struct AovSets {
    bool keep0;
    int count() const { return keep0 ? 4 : 3; }
    int of(int level) const { return keep0 ? (level == 0 ? 0 : 1 + (level - 1) % 3) : level % 3; }
};
// The kernels' description of the caller's planes for the traced frame (W x H: aa's sub-sample frame) of F
static AovDev aov_of(const CgrtAovOut& a, const FrameDev& F, int W, int H, uint32_t nviews, int rank, int nranks) {
    AovDev A{};
    A.depth = a.depth, A.normal = a.normal, A.position = a.position, A.albedo = a.albedo;
    A.prim_id = a.prim_id, A.material_id = a.material_id, A.mask = a.mask;
    A.chw = a.chw != 0;
    A.W = W, A.H = H, A.views = (int)nviews;
    A.tiles_x = F.st_x, A.rank = rank, A.nranks = nranks;
    return A;
}
// The plan of a checked CgrtLightSets (light_sets_args): distinct slots in order of first appearance, set after set.
void cgrt::plan_light_sets(const CgrtLightSets& L, LightSetSrc& P) {
    const uint32_t B = L.nsets, np = L.light_offsets[B], ns = L.spherical_offsets ? L.spherical_offsets[B] : 0u;
    P.nsets = B;
    const size_t head = 2 * ((size_t)B + 1) + ns;
    P.point_at = (head + 3) & ~(size_t)3;
    P.sph_at = P.point_at + 8 * (size_t)np;
    P.table.assign(P.sph_at + 8 * (size_t)ns, 0u);
    for (uint32_t b = 0; b <= B; b++) {
        P.table[b] = L.light_offsets[b];
        P.table[B + 1 + b] = L.spherical_offsets ? L.spherical_offsets[b] : 0u;
    }
    std::map<std::array<uint32_t, 3>, uint32_t> pos;  // position bits -> distinct slot
    for (uint32_t k = 0; k < np; k++) {
        const float* l = L.lights + 6 * (size_t)k;
        std::array<uint32_t, 3> key;
        std::memcpy(key.data(), l, 12);
        const auto r = pos.emplace(key, (uint32_t)(P.points.size() / 6));
        if (r.second) {
            P.points.resize(P.points.size() + 6, 0.0f);
            std::memcpy(P.points.data() + P.points.size() - 6, l, 12);
        }
        uint32_t* rec = P.table.data() + P.point_at + 8 * (size_t)k;
        std::memcpy(rec, l, 12);
        rec[3] = r.first->second;
        std::memcpy(rec + 4, l + 3, 12);
    }
    std::map<std::array<uint32_t, 5>, uint32_t> sph;  // (position, radius) bits and in-set index -> distinct key
    for (uint32_t b = 0; b < B && ns; b++)
        for (uint32_t k = L.spherical_offsets[b]; k < L.spherical_offsets[b + 1]; k++) {
            const float* l = L.spherical + 7 * (size_t)k;
            std::array<uint32_t, 5> key;
            std::memcpy(key.data(), l, 16);
            key[4] = k - L.spherical_offsets[b];
            const auto r = sph.emplace(key, (uint32_t)P.sph_index.size());
            if (r.second) {
                P.sph_index.push_back(key[4]);
                P.spherical.resize(P.spherical.size() + 7, 0.0f);
                std::memcpy(P.spherical.data() + P.spherical.size() - 7, l, 16);
            }
            uint32_t* rec = P.table.data() + P.sph_at + 8 * (size_t)k;
            std::memcpy(rec, l, 12);
            rec[3] = r.first->second;
            std::memcpy(rec + 4, l + 4, 12);
        }
    std::copy(P.sph_index.begin(), P.sph_index.end(), P.table.begin() + 2 * ((size_t)B + 1));
}
// k_export_frame's description of a frame F (its PW x PH pixels in `src`) for the caller's buffer (render_impl, enqueue_impl)
static ExportDev export_of(const FrameDev& F, const float* src, const DeviceOut& dout, int PW, int PH, uint32_t nviews, bool aa, int rank, int nranks,
                           int packed) {
    ExportDev E{};
    E.src = src;
    E.dst = static_cast<unsigned char*>(dout.p);
    E.pitch = dout.pitch;
    E.W = PW;
    E.H = PH;
    E.format = dout.format;
    if (nviews) {
        E.views = (int)nviews;
        E.view_bytes = dout.view_bytes;
    }
    if (nranks > 1) {  // super-tiles of the frame, or (aa) 32x32 blocks = super-tiles of the sub-sample frame; F.st_x counts either
        E.tile = aa ? 32 : 64;
        E.tiles_x = F.st_x;
        E.rank = rank;
        E.nranks = nranks;
        E.packed = packed;
    }
    return E;
}
// The sizes that follow from a request.
struct FrameShape {
    int PW, PH;  // the frame the caller receives
    int W, H;    // the frame the wavefront shades (aa: 2 PW x 2 PH, sub-sample (xc, yc) is its pixel (xc, yc))
    int max_level;
    bool aa, list, light_sets;
    unsigned L, SL;          // point lights; spherical lights
    uint32_t nviews, nsets;  // (the frame buffer holds the views' and the sets' frames back to back)
    unsigned long long npix;
    unsigned long long n;  // items: this rank's part of the frame in the primary kernel's order, or the caller's rays
    FrameDev F;
    int packed;
    size_t res_bytes, dres_bytes;  // the resolved frame (aa), and the buffer k_resolve_aa writes it into
    size_t nctr;  // counter words: per level {shadow rays, mirror rays, hits, -}; the last block: [2], [3] = entries of levels 0, 1 / primary hits
    AovSets sets_for;
};
static int frame_shape(const FrameRequest& R, int block, FrameShape& S) {
    S.PW = R.W, S.PH = R.H;
    S.W = R.aa ? 2 * R.W : R.W, S.H = R.aa ? 2 * R.H : R.H;
    S.max_level = R.max_level;
    S.aa = R.aa, S.list = R.list != nullptr, S.light_sets = R.sets != nullptr;
    S.L = R.nlights, S.SL = R.spherical();
    S.nviews = R.views ? R.views->n : 1u;
    S.nsets = R.sets ? R.sets->nsets : 1u;
    S.npix = R.list ? R.list->n : (unsigned long long)S.W * S.H * S.nviews * S.nsets;
    S.F = FrameDev{};
    if (R.views) {
        if (!make_views_frame(S.W, S.H, S.nviews, block, S.F)) return fail(CGRT_E_ARG, "bad batch");
    } else if (!R.list && !make_frame(S.W, S.H, 0, 0, S.W, S.H, R.rank, R.nranks, block, S.F)) {
        return fail(CGRT_E_ARG, "bad frame or rank");
    }
    S.n = R.list ? R.list->n : (unsigned long long)S.F.nblocks * (unsigned long long)S.F.block;
    S.packed = R.aa && R.nranks > 1;
    S.res_bytes = S.packed ? (size_t)S.F.nst_rank * 1024 * 12 : (size_t)S.PW * S.PH * 12;
    S.dres_bytes = std::max<size_t>(S.res_bytes, (size_t)S.F.nst_rank * 1024 * 12);
    S.nctr = 4 * (size_t)(R.max_level + 1);
    S.sets_for = AovSets{R.aov && R.max_level >= 4};
    return CGRT_OK;
}
// The wavefront's part of the scene's workspace.
// Every level is a compact list: level 0 = the primary rays that hit, level l + 1 = the mirror rays of level l (at most one per entry,
// so the number of primary hits bounds every list, and n bounds that); the shadow list of a level holds at most entries * L rays.
// hits/normals/rays/pixels rotate through three sets (level l reads set l % 3 and writes its mirror rays into set (l + 1) % 3;
// level 1 is evaluated on a second stream while level 0 is still being shaded, so its mirror rays need a third set), the
// shadow lists through two.
// Geometry buffers (aov) are scattered from level 0's lists behind the frame: a frame deep enough to reuse set 0 (level 3 reads it,
// level 2 writes it) keeps level 0 in set 0 alone and rotates levels 1.. through sets 1, 2 and 3 instead.
struct Wavefront {
    const FrameShape& S;
    WsBuf rays[4], hits[4], normals[4], pix[4], ipix, srays[2], shits[2], sdist[2], sslot[2], levels, rgb, ctr, lit, resolved, sets;
    Wavefront(CgrtScene* s, const FrameShape& shape)
        : S(shape), rays{{s, WS_RAYS0}, {s, WS_RAYS1}, {s, WS_RAYS2}, {s, WS_RAYS3}}, hits{{s, WS_HITS0}, {s, WS_HITS1}, {s, WS_HITS2}, {s, WS_HITS3}},
          normals{{s, WS_NORMALS0}, {s, WS_NORMALS1}, {s, WS_NORMALS2}, {s, WS_NORMALS3}}, pix{{s, WS_PIX0}, {s, WS_PIX1}, {s, WS_PIX2}, {s, WS_PIX3}},
          ipix{s, WS_IPIX}, srays{{s, WS_SRAYS0}, {s, WS_SRAYS1}}, shits{{s, WS_SHITS0}, {s, WS_SHITS1}}, sdist{{s, WS_SDIST0}, {s, WS_SDIST1}},
          sslot{{s, WS_SSLOT0}, {s, WS_SSLOT1}}, levels{s, WS_LEVELS}, rgb{s, WS_RGB}, ctr{s, WS_CTR}, lit{s, WS_LIT}, resolved{s, WS_RESOLVED},
          sets{s, WS_SETS} {}
    // what both drivers allocate, sized for the worst case
    int reserve() {
        const unsigned long long n = S.n;
        const size_t depth = (size_t)(S.max_level > 0 ? S.max_level : 1);
        HIP_TRY(ipix.alloc(n * 4));  // pixels of level 0, kept to the end
        for (int k = 0; k < S.sets_for.count(); k++) {
            HIP_TRY(rays[k].alloc(n * 28));
            HIP_TRY(hits[k].alloc(n * sizeof(CgrtHit)));
            HIP_TRY(normals[k].alloc(n * 12));
            HIP_TRY(pix[k].alloc(n * 4));
        }
        for (int k = 0; k < 2; k++) {
            HIP_TRY(srays[k].alloc(n * S.L * 28));
            HIP_TRY(shits[k].alloc(n * S.L * sizeof(CgrtHit)));
            HIP_TRY(sdist[k].alloc(n * S.L * 4));
            HIP_TRY(sslot[k].alloc(n * S.L * 4));
        }
        HIP_TRY(levels.alloc(depth * n * 32));
        if (!S.list) HIP_TRY(rgb.alloc(S.npix * 12));  // (a ray list's colours go straight into the caller's buffer)
        if (S.aa) HIP_TRY(resolved.alloc(S.dres_bytes));
        HIP_TRY(ctr.alloc(S.nctr * sizeof(uint32_t)));
        if (S.SL) HIP_TRY(lit.alloc(n * S.SL * 4));
        // light sets: every set's colours of every level (set b's entry i of a level at b * n + i)
        if (S.light_sets) HIP_TRY(sets.alloc(depth * n * S.nsets * 16));
        return CGRT_OK;
    }
    uint32_t* ctr_of(int level) const { return ctr.as<uint32_t>() + 4 * (size_t)level; }
    float* lvl_of(int level) const { return levels.as<float>() + (size_t)level * S.n * 8; }
    float* sets_of(int level) const { return sets.p ? sets.as<float>() + (size_t)level * S.n * S.nsets * 4 : nullptr; }
    // Level l's lists, records and counters, and the next level's list: the one place that says which buffer set a level lives in.
    LevelDev level(int l) const {
        const int a = S.sets_for.of(l), b = S.sets_for.of(l + 1), q = l & 1;  // this level's buffer set, the next level's, this level's shadow set
        const bool child = l + 1 < S.max_level;
        LevelDev V{};
        V.rays = rays[a].as<float>(), V.hits = hits[a].as<CgrtHitDev>(), V.normals = normals[a].as<float>();
        V.pixels = l == 0 ? ipix.as<int>() : pix[a].as<int>();
        V.srays = srays[q].as<float>(), V.sdist = sdist[q].as<float>(), V.sslot = sslot[q].as<int>(), V.shits = shits[q].as<CgrtHitDev>();
        V.lvl = lvl_of(l), V.counters = ctr_of(l), V.sets = sets_of(l);
        V.spawn = child;
        V.next_rays = rays[b].as<float>(), V.next_hits = hits[b].as<CgrtHitDev>(), V.next_normals = normals[b].as<float>(), V.next_pixels = pix[b].as<int>();
        V.child_lvl = child ? lvl_of(l + 1) : nullptr, V.child_sets = child ? sets_of(l + 1) : nullptr;
        V.stride = S.n, V.nsets = S.nsets;
        return V;
    }
};
// The tables of a frame from where their data lies on the device: workspace slots (render_impl) or the staged table (enqueue_impl).
static SetsDev sets_dev(const LightSetSrc& P, const uint32_t* tab) {  // tab: a copy of P.table; sph_index follows the two offset rows
    SetsDev T{};
    T.point_off = tab, T.sph_off = tab + P.nsets + 1, T.nsets = P.nsets;
    T.point = reinterpret_cast<const float4*>(tab + P.point_at), T.sph = reinterpret_cast<const float4*>(tab + P.sph_at);
    return T;
}
// level 0's spawn as the primary kernel does it itself, from the registers of the lanes that hit (spawn_rays.h)
static SpawnDev spawn_dev(const LevelDev& V0, const FrameConst& K) {
    SpawnDev SP{};
    SP.materials = K.materials, SP.lights = K.lights, SP.nlights = K.nlights, SP.spawn = V0.spawn;
    SP.srays = V0.srays, SP.sdist = V0.sdist, SP.sslot = V0.sslot, SP.lvl = reinterpret_cast<float4*>(V0.lvl);
    SP.next_rays = V0.next_rays, SP.next_pixels = V0.next_pixels;
    return SP;
}
// The blocking frame.  The caller has checked the arguments (aa: aa_args).
int cgrt::render_impl(CgrtScene* s, const FrameRequest& R) {
    const ListSrc* const list = R.list;
    const ViewSrc* const views = R.views;
    const LightSetSrc* const sets = R.sets;
    const CgrtSoftShadows* const soft = R.soft;
    const DeviceOut* const dout = R.dout;
    const CgrtAovOut* const aov = R.aov;
    float* const rgb = R.rgb;
    const int max_level = R.max_level, rank = R.rank, nranks = R.nranks;
    const bool aa = R.aa, counted = R.counted != nullptr;
    if (!s || (!R.cam && !list && !views) || (!rgb && !R.mapped && !dout && !list) || (R.nlights && !R.lights)) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    if (R.W <= 0 || R.H <= 0 || max_level < 0 || max_level > 16) return fail(CGRT_E_ARG, "bad frame size or recursion depth");
    const unsigned L = R.nlights, SL = R.spherical();
    if (SL && !sets) {
        const int rc = soft_rules(soft);
        if (rc) return rc;
        if ((unsigned long long)R.W * R.H > 0x7fffffffull) return fail(CGRT_E_ARG, "frame too large");
    }
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> one_frame(s->render_mutex);  // the workspace below belongs to one frame at a time
    FrameShape S;
    if (const int rc = frame_shape(R, trace_block(s->dev), S)) return rc;
    const int W = S.W, H = S.H, PW = S.PW, PH = S.PH, packed = S.packed;
    const uint32_t nviews = S.nviews, nsets = S.nsets;
    const unsigned long long npix = S.npix, n = S.n;
    const size_t nctr = S.nctr;
    FrameDev& F = S.F;
    CgrtRenderStats st{};
    Wavefront ws(s, S);
    WsBuf dlights{s, WS_LIGHTS}, dslights{s, WS_SLIGHTS}, dunits{s, WS_UNITS}, dwork{s, WS_COUNTED}, dspawn{s, WS_SPAWN}, dviews{s, WS_VIEWS},
        dsettab{s, WS_SETTAB};  // (the blocking frame's own slots)
    unsigned long long *cw_primary = nullptr, *cw_shadow = nullptr, *cw_mirror = nullptr;
    if (counted) {
        HIP_TRY(dwork.alloc(3 * 8 * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(dwork.p, 0, 3 * 8 * sizeof(unsigned long long)));
        cw_primary = dwork.as<unsigned long long>();
        cw_shadow = cw_primary + 8;
        cw_mirror = cw_primary + 16;
    }
    // A cgrt_render_device export of an earlier frame may still be reading the frame or the resolved frame on its caller's stream: the
    // frame's streams wait for it below, and a buffer that has to grow (hipFree) is not taken from under it.
    const bool after_export = s->export_pending;
    if (after_export && ((!list && ws.rgb.cap() < npix * 12) || (aa && ws.resolved.cap() < S.dres_bytes))) HIP_TRY(hipEventSynchronize(s->export_done));
    HIP_TRY(dspawn.alloc(sizeof(SpawnDev)));
    if (const int rc = ws.reserve()) return rc;
    HIP_TRY(dlights.alloc((size_t)L * 24));
    float* const frame_rgb = list ? list->rgb : ws.rgb.as<float>();
    // (k_resolve_aa's grid covers whole 32x32 blocks; threads outside the frame write nothing)
    auto resolve = [&](hipStream_t on) { return aa ? launch_resolve_aa(F, ws.rgb.as<float>(), ws.resolved.as<float>(), packed, on) : hipSuccess; };
    if (L) HIP_TRY(hipMemcpy(dlights.p, R.lights, (size_t)L * 24, hipMemcpyHostToDevice));
    SetsDev T{};
    if (sets) {  // the sets' table (SetsDev)
        HIP_TRY(dsettab.alloc(sets->table.size() * 4));
        HIP_TRY(hipMemcpy(dsettab.p, sets->table.data(), sets->table.size() * 4, hipMemcpyHostToDevice));
        T = sets_dev(*sets, dsettab.as<uint32_t>());
    }
    SoftDev Q{};
    if (SL) {
        HIP_TRY(dslights.alloc((size_t)SL * 28));
        HIP_TRY(dunits.alloc((size_t)soft->nunits * 12));
        HIP_TRY(hipMemcpy(dslights.p, sets ? sets->spherical.data() : soft->spherical, (size_t)SL * 28, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dunits.p, soft->unit_vectors, (size_t)soft->nunits * 12, hipMemcpyHostToDevice));
        Q = soft_dev(*soft, SL, dslights.as<float>(), dunits.as<float>());
        if (sets) Q.set_index = dsettab.as<uint32_t>() + 2 * ((size_t)nsets + 1);
    }
    const CameraDev C = (list || views) ? CameraDev{} : make_camera(*R.cam);
    if (!list && !views) apply_frame_gate(s, C, F);  // (one camera: the compact primary kernel of every path below)
    if (views) {  // (the table of the VIEWS kernels; this call waits for its frame, so the slot is free again when it returns)
        const std::vector<uint8_t> tab = view_table(views->cams, views->raycams, nviews);
        HIP_TRY(dviews.alloc(tab.size()));
        HIP_TRY(hipMemcpy(dviews.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
        F.views = dviews.as<CameraDev>();  // (F.raycams: the same slot)
        Q.view_pixels = (uint32_t)W * (uint32_t)H;
    }
    const float* const mats = static_cast<const float*>(s->d_materials);
    const FrameConst K{mats, dlights.as<float>(), L, Q.lights, SL, ws.lit.as<uint32_t>(), Q.samples, frame_rgb, (unsigned long long)W * H};
    const LevelDev V0 = ws.level(0);
    CgrtScene::RenderAux& aux = s->raux;  // second stream + the events that order it against the default stream
    if (!aux.pin_counts) {
        // The second stream carries the frame's critical path (level 0's mirror list, then all of level 1), the default stream the
        // level-0 shadow list beside it.  A higher queue priority for the critical path was measured: within the noise (Cornell
        // 0.185 / 0.193 ms, dragon 0.468 / 0.455 ms with / without, profiles/r3_config3.txt); CGRT_AUX_PRIORITY=1 selects it.
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);  // (numerically lower = higher priority)
        const char* ap = getenv("CGRT_AUX_PRIORITY");
        if (ap && ap[0] == '1')
            HIP_TRY(hipStreamCreateWithPriority(&aux.s, hipStreamNonBlocking, prio_hi));
        else
            HIP_TRY(hipStreamCreateWithFlags(&aux.s, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&aux.copy, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&aux.spawned, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&aux.traced, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&aux.primary_done, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&aux.caller, hipEventDisableTiming));
        HIP_TRY(hipEventCreate(&aux.e0));
        HIP_TRY(hipEventCreate(&aux.e1));
        HIP_TRY(hipHostMalloc((void**)&aux.pin_counts, 64, hipHostMallocDefault));
    }
    if (after_export)  // (every stream of the frame, before its first write; a no-op once the export has run)
        for (hipStream_t st : {(hipStream_t) nullptr, aux.s, aux.copy}) HIP_TRY(hipStreamWaitEvent(st, s->export_done, 0));
    if (s->enq_pending)  // (the scene's enqueued frames share the workspace: every stream of this one starts behind the last of them)
        for (hipStream_t st : {(hipStream_t) nullptr, aux.s, aux.copy}) HIP_TRY(hipStreamWaitEvent(st, s->enq_done, 0));
    s->frame_seq++;
    // Geometry buffers: the miss values of every owned pixel do not depend on the frame.  They are written beside the frame's kernels (a
    // bandwidth-bound pass next to latency-bound traversals) instead of behind them: on a stream of their own, behind everything the
    // caller queued on its stream before the call, and issued right behind the primary kernel so that the frame's first launch does not
    // wait for these host calls.  Level 0's entries are scattered over them behind the frame, on the same stream, beside the colour
    // export, and the caller's stream waits for both (below).
    const AovDev A = aov ? aov_of(*aov, F, W, H, nviews, rank, nranks) : AovDev{};
    bool planes_filled = false;  // (a frame that is redrawn fills them once)
    auto fill_planes = [&]() -> int {
        if (!aov || planes_filled) return CGRT_OK;
        if (!aux.fill) {
            HIP_TRY(hipStreamCreateWithFlags(&aux.fill, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&aux.filled, hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(aux.caller, dout->stream));
        HIP_TRY(hipStreamWaitEvent(aux.fill, aux.caller, 0));
        HIP_TRY(launch_aov_fill(A, aux.fill));
        planes_filled = true;
        return CGRT_OK;
    };
    if (list) {  // the rays were written on the caller's stream: every stream of the frame starts from the default stream, which waits here
        HIP_TRY(hipEventRecord(aux.caller, list->stream));
        HIP_TRY(hipStreamWaitEvent(nullptr, aux.caller, 0));
    }
    uint32_t* const primary_hits = ws.ctr_of(max_level) + 3;
    // ---- The frame as the previous frame of this shape predicts it ----
    // An interactive renderer draws the same scene again and again (main.cpp:776-797 re-renders on every camera change), and what
    // stands between the kernels of one frame is the HOST learning list lengths: a read-back and a round trip (~25-40 us of an
    // idle GPU, profiles/r3_config3_timeline.txt) after the primary kernel, and another one per level beyond the second.  Here
    // every launch of the frame is issued at once: grids cover 1.125 x the previous frame's entries of that level + 1024, the
    // kernels stop at the counts they read on the device, and levels the previous frame did not reach are not issued.  The
    // counters come back once, behind the frame; if any list outgrew its grid, or a level that was not issued turns out to have
    // entries, the frame is drawn again the exact way below (first frames, resized frames and frames with spherical lights or
    // work counters always are).  Same kernels on the same lists: the frame is bit-identical either way (tests/test_render_prediction_gpu.py).
    bool frame_done = false;
    unsigned long long aov_entries = 0;  // level 0's entries of the frame that was kept (the geometry buffers' source)
    CgrtScene::RenderPred& P = s->rpred;
    const bool predictable = g_render_predict.load() && P.valid && P.W == W && P.H == H && P.rank == rank && P.nranks == nranks &&
                             P.max_level == max_level && P.L == L && !P.counts.empty() && SL == 0 && !counted && max_level >= 1 && !list &&
                             !views && !sets;
    auto predicted = [&]() -> int {
        const int np = (int)P.counts.size();  // levels the previous frame evaluated (P.counts[l] > 0 entries each)
        // {level 0's entries, level 1's entries}: one 64-bit word, filled by the primary kernel's fused spawn with one atomic
        uint32_t* const pair = ws.ctr_of(max_level) + 2;
        auto count_of = [&](int level) { return level <= 1 ? pair + level : ws.ctr_of(level - 1) + 1; };  // device word: entries of the level
        auto cap_of = [&](int level) { return std::min<unsigned long long>(n, (unsigned long long)P.counts[level] + P.counts[level] / 8 + 1024); };
        HIP_TRY(hipEventRecord(aux.e0, nullptr));
        HIP_TRY(hipMemsetAsync(ws.ctr.p, 0, nctr * sizeof(uint32_t), nullptr));
        // (level 0's spawn is done by the primary kernel itself, from the registers of the lanes that hit: spawn_rays.h)
        const SpawnDev SP = spawn_dev(V0, K);
        if (!aux.spawn_valid || std::memcmp(&SP, &aux.spawn_host, sizeof(SP)) != 0) {  // (the workspace keeps its addresses from frame to frame)
            HIP_TRY(hipMemcpy(dspawn.p, &SP, sizeof(SP), hipMemcpyHostToDevice));
            aux.spawn_host = SP;
            aux.spawn_valid = true;
        }
        HIP_TRY(launch_trace_primary_compact(s->dev, C, F, V0.rays, V0.hits, V0.normals, V0.pixels, pair, nullptr, nullptr, K.rgb,
                                             static_cast<const SpawnDev*>(dspawn.p)));
        if (const int frc = fill_planes()) return frc;
        const unsigned long long cap0 = cap_of(0);
        // Level 0's two lists.  With a fast tree they go out as ONE launch (k_trace_pair: workgroups dealt alternately) and the whole
        // frame stays on one stream; otherwise the shadow list runs on the default stream and the mirror list, with all of level 1
        // behind it, on the second one.
        const bool paired = np >= 2 && L > 0 && can_trace_pair(s->dev);
        hipStream_t const side = paired ? nullptr : aux.s;  // where level 1 is evaluated
        bool tail_on_aux = false;
        const LevelDev V1 = ws.level(1);
        if (paired) {
            HIP_TRY(launch_trace_pair(s->dev, V0.shadow_list(cap0 * L, pair, L, (unsigned long long)P.counts[0] * L), V0.mirror_list(cap_of(1), pair + 1, P.counts[1]),
                                      nullptr));
        } else {
            HIP_TRY(hipEventRecord(aux.spawned, nullptr));
            if (L)  // (hits x lights rays)
                HIP_TRY(launch_trace_shadow(s->dev, V0.shadow_list(cap0 * L, pair, L, (unsigned long long)P.counts[0] * L), nullptr, nullptr));
        }
        if (np >= 2) {  // level 1 (and, unpaired, level 0's mirror list in front of it)
            const unsigned long long cap1 = cap_of(1);
            if (!paired) {
                HIP_TRY(hipStreamWaitEvent(aux.s, aux.spawned, 0));
                HIP_TRY(launch_trace_batch(s->dev, V0.mirror_list(cap1, pair + 1, P.counts[1]), nullptr, aux.s));
            }
            HIP_TRY(launch_spawn(V1, K, cap1, side, pair + 1));
            if (L)
                HIP_TRY(launch_trace_shadow(s->dev, V1.shadow_list(cap1 * L, V1.counters + 0, 1, (unsigned long long)P.counts[1] * L), nullptr, side));
            HIP_TRY(launch_shade(V1, K, cap1, side, pair + 1));
            if (np >= 3)
                HIP_TRY(launch_trace_batch(s->dev, V1.mirror_list(cap_of(2), V1.counters + 1, P.counts[2]), nullptr, side));
            if (!paired) HIP_TRY(hipEventRecord(aux.traced, aux.s));
        }
        HIP_TRY(launch_shade(V0, K, cap0, nullptr, pair));
        if (!paired) {
            // Two levels (the reference's depth, and most frames at any depth): the frame's last kernels are on the second stream, so
            // the scatter into the frame goes there too, behind level 0's shading -- which finished long before -- instead of the
            // default stream waiting for the second one (a cross-stream wait in front of the last kernel cost ~10 us of idle GPU).
            tail_on_aux = np == 2;
            if (tail_on_aux) {
                HIP_TRY(hipEventRecord(aux.primary_done, nullptr));  // (reused: level 0 is shaded)
                HIP_TRY(hipStreamWaitEvent(aux.s, aux.primary_done, 0));
            } else if (np >= 2) {
                HIP_TRY(hipStreamWaitEvent(nullptr, aux.traced, 0));
            }
        }
        hipStream_t const tail = tail_on_aux ? aux.s : nullptr;
        for (int level = 2; level < np; level++) {  // deeper levels: small, one after the other (buffer sets as in the exact path)
            const LevelDev V = ws.level(level);
            const unsigned long long cap = cap_of(level);
            HIP_TRY(launch_spawn(V, K, cap, nullptr, count_of(level)));
            if (L)
                HIP_TRY(launch_trace_shadow(s->dev, V.shadow_list(cap * L, V.counters + 0, 1, (unsigned long long)P.counts[level] * L), nullptr, nullptr));
            HIP_TRY(launch_shade(V, K, cap, nullptr, count_of(level)));
            if (level + 1 < np)
                HIP_TRY(launch_trace_batch(s->dev, V.mirror_list(cap_of(level + 1), V.counters + 1, P.counts[level + 1]), nullptr, nullptr));
        }
        for (int level = np - 2; level >= 1; level--) HIP_TRY(launch_fold(ws.level(level), cap_of(level), nullptr, count_of(level)));
        HIP_TRY(launch_write_rgb(V0, K, np >= 2, cap0, tail, pair));
        HIP_TRY(resolve(tail));
        HIP_TRY(hipEventRecord(aux.e1, tail));
        HIP_TRY(hipEventSynchronize(aux.e1));
        std::vector<uint32_t> hc(nctr);
        HIP_TRY(hipMemcpy(hc.data(), ws.ctr.p, nctr * sizeof(uint32_t), hipMemcpyDeviceToHost));  // (waits for the frame)
        // ---- did every list fit its grid, and did the frame end where it was expected to? ----
        std::vector<uint32_t> actual;  // entries per level, levels with entries only
        bool fits = true;
        for (int level = 0; level < max_level; level++) {
            const uint32_t cnt = level <= 1 ? hc[4 * (size_t)max_level + 2 + level] : hc[4 * (size_t)(level - 1) + 1];
            if (level < np) {
                fits = fits && cnt <= cap_of(level);
            } else {
                fits = fits && cnt == 0;  // a level that was not issued has entries
            }
            if (cnt == 0 || !fits) break;
            actual.push_back(cnt);
        }
        if (!fits) {
            P.valid = false;
            return CGRT_OK;  // (frame_done stays false: the exact path draws the frame)
        }
        st.primary_rays = owned_pixels(F);
        // (level 0's counter block is not used by the fused spawn; a frame without primary hits has no level at all: it is black,
        // the primary kernel cleared its pixels)
        st.shadow_rays = actual.empty() ? 0 : (uint64_t)actual[0] * L;
        st.reflection_rays = hc[4 * (size_t)max_level + 3];
        for (size_t level = 1; level < actual.size(); level++) {
            st.shadow_rays += hc[4 * level + 0];
            st.reflection_rays += hc[4 * level + 1];
        }
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, aux.e0, aux.e1));
        st.device_ms = ms;
        st.levels = (int)actual.size();
        aov_entries = actual.empty() ? 0 : actual[0];
        P.counts = actual;
        P.valid = !actual.empty();
        P.last_path = 1;
        frame_done = true;
        return CGRT_OK;
    };
    if (predictable) {
        const int prc = predicted();
        if (prc != CGRT_OK) return prc;
    }
    // A level's shading (k_shade into its level record; light sets: k_shade_sets into every set's colours of the level) and the scatter of
    // level 0 into the frame (k_write_rgb, folded with level 1 when with_child; light sets: k_write_rgb_sets, every set into its own frame).
    auto shade = [&](const LevelDev& V, unsigned long long cnt, hipStream_t on, const uint32_t* dc) -> hipError_t {
        return sets ? launch_shade_sets(V, K, T, cnt, on, dc) : launch_shade(V, K, cnt, on, dc);
    };
    auto write_rgb = [&](bool with_child, unsigned long long cnt) -> hipError_t {
        if (sets) return launch_write_rgb_sets(V0, K, views != nullptr, with_child, cnt, nullptr);  // (views: frame (view, set) at view * nsets + set)
        return launch_write_rgb(V0, K, with_child, cnt, nullptr);
    };
    auto exact = [&]() -> int {
        HIP_TRY(hipEventRecord(aux.e0, nullptr));
        int nlev = 0;
        bool finished = false;  // the frame's last kernels and its closing event have been issued inside the level loop
        std::vector<unsigned long long> level_count;  // entries per evaluated level
        HIP_TRY(hipMemsetAsync(ws.ctr.p, 0, nctr * sizeof(uint32_t), nullptr));
        if (max_level >= 1) {  // trace(level 0): main.cpp:267 returns black without tracing when level >= maxLevel
            // level 0 = the primary rays that hit something, straight out of the fused primary kernel (pixels that miss are
            // black, main.cpp:293, and spawn nothing)
            if (list) {  // (also clears the list's colours)
                HIP_TRY(launch_trace_list_compact(s->dev, list->rays, n, V0.rays, V0.hits, V0.normals, V0.pixels, primary_hits, frame_rgb, nullptr, cw_primary));
                st.primary_rays = n;
            } else if (views) {  // (also clears every view's pixels)
                HIP_TRY(launch_trace_primary_views_compact(s->dev, F, V0.rays, V0.hits, V0.normals, V0.pixels, primary_hits, frame_rgb, nullptr,
                                                           views->raycams != nullptr));
                st.primary_rays = (unsigned long long)W * H * nviews;
            } else {  // (also clears this rank's pixels)
                HIP_TRY(launch_trace_primary_compact(s->dev, C, F, V0.rays, V0.hits, V0.normals, V0.pixels, primary_hits, nullptr, cw_primary, frame_rgb));
                st.primary_rays = owned_pixels(F);
            }
            if (const int frc = fill_planes()) return frc;
            // (light sets: the primary kernel clears the first nviews * W * H pixels of the frame buffer; the sets' scatter writes only the
            // pixels that hit, and a pixel that misses is black in every set: the rest of the buffer is cleared here)
            if (nsets > 1)
                HIP_TRY(hipMemsetAsync(frame_rgb + 3ull * W * H * nviews, 0, (npix - (unsigned long long)W * H * nviews) * 12, nullptr));
            // Level 0's spawn does not wait for the host to learn how many primary rays hit: it is launched over every item of the
            // rank's frame and stops at the count it reads on the device, while the host fetches that count on a stream of its own
            // (behind the primary kernel only) to size the traversal launches that follow -- the host round trip (~25 us of an idle
            // GPU per frame, profiles/r3_config3_timeline.txt) now overlaps the spawn kernel.
            HIP_TRY(hipEventRecord(aux.primary_done, nullptr));
            HIP_TRY(launch_spawn(V0, K, n, nullptr, primary_hits));
            // (Issuing level 0's shadow list here too, over its capacity n * L, was measured: Cornell 0.182 -> 0.179 ms, but the dragon
            // frame 0.46 -> 0.50 ms -- a grid of 32 K workgroups for 318 K rays costs more than the round trip it saves.  It is sized
            // exactly after the read-back, and issued FIRST: it used to start 64 us after the spawn kernel ended, behind the second
            // stream's five launches, profiles/r3_config3_timeline.txt.)
            HIP_TRY(hipEventRecord(aux.spawned, nullptr));
            HIP_TRY(hipStreamWaitEvent(aux.copy, aux.primary_done, 0));
            HIP_TRY(hipMemcpyAsync(aux.pin_counts, primary_hits, sizeof(uint32_t), hipMemcpyDeviceToHost, aux.copy));
            HIP_TRY(hipStreamSynchronize(aux.copy));
            unsigned long long cnt = aux.pin_counts[0];
            aov_entries = cnt;
            int level = 0;
            while (level < max_level && cnt > 0) {
                const LevelDev V = ws.level(level);
                const int spawn = V.spawn;
                uint32_t* const ctr = V.counters;
                if (level > 0) HIP_TRY(launch_spawn(V, K, cnt, nullptr));  // (level 0's spawn is already in flight, see above)
                // Level 0's mirror batch runs on the second stream, beside level 0's shadow batch (two batches of a few hundred
                // thousand rays each; its grid covers the list's capacity -- one mirror ray per entry -- and the kernel stops at the
                // appended count).  Without spherical lights the whole of level 1 follows it there -- spawn, shadow list, shading,
                // level 2's mirror batch: none of it needs level 0's shading, all of it is sized by counts on the device -- so that
                // level 1's tail overlaps level 0's.  Deeper levels are small and often empty: they run one after the other,
                // exactly sized after each level's read-back, or not at all.
                // the level's shadow list first: the long pole of the default stream must not wait behind the second stream's launches
                if (L) HIP_TRY(launch_trace_shadow(s->dev, V.shadow_list(cnt * L, ctr + 0), cw_shadow, nullptr));
                const bool overlap = spawn && level == 0;
                const bool pipelined = overlap && SL == 0;
                const int spawn1 = 2 < max_level;
                if (overlap) {  // (level 0: aux.spawned was recorded right behind the spawn kernel)
                    HIP_TRY(hipStreamWaitEvent(aux.s, aux.spawned, 0));
                    HIP_TRY(launch_trace_batch(s->dev, V.mirror_list(cnt, ctr + 1), cw_mirror, aux.s));
                    if (pipelined) {
                        const LevelDev V1 = ws.level(1);
                        HIP_TRY(launch_spawn(V1, K, cnt, aux.s, ctr + 1));
                        if (L) HIP_TRY(launch_trace_shadow(s->dev, V1.shadow_list(cnt * L, V1.counters + 0), cw_shadow, aux.s));
                        HIP_TRY(shade(V1, cnt, aux.s, ctr + 1));
                        if (spawn1)
                            HIP_TRY(launch_trace_batch(s->dev, V1.mirror_list(cnt, V1.counters + 1), cw_mirror, aux.s));
                    }
                    HIP_TRY(hipEventRecord(aux.traced, aux.s));
                }
                if (SL) {
                    Q.level = (uint32_t)level;
                    HIP_TRY(hipMemsetAsync(ws.lit.p, 0, cnt * SL * 4, nullptr));
                    HIP_TRY(launch_soft_shadow(s->dev, Q, V.rays, V.hits, V.pixels, cnt, ws.lit.as<uint32_t>(), soft->closest_hit == 0, nullptr));
                }
                HIP_TRY(shade(V, cnt, nullptr, nullptr));
                if (overlap) HIP_TRY(hipStreamWaitEvent(nullptr, aux.traced, 0));  // the next level (and the end of the frame) need the second stream's results
                nlev = level + 1;
                level_count.push_back(cnt);
                if (pipelined && !spawn1) {
                    // Depth 2 (the reference's own depth, main.cpp:267): both levels are in flight or done and nothing further depends
                    // on their counts -- the frame is finished without a host round trip (an entry of level 0 without a mirror ray
                    // carries child = -1, so the scatter kernel can fold with level 1 whether or not level 1 has entries); the
                    // counts are read after the frame's closing event.
                    HIP_TRY(write_rgb(true, cnt));
                    HIP_TRY(resolve(nullptr));
                    finished = true;
                    HIP_TRY(hipEventRecord(aux.e1, nullptr));
                    uint32_t h2[8];
                    HIP_TRY(hipMemcpy(h2, ctr, sizeof(h2), hipMemcpyDeviceToHost));  // levels 0 and 1, adjacent
                    st.shadow_rays += (uint64_t)h2[0] + h2[4];
                    st.reflection_rays += (uint64_t)h2[1] + h2[5];
                    if (h2[1] > 0) {
                        nlev = 2;
                        level_count.push_back(h2[1]);
                    }
                    break;
                }
                uint32_t h[8];
                HIP_TRY(hipMemcpy(h, ctr, pipelined ? sizeof(h) : sizeof(h) / 2, hipMemcpyDeviceToHost));  // also the level's sync point (pipelined: levels 0 and 1, adjacent)
                st.shadow_rays += h[0];
                st.reflection_rays += h[1];
                st.soft_shadow_rays += (uint64_t)h[2] * SL * Q.samples;
                if (!spawn || h[1] == 0) break;
                if (pipelined) {  // level 1 has been evaluated on the second stream, and level 2's rays traversed
                    const uint32_t* h1 = h + 4;
                    nlev = 2;
                    level_count.push_back(h[1]);
                    st.shadow_rays += h1[0];
                    st.reflection_rays += h1[1];
                    if (!spawn1 || h1[1] == 0) break;
                    cnt = h1[1];
                    level = 2;
                    continue;
                }
                if (!overlap) HIP_TRY(launch_trace_batch(s->dev, V.mirror_list(h[1], nullptr), cw_mirror, nullptr));
                cnt = h[1];
                level += 1;
            }
        }
        if (finished) {
        } else if (max_level < 1) {  // trace() returns black without tracing (main.cpp:267): no primary kernel ran, clear here
            if (list || views || sets)
                HIP_TRY(hipMemsetAsync(frame_rgb, 0, npix * 12, nullptr));
            else
                HIP_TRY(launch_clear_owned(F, frame_rgb, nullptr));
        } else if (nlev == 0) {  // nothing was hit: the primary kernel has left this rank's pixels black
        } else {
            // color = directColor + reflectedColor * ks (main.cpp:262), deepest level first; the last fold (level 0 with level 1) is
            // done by the kernel that scatters level 0 over the frame
            for (int level = nlev - 2; level >= 1; level--) {
                const LevelDev V = ws.level(level);
                HIP_TRY(sets ? launch_fold_sets(V, level_count[level], nullptr) : launch_fold(V, level_count[level], nullptr));
            }
            HIP_TRY(write_rgb(nlev >= 2, level_count[0]));
        }
        if (!finished) {
            HIP_TRY(resolve(nullptr));
            HIP_TRY(hipEventRecord(aux.e1, nullptr));
        }
        HIP_TRY(hipEventSynchronize(aux.e1));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, aux.e0, aux.e1));
        st.device_ms = ms;
        st.levels = nlev;
        if (list || views || sets) return CGRT_OK;  // (a ray list or a batch of views or light sets sizes no frame)
        // what this frame found sizes the next one
        P.valid = g_render_predict.load() && SL == 0 && !counted && max_level >= 1 && !level_count.empty();
        P.W = W, P.H = H, P.rank = rank, P.nranks = nranks, P.max_level = max_level, P.L = L;
        P.counts.clear();
        for (unsigned long long c : level_count) P.counts.push_back((uint32_t)c);
        return CGRT_OK;
    };
    if (!frame_done) {
        if (!list && !views && !sets) P.last_path = predictable ? 2 : 0;
        st = CgrtRenderStats{};
        const int erc = exact();
        if (erc != CGRT_OK) return erc;
    }
    if (after_export) s->export_pending = false;  // aux.e1, which this call has waited for, is behind it
    if (list) {
        // The colours are in the caller's buffer and the frame's last kernel is done (aux.e1 was waited for); the wait only makes that
        // ordering explicit on the caller's stream.
        HIP_TRY(hipStreamWaitEvent(list->stream, aux.e1, 0));
    } else if (dout) {
        // The frame's last kernel is done (aux.e1 was waited for); the wait below only makes that ordering explicit on the caller's stream.
        const ExportDev E = export_of(F, aa ? ws.resolved.as<float>() : ws.rgb.as<float>(), *dout, PW, PH, (views || sets) ? nviews * nsets : 0u, aa, rank,
                                      nranks, packed);
        if (!s->export_done) HIP_TRY(hipEventCreateWithFlags(&s->export_done, hipEventDisableTiming));
        HIP_TRY(hipStreamWaitEvent(dout->stream, aux.e1, 0));
        if (aov) {  // (level 0 of the frame that was kept is in set 0, untouched since its primary kernel; aux.e1 has been waited for)
            HIP_TRY(launch_aov_scatter(A, V0, mats, aov_entries, aux.fill));
            HIP_TRY(hipEventRecord(aux.filled, aux.fill));
        }
        HIP_TRY(launch_export_frame(E, dout->stream));
        if (aov) HIP_TRY(hipStreamWaitEvent(dout->stream, aux.filled, 0));  // (export_done, below, is behind the planes too)
        HIP_TRY(hipEventRecord(s->export_done, dout->stream));
        s->export_pending = true;
    } else {
        const size_t bytes = aa ? S.res_bytes : (size_t)npix * 12;
        if (s->pin_frame_cap < bytes) {
            if (s->pin_frame) (void)hipHostFree(s->pin_frame);
            s->pin_frame = nullptr;
            s->pin_frame_cap = 0;
            HIP_TRY(hipHostMalloc(&s->pin_frame, bytes, hipHostMallocDefault));
            s->pin_frame_cap = bytes;
        }
        HIP_TRY(hipMemcpyAsync(s->pin_frame, aa ? ws.resolved.p : ws.rgb.p, bytes, hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        const float* pin = static_cast<const float*>(s->pin_frame);
        if (R.mapped) *R.mapped = pin;
        if (rgb && nranks == 1) {
            parallel_copy(rgb, pin, bytes);
        } else if (rgb && aa) {  // this rank's 32x32 pixel blocks, packed by k_resolve_aa
            for (uint64_t sl = 0; sl < F.nst_rank; sl++) {
                const uint64_t k = (uint64_t)rank + (uint64_t)nranks * sl;
                const int sx = (int)(k % (uint64_t)F.st_x) * 32, sy = (int)(k / (uint64_t)F.st_x) * 32;
                const int w = std::min(32, PW - sx), h = std::min(32, PH - sy);
                for (int r = 0; r < h; r++) std::memcpy(rgb + 3 * ((size_t)(sy + r) * PW + sx), pin + 3 * (sl * 1024 + 32 * (uint64_t)r), (size_t)w * 12);
            }
        } else if (rgb) {  // this rank's super-tiles only (the ownership rule of cgrt_trace_primary)
            const uint64_t nst = (uint64_t)F.st_x * (uint64_t)F.st_y;
            for (uint64_t k = (uint64_t)rank; k < nst; k += (uint64_t)nranks) {
                const int sx = (int)(k % (uint64_t)F.st_x) * 64, sy = (int)(k / (uint64_t)F.st_x) * 64;
                const int w = std::min(64, W - sx), h = std::min(64, H - sy);
                for (int r = 0; r < h; r++) std::memcpy(rgb + 3 * ((size_t)(sy + r) * W + sx), pin + 3 * ((size_t)(sy + r) * W + sx), (size_t)w * 12);
            }
        }
    }
    if (counted) {
        unsigned long long h[24];
        HIP_TRY(hipMemcpy(h, dwork.p, sizeof(h), hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; k++) {
            const unsigned long long* q = h + 8 * k;
            R.counted[k] = CgrtCounters{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
        }
    }
    if (R.stats) *R.stats = st;
    return CGRT_OK;
}

// ---- enqueued frames (include/cgrt.h cgrt_enqueue_*) ----
// The frame of render_impl's exact path, issued without a host round trip: every list is sized for the worst case (as render_impl
// sizes the workspace anyway), all max_level levels are issued, and every launch after the primary kernel is a capped, count-driven grid
// (GRID_STRIDED) that reads its list's length on the device.  A single camera's level 0 is spawned by the primary kernel
// itself (the predicted frame's fused spawn); views and ray lists run their own primary kernels and a count-driven spawn.  The whole
// frame, export included, is on the caller's stream, behind the scene's previous frames (enq_done, export_done), and nothing is waited
// for on the host unless the workspace grows or every ticket slot is in flight.  Same kernels' expressions on the same entries, each
// scattered back by its pixel: the bytes are the blocking entry's.  The caller has checked the arguments (the blocking entries' checks).
int cgrt::enqueue_impl(CgrtScene* s, const FrameRequest& R) {
    const ListSrc* const list = R.list;
    const ViewSrc* const views = R.views;
    const LightSetSrc* const sets = R.sets;  // (light sets: always with views; frame (view, set) is frame view * nsets + set)
    const CgrtSoftShadows* const soft = R.soft;
    const int max_level = R.max_level;
    hipStream_t const stream = R.stream;
    HIP_TRY(hipSetDevice(s->device));
    std::lock_guard<std::mutex> one_frame(s->render_mutex);
    FrameShape S;
    if (const int rc = frame_shape(R, trace_block(s->dev), S)) return rc;
    const int W = S.W, H = S.H;
    const uint32_t nviews = S.nviews, nsets = S.nsets;
    const unsigned long long npix = S.npix, n = S.n;
    const unsigned L = S.L, SL = S.SL;
    FrameDev& F = S.F;
    // the ticket slot: its last frame must be over before its staging is written again (the documented wait)
    CgrtScene::EnqSlot& slot = s->eslot[s->enq_count % CgrtScene::ENQ_SLOTS];
    if (slot.pending) {
        HIP_TRY(hipEventSynchronize(slot.done));
        slot.pending = false;
    }
    if (!slot.done) {
        HIP_TRY(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
        HIP_TRY(hipEventCreate(&slot.t0));
        HIP_TRY(hipEventCreate(&slot.t1));
        HIP_TRY(hipHostMalloc((void**)&slot.pin_ctr, 4 * 17 * sizeof(uint32_t), hipHostMallocDefault));
    }
    // the workspace of render_impl, sized for the worst case (WsBuf::alloc waits for the scene's frames before a buffer grows)
    Wavefront ws(s, S);
    if (n)
        if (const int rc = ws.reserve()) return rc;
    // the frame's tables, through the slot's pinned staging: the caller may reuse its arrays once the call returns (light sets: `lights` is
    // the distinct positions, the spherical lights the distinct keys, and the sets' own table -- SetsDev's memory -- comes last)
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_lights = 0, o_slights = up16((size_t)L * 24), o_units = o_slights + up16((size_t)SL * 28),
                 o_spawn = o_units + up16(SL ? (size_t)soft->nunits * 12 : 0), o_views = o_spawn + up16(sizeof(SpawnDev)),
                 o_sets = o_views + up16(views ? views->table_bytes() : 0),
                 table_bytes = o_sets + (sets ? sets->table.size() * 4 : 0);
    if (slot.cap < table_bytes) {
        if (slot.pin) (void)hipHostFree(slot.pin);
        slot.pin = nullptr;
        slot.cap = 0;
        HIP_TRY(hipHostMalloc(&slot.pin, table_bytes, hipHostMallocDefault));
        slot.cap = table_bytes;
    }
    if (s->enq_dev_cap < table_bytes) {
        if (s->enq_dev && s->enq_pending) HIP_TRY(hipEventSynchronize(s->enq_done));  // (the frames in flight read it)
        if (s->enq_dev) (void)hipFree(s->enq_dev);
        s->enq_dev = nullptr;
        s->enq_dev_cap = 0;
        HIP_TRY(hipMalloc(&s->enq_dev, table_bytes));
        s->enq_dev_cap = table_bytes;
    }
    char* const pin = static_cast<char*>(slot.pin);
    char* const tab = static_cast<char*>(s->enq_dev);
    if (L) std::memcpy(pin + o_lights, R.lights, (size_t)L * 24);
    SoftDev Q{};
    SetsDev T{};
    if (SL) {
        std::memcpy(pin + o_slights, sets ? sets->spherical.data() : soft->spherical, (size_t)SL * 28);
        std::memcpy(pin + o_units, soft->unit_vectors, (size_t)soft->nunits * 12);
        Q = soft_dev(*soft, SL, reinterpret_cast<const float*>(tab + o_slights), reinterpret_cast<const float*>(tab + o_units));
        if (views) Q.view_pixels = (uint32_t)W * (uint32_t)H;
    }
    if (sets) {
        std::memcpy(pin + o_sets, sets->table.data(), sets->table.size() * 4);
        T = sets_dev(*sets, reinterpret_cast<const uint32_t*>(tab + o_sets));
        Q.set_index = T.point_off + 2 * ((size_t)nsets + 1);
    }
    float* const frame_rgb = list ? list->rgb : ws.rgb.as<float>();
    const float* const mats = static_cast<const float*>(s->d_materials);
    const FrameConst K{mats, reinterpret_cast<const float*>(tab + o_lights), L, Q.lights, SL, ws.lit.as<uint32_t>(), Q.samples, frame_rgb,
                       (unsigned long long)W * H};
    const bool fused = !list && !views;  // level 0 spawned by the primary kernel (spawn_rays.h)
    uint32_t* const pair = ws.ctr_of(max_level) + 2;  // fused: {level 0's entries, level 1's entries}
    uint32_t* const primary_hits = pair + 1;          // views, lists: level 0's entries
    if (fused && max_level >= 1) {
        const SpawnDev SP = spawn_dev(ws.level(0), K);
        std::memcpy(pin + o_spawn, &SP, sizeof(SP));
    }
    if (views) {
        const std::vector<uint8_t> vt = view_table(views->cams, views->raycams, nviews);
        std::memcpy(pin + o_views, vt.data(), vt.size());
        F.views = reinterpret_cast<CameraDev*>(tab + o_views);  // (F.raycams: the same slot)
    }
    // ---- the frame, on the caller's stream ----
    if (s->enq_pending) HIP_TRY(hipStreamWaitEvent(stream, s->enq_done, 0));
    if (s->export_pending) HIP_TRY(hipStreamWaitEvent(stream, s->export_done, 0));
    HIP_TRY(hipEventRecord(slot.t0, stream));
    HIP_TRY(hipMemcpyAsync(tab, pin, table_bytes, hipMemcpyHostToDevice, stream));
    if (n) {
        const LevelDev V0 = ws.level(0);
        HIP_TRY(hipMemsetAsync(ws.ctr.p, 0, S.nctr * sizeof(uint32_t), stream));
        if (max_level < 1) {  // trace() returns black without tracing (main.cpp:267)
            if (list || views)
                HIP_TRY(hipMemsetAsync(frame_rgb, 0, npix * 12, stream));
            else
                HIP_TRY(launch_clear_owned(F, frame_rgb, stream));
        } else {
            // device word with the entries of a level / the mirror rays a level spawned
            auto count_of = [&](int level) -> uint32_t* {
                if (level == 0) return fused ? pair : primary_hits;
                return (fused && level == 1) ? pair + 1 : ws.ctr_of(level - 1) + 1;
            };
            auto mirrors_of = [&](int level) -> uint32_t* { return (fused && level == 0) ? pair + 1 : ws.ctr_of(level) + 1; };
            if (list)  // (also clears the list's colours)
                HIP_TRY(launch_trace_list_compact(s->dev, list->rays, n, V0.rays, V0.hits, V0.normals, V0.pixels, primary_hits, frame_rgb, stream));
            else if (views)  // (also clears every view's pixels)
                HIP_TRY(launch_trace_primary_views_compact(s->dev, F, V0.rays, V0.hits, V0.normals, V0.pixels, primary_hits, frame_rgb, stream,
                                                           views->raycams != nullptr));
            else {  // (also clears this rank's pixels, and spawns level 0)
                const CameraDev C = make_camera(*R.cam);
                apply_frame_gate(s, C, F);
                HIP_TRY(launch_trace_primary_compact(s->dev, C, F, V0.rays, V0.hits, V0.normals, V0.pixels, pair, stream, nullptr,
                                                     frame_rgb, reinterpret_cast<const SpawnDev*>(tab + o_spawn)));
            }
            if (nsets > 1)  // (as render_impl: the views' kernel cleared the first nviews * W * H pixels, a miss is black in every set)
                HIP_TRY(hipMemsetAsync(frame_rgb + 3ull * W * H * nviews, 0, (npix - (unsigned long long)W * H * nviews) * 12, stream));
            const bool pairable = can_trace_pair(s->dev);
            for (int level = 0; level < max_level; level++) {
                const LevelDev V = ws.level(level);
                const bool fused0 = fused && level == 0;
                if (!fused0) HIP_TRY(launch_spawn(V, K, n, stream, count_of(level), GRID_STRIDED));
                // the level's shadow list: hits x lights rays (fused level 0) or the appended count
                const uint32_t* sdc = fused0 ? pair : V.counters;
                const unsigned sdmul = fused0 ? L : 1u;
                if (L && V.spawn && pairable) {
                    HIP_TRY(launch_trace_pair(s->dev, V.shadow_list(n * L, sdc, sdmul), V.mirror_list(n, mirrors_of(level)), stream, GRID_STRIDED));
                } else {
                    if (L) HIP_TRY(launch_trace_shadow(s->dev, V.shadow_list(n * L, sdc, sdmul), nullptr, stream, GRID_STRIDED));
                    if (V.spawn) HIP_TRY(launch_trace_batch(s->dev, V.mirror_list(n, mirrors_of(level)), nullptr, stream, GRID_STRIDED));
                }
                if (SL) {
                    Q.level = (uint32_t)level;
                    HIP_TRY(hipMemsetAsync(ws.lit.p, 0, n * SL * 4, stream));
                    HIP_TRY(launch_soft_shadow(s->dev, Q, V.rays, V.hits, V.pixels, n, ws.lit.as<uint32_t>(), soft->closest_hit == 0, stream, count_of(level),
                                               GRID_STRIDED));
                }
                if (sets)
                    HIP_TRY(launch_shade_sets(V, K, T, n, stream, count_of(level), GRID_STRIDED));
                else
                    HIP_TRY(launch_shade(V, K, n, stream, count_of(level), GRID_STRIDED));
            }
            for (int level = max_level - 2; level >= 1; level--) {
                const LevelDev V = ws.level(level);
                HIP_TRY(sets ? launch_fold_sets(V, n, stream, count_of(level), GRID_STRIDED) : launch_fold(V, n, stream, count_of(level), GRID_STRIDED));
            }
            if (sets)  // (an enqueued batch of sets is a multi-view one)
                HIP_TRY(launch_write_rgb_sets(V0, K, true, max_level >= 2, n, stream, count_of(0), GRID_STRIDED));
            else
                HIP_TRY(launch_write_rgb(V0, K, max_level >= 2, n, stream, count_of(0), GRID_STRIDED));
        }
        if (R.aa) HIP_TRY(launch_resolve_aa(F, ws.rgb.as<float>(), ws.resolved.as<float>(), S.packed, stream));
        if (R.dout)
            HIP_TRY(launch_export_frame(export_of(F, R.aa ? ws.resolved.as<float>() : ws.rgb.as<float>(), *R.dout, S.PW, S.PH, views ? nviews * nsets : 0u,
                                                  R.aa, R.rank, R.nranks, S.packed), stream));
        if (R.aov) {  // (max_level >= 1: level 0's length is the word the primary kernel counted into)
            const AovDev A = aov_of(*R.aov, F, W, H, nviews, R.rank, R.nranks);
            HIP_TRY(launch_aov_fill(A, stream));
            HIP_TRY(launch_aov_scatter(A, V0, mats, n, stream, fused ? pair : primary_hits, GRID_STRIDED));
        }
        HIP_TRY(hipMemcpyAsync(slot.pin_ctr, ws.ctr.p, S.nctr * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipEventRecord(slot.t1, stream));
    HIP_TRY(hipEventRecord(slot.done, stream));
    s->enq_done = slot.done;
    s->enq_pending = true;
    s->enq_count++;
    slot.pending = true;
    slot.ticket = ++s->frame_seq;
    slot.max_level = n ? max_level : 0;
    slot.fused = fused;
    slot.L = L;
    slot.SL = SL;
    slot.samples = SL ? soft->samples : 0;
    slot.primary_rays = (n && max_level >= 1) ? (list ? n : views ? (unsigned long long)W * H * nviews : owned_pixels(F)) : 0;
    if (R.ticket) *R.ticket = slot.ticket;
    return CGRT_OK;
}

extern "C" {

int cgrt_enqueue_stats(CgrtScene* s, uint64_t ticket, CgrtRenderStats* stats) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    hipEvent_t done = nullptr;
    {
        std::lock_guard<std::mutex> lk(s->render_mutex);
        for (const CgrtScene::EnqSlot& e : s->eslot)
            if (ticket && e.ticket == ticket) done = e.done;
    }
    if (!done) return fail(CGRT_E_ARG, "unknown ticket: never issued, or no longer in the scene's ring of enqueued frames");
    HIP_TRY(hipEventSynchronize(done));
    std::lock_guard<std::mutex> lk(s->render_mutex);
    const CgrtScene::EnqSlot* e = nullptr;
    for (const CgrtScene::EnqSlot& x : s->eslot)
        if (x.ticket == ticket) e = &x;
    if (!e) return fail(CGRT_E_ARG, "unknown ticket: no longer in the scene's ring of enqueued frames");
    CgrtRenderStats st{};
    const uint32_t* h = e->pin_ctr;
    const int ml = e->max_level;
    st.primary_rays = e->primary_rays;
    for (int level = 0; level < ml; level++) {  // the levels with entries, as the blocking frame evaluates them
        const uint32_t entries = level == 0 ? h[4 * ml + (e->fused ? 2 : 3)] : (e->fused && level == 1) ? h[4 * ml + 3] : h[4 * (level - 1) + 1];
        if (entries == 0) break;
        const bool f0 = e->fused && level == 0;  // (the fused spawn keeps no counter block: every entry is a hit)
        const uint64_t hits = f0 ? entries : h[4 * level + 2];
        st.shadow_rays += f0 ? (uint64_t)entries * e->L : h[4 * level + 0];
        st.reflection_rays += f0 ? h[4 * ml + 3] : h[4 * level + 1];
        st.soft_shadow_rays += hits * e->SL * e->samples;
        st.levels = level + 1;
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->t0, e->t1));
    st.device_ms = ms;
    if (stats) *stats = st;
    return CGRT_OK;
}
int cgrt_set_render_prediction(int enabled) {
    g_render_predict.store(enabled ? 1 : 0);
    return CGRT_OK;
}
int cgrt_debug_render_path(const CgrtScene* s) { return s ? s->rpred.last_path : -1; }

}  // extern "C"
