// capi_primary.cpp -- primary frames of the C-ABI: the frame hints and the frame gate of a launch, launch_primary, multi-view and
// ray-camera frames, the cgrt_trace_primary*, cgrt_generate_rays* and cgrt_count_primary entries, and the shadow and soft-light debug entries.
#include "capi_internal.h"

// Frame hints: which regime a frame is in goes by its size (profiles/r3_frame_hints.txt; six scenes -- the regular and the irregular
// dragon stand-in, the 87 K dragon, dodgeColorTest, monkey, Cornell -- at eight frame shapes).  Frames of up to ~0.8 M rays (640x360,
// 960x540, 800x800) are as long as their longest wave: their hard tiles are traced 16 rays per wave (0 .. -30 %, never more than
// +3 %).  Around 1 M rays the outcome depends on the scene for whole frames and halves of frames (1280x720, half a 1080p frame:
// -8 .. +7 %) -- no hints -- but a rank's share of a frame split over four or more GPUs still gains (1/8 of the 4K frame: -12 ..
// +5 %).  A 1/4 share (2 M rays) gains 2 - 6 % from tracing its hard tiles first in the usual 64-ray waves (mode 1) once the lists
// have settled, but its first twenty-odd frames are slower than plain ones: mode 1 is there to be asked for, the policy does not
// choose it.  A whole frame of that size does not gain (1080p: +2 %), larger frames gain nothing.  cgrt_set_frame_hints forces a
// mode; CGRT_FRAME_HINTS likewise.
#ifndef CGRT_HINT_SPARSE_MAX_RAYS
#define CGRT_HINT_SPARSE_MAX_RAYS 800000ull
#endif
#ifndef CGRT_HINT_SPARSE_MAX_RAYS_SHARE
#define CGRT_HINT_SPARSE_MAX_RAYS_SHARE 1300000ull  // a rank's share, four or more ranks
#endif
#ifndef CGRT_HINT_THR_DENSE
#define CGRT_HINT_THR_DENSE 4500u  // 45 us of s_memrealtime (swept: profiles/r3_frame_hints.txt)
#endif
#ifndef CGRT_HINT_THR_SPARSE
#define CGRT_HINT_THR_SPARSE 2500u  // (kept for cgrt_debug_set_hint_thresholds' second argument: a 16-ray wave counts from 5/9 of the threshold)
#endif
static int hint_mode_for(const FrameDev& F) {
    static const int env = [] {
        const char* e = getenv("CGRT_FRAME_HINTS");
        return e ? atoi(e) : -2;
    }();
    const int m = env >= -1 ? env : g_frame_hints.load();
    if (m >= 0) return m > 2 ? 0 : m;
    const unsigned long long rays = owned_pixels(F);
    if (rays <= CGRT_HINT_SPARSE_MAX_RAYS) return 2;
    if (F.nranks >= 4 && rays <= CGRT_HINT_SPARSE_MAX_RAYS_SHARE) return 2;
    return 0;  // (mode 1 is never chosen: see above)
}
// Attaches the scene's hint buffers to F for ONE launch on `stream` (or leaves F without hints).  Called with s->hints.mu held
// until the launch has been issued.  What keeps the buffers consistent: a frame reads the set the previous frame wrote, writes the
// next and zeroes the counter of the third -- so frames that use them must run one after the other.  Frames issued on one stream
// do.  When the caller changes streams, frames run WITHOUT hints (they touch no buffer) for a few launches, and before hints are
// taken up again the stream that used them last is waited for (it has long finished).
static int attach_hints(CgrtScene* s, FrameDev& F, hipStream_t stream) {
    CgrtScene::FrameHints& Hs = s->hints;
    const int mode = (F.block == 64 && !F.packed && s->dev.fast_root != REF_NONE) ? hint_mode_for(F) : 0;
    if (Hs.last_stream_valid && stream != Hs.last_stream) {
        Hs.cooldown = 8;
        Hs.have_prev = false;
    }
    const hipStream_t prev_stream = Hs.last_stream;
    const bool prev_valid = Hs.last_stream_valid;
    Hs.last_stream = stream;
    Hs.last_stream_valid = true;
    if (mode == 0) {
        Hs.have_prev = false;
        return CGRT_OK;
    }
    if (Hs.cooldown > 0) {
        if (--Hs.cooldown > 0) return CGRT_OK;
        if (prev_valid) (void)hipStreamSynchronize(prev_stream);  // (a destroyed stream answers with an error: nothing of ours is on it then)
        if (Hs.hint_stream_valid && Hs.hint_stream != stream) (void)hipStreamSynchronize(Hs.hint_stream);
        (void)hipGetLastError();
    }
    const int key[8] = {F.W, F.H, F.x0, F.y0, F.x1, F.y1, F.rank, F.nranks};
    const int per_tile = mode == 2 ? 4 : 1;
    const uint32_t ntiles = (uint32_t)F.tiles_x * (uint32_t)F.tiles_y;
    const unsigned td = g_hint_thr_dense.load(), ts = g_hint_thr_sparse.load();
    const unsigned thr[2] = {td ? td : CGRT_HINT_THR_DENSE, ts ? ts : CGRT_HINT_THR_SPARSE};
    if (!Hs.ready || std::memcmp(key, Hs.key, sizeof(key)) != 0 || Hs.per_tile != per_tile || thr[0] != Hs.thr[0] || thr[1] != Hs.thr[1]) {
        // Other buffers are needed: the frame's shape has changed.  Rebuilding waits for whatever used the old ones, so it is only
        // done for a shape that has been asked for three launches in a row -- a caller that alternates between shapes (two
        // viewports, a tool that walks through the ranks) gets plain launches, not a host synchronisation per frame.
        const int wanted[10] = {key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7], per_tile, (int)thr[0]};
        if (std::memcmp(wanted, Hs.wanted, sizeof(wanted)) != 0) {
            std::memcpy(Hs.wanted, wanted, sizeof(wanted));
            Hs.wanted_count = 0;
        }
        if (++Hs.wanted_count < 3) {
            Hs.have_prev = false;
            return CGRT_OK;
        }
        Hs.wanted_count = 0;
        // (re)build the buffers.  Whatever used the old ones must have finished.
        if (Hs.hint_stream_valid) (void)hipStreamSynchronize(Hs.hint_stream);
        (void)hipGetLastError();
        const uint64_t owned_tiles = (owned_pixels(F) + 63) / 64;
        // a list holds 4 % of the frame's tiles: the threshold keeps the listed share at 0.5 - 2 % (HintDev)
        const uint32_t cap = (uint32_t)std::min<uint64_t>(0xfffeu, std::max<uint64_t>(64, owned_tiles * 4 / 100));
        const size_t set_words = (size_t)ntiles + cap + 16;  // flag | list | count (+ padding)
        const size_t bytes = 3 * set_words * 4 + 3 * 256 + 64;
        // (hints are an accelerator: if their buffers cannot be had the frame is traced without them, it does not fail)
        hipError_t e = hipSuccess;
        if (!Hs.mailbox) {
            e = hipHostMalloc((void**)&Hs.mailbox, 64, hipHostMallocMapped);
            if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&Hs.mailbox_dev, Hs.mailbox, 0);
        }
        if (e == hipSuccess && Hs.mem_bytes < bytes) {
            if (Hs.mem) (void)hipFree(Hs.mem);
            Hs.mem = nullptr;
            Hs.mem_bytes = 0;
            e = hipMalloc(&Hs.mem, bytes);
            if (e == hipSuccess) Hs.mem_bytes = bytes;
        }
        if (e == hipSuccess) e = hipMemsetAsync(Hs.mem, 0, bytes, stream);  // (generation 0 is never used: every flag is stale; on the launch's stream: ordered before it)
        uint32_t* base = static_cast<uint32_t*>(Hs.mem);
        char* structs = reinterpret_cast<char*>(base + 3 * set_words);
        uint32_t* ctl = reinterpret_cast<uint32_t*>(structs + 3 * 256);
        auto flag = [&](int k) { return base + (size_t)k * set_words; };
        auto list = [&](int k) { return flag(k) + ntiles; };
        auto count = [&](int k) { return list(k) + cap; };
        for (int p = 0; p < 3 && e == hipSuccess; p++) {
            HintDev h{};
            const int r = p, w = (p + 1) % 3, z = (p + 2) % 3;
            h.flag_r = flag(r), h.list_r = list(r), h.count_r = count(r);
            h.flag_w = flag(w), h.list_w = list(w), h.count_w = count(w);
            h.count_z = count(z);
            h.ctl = ctl;
            h.mailbox = Hs.mailbox_dev;
            h.cap = cap;
            h.per_tile = (uint32_t)per_tile;
            h.thr_floor = thr[0];
            h.thr_ceil = thr[0] * 8u;
            h.lo = (uint32_t)std::max<uint64_t>(1, owned_tiles / 200);
            h.hi = (uint32_t)std::max<uint64_t>(4, owned_tiles * 2 / 100);
            h.thr_min = (thr[0] * 5u / 9u) - ((thr[0] * 5u / 9u) >> 2);
            Hs.phase[p] = reinterpret_cast<HintDev*>(structs + 256 * p);
            Hs.phase_host[p] = h;
            e = hipMemcpyAsync(Hs.phase[p], &h, sizeof(h), hipMemcpyHostToDevice, stream);  // (pageable source: staged before the call returns)
        }
        const uint32_t thr_start = thr[0] + thr[0] / 2;  // (HintDev: from the side on which a frame is not slower than a plain one)
        if (e == hipSuccess) e = hipMemcpyAsync(ctl, &thr_start, 4, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            Hs.ready = false;
            Hs.have_prev = false;
            return CGRT_OK;
        }
        Hs.mailbox[0] = Hs.mailbox[1] = Hs.mailbox[2] = 0;
        Hs.seen_gen = 0;
        Hs.last_listed = 0;
        Hs.empty_streak = 0;
        Hs.dormant = 0;
        std::memcpy(Hs.key, key, sizeof(key));
        Hs.per_tile = per_tile;
        Hs.thr[0] = thr[0], Hs.thr[1] = thr[1];
        Hs.cap = cap;
        Hs.seq = 0;
        Hs.have_prev = false;
        Hs.ready = true;
    }
    // What the device has said about the lists so far (never waited for: the mailbox is a frame or two behind).
    {
        volatile uint32_t* mb = Hs.mailbox;
        const uint32_t g = mb[0];
        if (g != 0 && g != Hs.seen_gen) {
            Hs.seen_gen = g;
            Hs.last_listed = mb[1];
            // ("empty": a handful of tiles does not pay for the mechanism either -- a monkey's 1/8 share with one listed tile was 6 % slower)
            Hs.empty_streak = Hs.last_listed <= std::max<uint32_t>(2u, Hs.cap / 80u) ? Hs.empty_streak + 1 : 0;
        }
    }
    // A scene without long waves (a Cornell box, a small mesh) gains nothing and pays the mechanism (3-5 us per frame): after eight
    // frames with (all but) empty lists -- at most 0.05 % of the tiles -- the frames run plain for 56 launches, then the hints are
    // tried again.
    if (Hs.dormant > 0) {
        Hs.dormant--;
        Hs.have_prev = false;
        return CGRT_OK;
    }
    if (Hs.empty_streak >= 8) {
        Hs.empty_streak = 0;
        Hs.dormant = 56;
        Hs.have_prev = false;
        return CGRT_OK;
    }
    const uint64_t seq = Hs.seq++;
    auto gen_of = [](uint64_t q) { return (uint32_t)(q % 65535u) + 1u; };
    F.hint = Hs.phase[seq % 3];
    // The launch takes every entry the list has room for.  (Sizing it from the last list length heard of was tried: a caller that
    // issues its frames back to back is dozens of launches ahead of the device, what it has heard is that much out of date -- a
    // list length of 0 from a shape's first frame kept all those launches at 32 entries, and the hints did nothing for them.)
    const uint32_t entries = Hs.cap;
    F.hint_blocks = entries * (uint32_t)per_tile;
    F.hint_rgen = Hs.have_prev ? gen_of(seq - 1) : 0u;
    F.hint_wgen = gen_of(seq);
    Hs.have_prev = true;
    Hs.hint_stream = stream;
    Hs.hint_stream_valid = true;
    return CGRT_OK;
}

// Frame order (cgrt_layout.h FrameDev::order): which frames get an order table, and when the table is rebuilt.  A frame
// qualifies when it is launched as single-wave workgroups on a fast tree, unpacked, and the hint policy above left it alone (whole
// frames and large shares: the frames whose end is set by WHERE in the launch their medium-long waves sit, not by their longest wave).
// The third launch in a row of one shape on one stream is a PROFILE frame (k_trace_primary's STAMP: same pixels, and the longest wave
// time of every super-tile), the builder follows it on the same stream and writes the table that is not in use, and the launches after it
// carry that table; every CGRT_ORDER_PERIOD launches the shape is profiled again.  All of it is enqueued: the host never waits, so a
// caller dozens of launches ahead of the device gets its table from the fourth launch on.  Streams and shapes as with the hints: a
// change means eight launches without a table, and the stream that touched the buffers last is waited for before they are used again.
#ifndef CGRT_ORDER_PERIOD
#define CGRT_ORDER_PERIOD 32
#endif
static int order_mode() {
    static const int env = [] {
        const char* e = getenv("CGRT_FRAME_ORDER");
        return e ? atoi(e) : -2;
    }();
    const int m = env >= -1 ? env : g_frame_order.load();
    return m > 1 ? 1 : m;
}
static uint32_t order_live_ticks() {
    static const uint32_t env = [] {
        const char* e = getenv("CGRT_ORDER_LIVE_TICKS");  // (experiments)
        return e ? (uint32_t)atoi(e) : CGRT_ORDER_LIVE_TICKS;
    }();
    return env;
}
static bool order_buffers(CgrtScene::FrameOrder& O, uint32_t n_pad) {
    const size_t bytes = (size_t)n_pad * 4 + 2 * (size_t)n_pad * 2;
    if (O.mem_bytes < bytes) {
        if (O.mem) (void)hipFree(O.mem);
        O.mem = nullptr;
        O.mem_bytes = 0;
        if (hipMalloc(&O.mem, bytes) != hipSuccess) {  // (the table is an accelerator: without its buffers the frame is traced plain)
            (void)hipGetLastError();
            return false;
        }
        O.mem_bytes = bytes;
    }
    O.n_pad = n_pad;
    return true;
}
static void order_drop(CgrtScene::FrameOrder& O) {
    O.state = 0;
    O.active = -1;
    O.since_profile = 0;
    O.installed = false;
}
// For ONE launch on `stream`, with s->hints.mu held until the launch has been issued (after attach_hints): 0 = no table, 1 = F.order is
// set, 2 = this launch is the shape's profile frame (launch_primary issues it and the builder, then order_profiled).
static int attach_order(CgrtScene* s, FrameDev& F, hipStream_t stream) {
    CgrtScene::FrameOrder& O = s->order;
    const uint32_t n_pad = (F.nst_rank + 7u) / 8u * 8u;
    const bool qualifies = order_mode() != 0 && !F.hint && n_pad <= CGRT_ORDER_MAX_POSITIONS && can_profile_frame(s->dev, F) && hint_mode_for(F) == 0;
    if (O.last_stream_valid && stream != O.last_stream) {
        O.cooldown = 8;
        if (!O.installed) order_drop(O);
        else O.state = 0;
    }
    const hipStream_t prev_stream = O.last_stream;
    const bool prev_valid = O.last_stream_valid;
    O.last_stream = stream;
    O.last_stream_valid = true;
    if (!qualifies) {
        O.wanted_count = 0;
        if (O.state == 2) O.state = 1;
        return 0;
    }
    const int key[8] = {F.W, F.H, F.x0, F.y0, F.x1, F.y1, F.rank, F.nranks};
    if (O.ready && std::memcmp(key, O.key, sizeof(key)) != 0) {  // another shape
        O.ready = false;
        order_drop(O);
        O.cooldown = 8;
    }
    if (!O.ready) {
        if (std::memcmp(key, O.wanted, sizeof(key)) != 0) {
            std::memcpy(O.wanted, key, sizeof(key));
            O.wanted_count = 0;
        }
        if (O.wanted_count < 3) O.wanted_count++;
    }
    if (O.cooldown > 0) {
        if (--O.cooldown > 0) return 0;
        if (prev_valid) (void)hipStreamSynchronize(prev_stream);  // (a destroyed stream answers with an error: nothing of ours is on it then)
        if (O.use_stream_valid && O.use_stream != stream) (void)hipStreamSynchronize(O.use_stream);
        (void)hipGetLastError();
    }
    if (!O.ready) {
        if (O.wanted_count < 3) return 0;
        O.wanted_count = 0;
        if (O.use_stream_valid && O.use_stream != stream) (void)hipStreamSynchronize(O.use_stream);  // whatever used the old buffers
        (void)hipGetLastError();
        if (!order_buffers(O, n_pad)) return 0;
        std::memcpy(O.key, key, sizeof(key));
        order_drop(O);
        O.ready = true;
    }
    O.use_stream = stream;
    O.use_stream_valid = true;
    if (!O.installed && (O.active < 0 || O.since_profile >= CGRT_ORDER_PERIOD - 1)) return 2;
    F.order = O.table(O.active);
    O.state = 2;
    O.since_profile++;
    return 1;
}
static void order_profiled(CgrtScene::FrameOrder& O, int table) {
    O.active = table;
    O.state = 1;
    O.since_profile = 0;
}
// A table is valid iff it is a permutation of the n positions that keeps every position's % 8 residue and maps the padded ones to themselves.
static bool order_table_valid(const uint16_t* t, uint32_t n, uint32_t nst) {
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t e = t[p];
        if (e >= n || (e & 7u) != (p & 7u) || seen[e] || ((p >= nst || e >= nst) && e != p)) return false;
        seen[e] = 1;
    }
    return true;
}

// The frame gate of one camera launch (frame_gate_rect): F's rectangle, or none.  What disables it beyond the geometry: the switch, a
// scene with spheres (resolve_hit tests every sphere for a ray that failed the mesh root gate) and a scene without a tree (walk_begin
// returns before the gate).  Nothing else is evaluated for such a ray: finish_ray writes {t as given, no primitive, no material, hit = 0}.
static bool scene_frame_gate(const CgrtScene* s, const CameraDev& C, int W, int H, int out[4]) {
    if (!s->bvh.spheres.empty() || s->bvh.root_ref == REF_NONE) return false;
    return frame_gate_rect(C, s->bvh.root_box, W, H, out);
}
void cgrt::apply_frame_gate(const CgrtScene* s, const CameraDev& C, FrameDev& F) {
    int r[4];
    F.gate_x0 = F.gate_y0 = F.gate_x1 = F.gate_y1 = 0;
    if (!g_frame_gate.load() || !scene_frame_gate(s, C, F.W, F.H, r)) return;
    if (r[2] == 0) {  // every pixel misses: a rectangle no pixel is inside of (gate_x1 != 0: the gate is on)
        F.gate_x0 = F.gate_y0 = F.gate_x1 = F.gate_y1 = 0x7fffffff;
        return;
    }
    F.gate_x0 = r[0], F.gate_y0 = r[1], F.gate_x1 = r[2], F.gate_y1 = r[3];
}

extern "C" {

int cgrt_debug_strided_waves(void) { return (int)strided_waves(); }
int cgrt_debug_hint_counts(CgrtScene* s, uint32_t* out3) {  // the three hard lists' lengths (after a device synchronise): diagnostics
    if (!s || !out3) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    std::lock_guard<std::mutex> lk(s->hints.mu);
    out3[0] = out3[1] = out3[2] = 0;
    if (!s->hints.ready) return CGRT_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < 3; k++) HIP_TRY(hipMemcpy(out3 + k, s->hints.phase_host[k].count_r, 4, hipMemcpyDeviceToHost));
    return CGRT_OK;
}
int cgrt_debug_set_hint_thresholds(unsigned dense_ticks, unsigned sparse_ticks) {
    g_hint_thr_dense.store(dense_ticks);
    g_hint_thr_sparse.store(sparse_ticks);
    return CGRT_OK;
}
int cgrt_set_frame_hints(int mode) {
    if (mode < -1 || mode > 2) return fail(CGRT_E_ARG, "frame hint mode: -1 auto, 0 off, 1 hard tiles first, 2 hard tiles 16 rays per wave");
    g_frame_hints.store(mode);
    return CGRT_OK;
}
int cgrt_set_frame_order(int mode) {
    if (mode < -1 || mode > 1) return fail(CGRT_E_ARG, "frame order mode: -1 the library's policy (default), 0 off, 1 on wherever a frame qualifies");
    g_frame_order.store(mode);
    return CGRT_OK;
}
int cgrt_debug_set_frame_order(CgrtScene* s, int W, int H, int x0, int y0, int x1, int y1, int rank, int nranks, const uint16_t* table, uint32_t n) {
    if (!s) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    std::lock_guard<std::mutex> lk(s->hints.mu);
    CgrtScene::FrameOrder& O = s->order;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());  // nothing in flight reads or writes the tables
    if (!table && n == 0) {  // back to the policy
        O.ready = false;
        order_drop(O);
        O.wanted_count = 0;
        O.cooldown = 0;
        O.last_stream_valid = O.use_stream_valid = false;
        return CGRT_OK;
    }
    FrameDev F;
    if (!table || !make_frame(W, H, x0, y0, x1, y1, rank, nranks, 64, F)) return fail(CGRT_E_ARG, "NULL table, bad frame rectangle or rank");
    const uint32_t n_pad = (F.nst_rank + 7u) / 8u * 8u;
    if (n != n_pad || n_pad == 0 || n_pad > CGRT_ORDER_MAX_POSITIONS) return fail(CGRT_E_ARG, "order table: its length must be the shape's super-tiles padded to 8");
    if (!order_table_valid(table, n, F.nst_rank)) return fail(CGRT_E_ARG, "order table: not a permutation that keeps every position's % 8 residue and the padded positions");
    if (!order_buffers(O, n_pad)) return fail(CGRT_E_HIP, "order table: no device memory");
    HIP_TRY(hipMemcpy(O.table(0), table, (size_t)n * 2, hipMemcpyHostToDevice));
    const int key[8] = {W, H, x0, y0, x1, y1, rank, nranks};
    std::memcpy(O.key, key, sizeof(key));
    order_drop(O);
    O.ready = true;
    O.installed = true;
    O.active = 0;
    O.wanted_count = 0;
    O.cooldown = 0;
    O.last_stream_valid = O.use_stream_valid = false;
    return CGRT_OK;
}
int cgrt_debug_get_frame_order(CgrtScene* s, uint16_t* table, uint32_t cap, uint32_t* n, int* state2) {
    if (!s || !n || !state2) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    std::lock_guard<std::mutex> lk(s->hints.mu);
    const CgrtScene::FrameOrder& O = s->order;
    state2[0] = O.state;
    state2[1] = O.since_profile;
    *n = 0;
    if (!O.ready || O.active < 0) return CGRT_OK;
    *n = O.n_pad;
    if (!table) return CGRT_OK;
    if (cap < O.n_pad) return fail(CGRT_E_ARG, "order table: the buffer is too short");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(table, O.table(O.active), (size_t)O.n_pad * 2, hipMemcpyDeviceToHost));
    return CGRT_OK;
}
int cgrt_debug_build_frame_order(const uint32_t* ticks, uint32_t n, uint16_t* out) {
    if (!ticks || !out) return fail(CGRT_E_ARG, "NULL argument");
    const uint32_t n_pad = (n + 7u) / 8u * 8u;
    if (n == 0 || n_pad > CGRT_ORDER_MAX_POSITIONS) return fail(CGRT_E_ARG, "order builder: 1 .. 16384 positions");
    void* mem = nullptr;
    HIP_TRY(hipMalloc(&mem, (size_t)n_pad * 6));
    uint32_t* d_ticks = static_cast<uint32_t*>(mem);
    uint16_t* d_out = reinterpret_cast<uint16_t*>(d_ticks + n_pad);
    hipError_t e = hipMemset(mem, 0, (size_t)n_pad * 6);
    if (e == hipSuccess) e = hipMemcpy(d_ticks, ticks, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_build_frame_order(d_ticks, n, CGRT_ORDER_LIVE_TICKS, d_out, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n_pad * 2, hipMemcpyDeviceToHost);
    (void)hipFree(mem);
    HIP_TRY(e);
    return CGRT_OK;
}
int cgrt_set_frame_gate(int mode) {
    if (mode != 0 && mode != 1) return fail(CGRT_E_ARG, "frame gate mode: 1 on (default), 0 off");
    g_frame_gate.store(mode);
    return CGRT_OK;
}
int cgrt_debug_frame_gate(const CgrtScene* s, const CgrtCamera* cam, int W, int H, int* out5) {
    if (!s || !cam || !out5) return fail(CGRT_E_ARG, "NULL argument");
    if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
    out5[0] = out5[1] = out5[2] = out5[3] = 0;
    out5[4] = scene_frame_gate(s, make_camera(*cam), W, H, out5) ? 1 : 0;
    return CGRT_OK;
}

static int launch_primary(CgrtScene* s, const CameraDev& C, const FrameDev& F_in, CgrtHitDev* d_hits, float* d_normals, unsigned long long* counters,
                          hipStream_t stream) {
    FrameDev F = F_in;
    apply_frame_gate(s, C, F);
    if (g_primary_mode.load() == 0 && !counters) {  // (the instrumented and the persistent kernels take no hints)
        std::lock_guard<std::mutex> lk(s->hints.mu);
        const int rc = attach_hints(s, F, stream);
        if (rc) return rc;
        if (attach_order(s, F, stream) == 2) {  // the shape's profile frame, and the builder behind it
            CgrtScene::FrameOrder& O = s->order;
            const int next = O.active < 0 ? 0 : 1 - O.active;
            HIP_TRY(launch_trace_primary_profile(s->dev, C, F, d_hits, d_normals, O.ticks(), stream));
            HIP_TRY(launch_build_frame_order(O.ticks(), F.nst_rank, order_live_ticks(), O.table(next), stream));
            order_profiled(O, next);
            return CGRT_OK;
        }
        HIP_TRY(launch_trace_primary(s->dev, C, F, d_hits, d_normals, counters, stream));
        return CGRT_OK;
    }
    if (g_primary_mode.load() == 1) {
        std::lock_guard<std::mutex> lk(s->queue_mutex);
        const unsigned k = s->launch_seq++ & 7u;
        unsigned int* q = s->d_queues + CGRT_QUEUE_BLOCK_WORDS * k;
        if (s->queue_done[k])
            HIP_TRY(hipStreamWaitEvent(stream, s->queue_done[k], 0));  // the block's previous launch, on whatever stream it ran
        else
            HIP_TRY(hipEventCreateWithFlags(&s->queue_done[k], hipEventDisableTiming));
        HIP_TRY(launch_trace_primary_persistent(s->dev, C, F, d_hits, d_normals, counters, q, s->persistent_blocks, stream));
        HIP_TRY(hipEventRecord(s->queue_done[k], stream));
    } else {
        HIP_TRY(launch_trace_primary(s->dev, C, F, d_hits, d_normals, counters, stream));
    }
    return CGRT_OK;
}

int cgrt_trace_primary_device(CgrtScene* s, const CgrtCamera* cam, int W, int H, int x0, int y0, int x1, int y1, int rank, int nranks,
                              CgrtHit* d_hits, float* d_normals, void* stream) {
    if (!s || !cam || !d_hits) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    FrameDev F;
    if (!make_frame(W, H, x0, y0, x1, y1, rank, nranks, trace_block(s->dev), F)) return fail(CGRT_E_ARG, "bad frame rectangle or rank");
    HIP_TRY(hipSetDevice(s->device));
    return launch_primary(s, make_camera(*cam), F, reinterpret_cast<CgrtHitDev*>(d_hits), d_normals, nullptr, static_cast<hipStream_t>(stream));
}

// ---- multi-view frames (include/cgrt.h cgrt_*_views*) ----
// The batch's own checks, all CGRT_E_ARG: NULL cams, nviews == 0, W or H <= 0, nviews * W * H > 0x7fffffff, more super-tiles than one
// launch takes (make_views_frame).
// The batch's size (views_args, views_light_sets_args; nviews > 0, W and H > 0): nviews * W * H and the super-tiles of all views.
extern "C++" int cgrt::views_extent_args(uint32_t nviews, int W, int H) {
    if ((unsigned long long)nviews * (unsigned long long)W * (unsigned long long)H > 0x7fffffffull)
        return fail(CGRT_E_ARG, "batch too large: nviews*W*H exceeds 0x7fffffff");
    FrameDev F;
    if (!make_views_frame(W, H, nviews, 64, F)) return fail(CGRT_E_ARG, "batch too large: more than 2^18 64x64 super-tiles over all views");
    return CGRT_OK;
}
// A batch of ray cameras (include/cgrt.h CgrtRayCamera), checked where the Trackball entries check `cams`: every field finite, a direction
// that is not identically zero, offsets that keep x + x_off and y + y_off exactly convertible to f32.
extern "C++" int cgrt::raycams_check(const CgrtRayCamera* cams, uint32_t nviews, int W, int H) {
    for (uint32_t b = 0; b < nviews; b++) {
        const CgrtRayCamera& c = cams[b];
        const float* f = c.origin;  // (the 18 floats are contiguous: static_assert below)
        for (int k = 0; k < 18; k++)
            if (!std::isfinite(f[k])) return fail(CGRT_E_ARG, "ray camera with a non-finite field");
        bool any = false;
        for (int k = 9; k < 18; k++) any = any || f[k] != 0.0f;
        if (!any) return fail(CGRT_E_ARG, "ray camera whose dir, dir_dx and dir_dy are all zero");
        const long long lim = 1ll << 24;
        if (std::llabs((long long)c.x_off) + (W > 0 ? W : 0) > lim || std::llabs((long long)c.y_off) + (H > 0 ? H : 0) > lim)
            return fail(CGRT_E_ARG, "ray camera offsets: |x_off| + W or |y_off| + H exceeds 2^24");
    }
    return CGRT_OK;
}
static_assert(sizeof(CgrtRayCamera) == 80 && offsetof(CgrtRayCamera, x_off) == 72, "CgrtRayCamera: 18 contiguous floats, two offsets");
static_assert(sizeof(CgrtRayCamera) == sizeof(RayCameraDev), "the device table holds the caller's records as they are");
// (ray: the batch's cameras are ray cameras, `cams` the same pointer)
// (extern "C++": this and the like below are capi_internal.h's, defined inside this file's extern "C" block)
extern "C++" int cgrt::views_args(const void* cams, uint32_t nviews, int W, int H, const CgrtRayCamera* ray) {
    if (!cams) return fail(CGRT_E_ARG, "cams is NULL");
    if (ray) {
        const int rc = raycams_check(ray, nviews, W, H);
        if (rc) return rc;
    }
    if (nviews == 0) return fail(CGRT_E_ARG, "nviews must be at least 1");
    if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
    return views_extent_args(nviews, W, H);
}
static std::vector<CameraDev> view_cameras(const CgrtCamera* cams, uint32_t nviews) {
    std::vector<CameraDev> v(nviews);
    for (uint32_t b = 0; b < nviews; b++) v[b] = make_camera(cams[b]);
    return v;
}
// The device table of a batch, as bytes: CameraDev per Trackball view, or the caller's ray cameras as they are (RayCameraDev).
extern "C++" std::vector<uint8_t> cgrt::view_table(const CgrtCamera* cams, const CgrtRayCamera* raycams, uint32_t nviews) {
    std::vector<uint8_t> t;
    if (raycams) {
        t.resize((size_t)nviews * sizeof(RayCameraDev));
        std::memcpy(t.data(), raycams, t.size());
    } else {
        const std::vector<CameraDev> v = view_cameras(cams, nviews);
        t.resize(v.size() * sizeof(CameraDev));
        std::memcpy(t.data(), v.data(), t.size());
    }
    return t;
}

// A launch that reads a camera table and returns before it runs (cgrt_trace_primary_views_device, cgrt_surface_views_device and their
// ray-camera twins): the table goes into the next of the scene's four slots (CgrtScene::ViewTable), is copied to the device on `st`,
// `launch` is issued with the device copy, and the slot's event is recorded behind it.
extern "C++" int cgrt::launch_with_view_table(CgrtScene* s, const std::vector<uint8_t>& tab, hipStream_t st, const std::function<hipError_t(const void*)>& launch) {
    const size_t bytes = tab.size();
    std::lock_guard<std::mutex> lk(s->vtab_mutex);
    CgrtScene::ViewTable& T = s->vtab[s->vtab_seq++ & 3u];
    if (T.pending) HIP_TRY(hipEventSynchronize(T.done));  // (the slot's last launch has read its table)
    T.pending = false;
    if (!T.done) HIP_TRY(hipEventCreateWithFlags(&T.done, hipEventDisableTiming));
    if (T.cap < bytes) {
        if (T.dev) (void)hipFree(T.dev);
        if (T.pin) (void)hipHostFree(T.pin);
        T.dev = T.pin = nullptr;
        T.cap = 0;
        HIP_TRY(hipMalloc(&T.dev, bytes));
        HIP_TRY(hipHostMalloc(&T.pin, bytes, hipHostMallocDefault));
        T.cap = bytes;
    }
    std::memcpy(T.pin, tab.data(), bytes);
    HIP_TRY(hipMemcpyAsync(T.dev, T.pin, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(launch(static_cast<const void*>(T.dev)));
    HIP_TRY(hipEventRecord(T.done, st));
    T.pending = true;
    return CGRT_OK;
}

// cgrt_trace_primary_views_device and its ray-camera twin (exactly one of cams, raycams)
static int trace_views_device(CgrtScene* s, const CgrtCamera* cams, const CgrtRayCamera* raycams, uint32_t nviews, int W, int H, CgrtHit* d_hits,
                              float* d_normals, void* stream) {
    if (!s || !d_hits) return fail(CGRT_E_ARG, "NULL argument");
    int rc = views_args(raycams ? static_cast<const void*>(raycams) : cams, nviews, W, H, raycams);
    if (rc) return rc;
    if ((uintptr_t)d_hits % 4 || (uintptr_t)d_normals % 4) return fail(CGRT_E_ARG, "d_hits / d_normals not 4-byte aligned");
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    const uint64_t npix = (uint64_t)nviews * (uint64_t)W * (uint64_t)H;
    if ((rc = check_device_span(s, d_hits, npix * sizeof(CgrtHit), "d_hits"))) return rc;
    if (d_normals && (rc = check_device_span(s, d_normals, npix * 12, "d_normals"))) return rc;
    FrameDev F;
    (void)make_views_frame(W, H, nviews, trace_block(s->dev), F);
    hipStream_t const st = static_cast<hipStream_t>(stream);
    return launch_with_view_table(s, view_table(cams, raycams, nviews), st, [&](const void* d_table) {
        F.views = static_cast<const CameraDev*>(d_table);  // (F.raycams: the same slot)
        return launch_trace_primary_views(s->dev, F, reinterpret_cast<CgrtHitDev*>(d_hits), d_normals, st, raycams != nullptr);
    });
}
int cgrt_trace_primary_views_device(CgrtScene* s, const CgrtCamera* cams, uint32_t nviews, int W, int H, CgrtHit* d_hits, float* d_normals,
                                    void* stream) {
    return trace_views_device(s, cams, nullptr, nviews, W, H, d_hits, d_normals, stream);
}
int cgrt_trace_primary_raycams_device(CgrtScene* s, const CgrtRayCamera* cams, uint32_t nviews, int W, int H, CgrtHit* d_hits, float* d_normals,
                                      void* stream) {
    return trace_views_device(s, nullptr, cams, nviews, W, H, d_hits, d_normals, stream);
}

int cgrt_trace_primary(CgrtScene* s, const CgrtCamera* cam, int W, int H, int x0, int y0, int x1, int y1, int rank, int nranks,
                       CgrtHit* hits, float* normals) {
    if (!s || !cam || !hits) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    if (W <= 0 || H <= 0) return fail(CGRT_E_ARG, "bad frame size");
    const size_t npix = (size_t)W * (size_t)H;
    LaneCall c(s);
    int rc = c.begin();
    if (rc) return rc;
    void *dh, *dn = nullptr;
    // pixels outside the traced tiles keep caller data: seed the device frame with it -- unless this call writes every pixel
    const bool whole_frame = (x0 == 0 && y0 == 0 && x1 == W && y1 == H && nranks == 1);
    HIP_TRY(whole_frame ? c.scratch(1, npix * sizeof(CgrtHit), &dh) : c.input(1, hits, npix * sizeof(CgrtHit), &dh));
    // normals of pixels that miss keep the caller's contents: seeded on the device, or -- a large whole frame, whose hit flags all
    // come from this call -- only the normals of pixels that hit are copied back
    const bool keep_by_hit = whole_frame && npix * sizeof(CgrtHit) > kStageBytes;
    if (normals) HIP_TRY(keep_by_hit ? c.scratch(2, npix * 12, &dn) : c.input(2, normals, npix * 12, &dn));
    rc = cgrt_trace_primary_device(s, cam, W, H, x0, y0, x1, y1, rank, nranks, static_cast<CgrtHit*>(dh), static_cast<float*>(dn), c.stream());
    if (rc) return rc;
    HIP_TRY(c.output(1, hits, dh, npix * sizeof(CgrtHit)));
    if (normals) HIP_TRY(c.output(2, normals, dn, npix * 12, keep_by_hit ? hits : nullptr, 12));
    HIP_TRY(c.finish());
    return CGRT_OK;
}

int cgrt_generate_rays(CgrtScene* s, const CgrtCamera* cam, int W, int H, int x0, int y0, int x1, int y1, CgrtRay* rays) {
    if (!s || !cam || !rays) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    FrameDev F;
    if (!make_frame(W, H, x0, y0, x1, y1, 0, 1, CGRT_BLOCK, F)) return fail(CGRT_E_ARG, "bad frame rectangle");
    const size_t n = (size_t)(x1 - x0) * (size_t)(y1 - y0);
    if (!n) return CGRT_OK;
    LaneCall c(s);
    int rc = c.begin();
    if (rc) return rc;
    void* dr;
    HIP_TRY(c.scratch(0, n * sizeof(CgrtRay), &dr));
    HIP_TRY(launch_generate_rays(make_camera(*cam), W, H, x0, y0, x1, y1, static_cast<float*>(dr), c.stream()));
    HIP_TRY(c.output(0, rays, dr, n * sizeof(CgrtRay)));
    HIP_TRY(c.finish());
    return CGRT_OK;
}

int cgrt_generate_rays_raycam(CgrtScene* s, const CgrtRayCamera* cam, int W, int H, CgrtRay* rays) {
    if (!s || !cam || !rays) return fail(CGRT_E_ARG, "NULL argument");
    int rc = raycams_check(cam, 1, W, H);
    if (rc) return rc;
    FrameDev F;
    if (!make_frame(W, H, 0, 0, W, H, 0, 1, CGRT_BLOCK, F)) return fail(CGRT_E_ARG, "bad frame size");
    NEED_DEVICE(s);
    const size_t n = (size_t)W * (size_t)H;
    LaneCall c(s);
    if ((rc = c.begin())) return rc;
    void* dr;
    HIP_TRY(c.scratch(0, n * sizeof(CgrtRay), &dr));
    RayCameraDev C;
    std::memcpy(&C, cam, sizeof(C));
    HIP_TRY(launch_generate_rays_raycam(C, W, H, static_cast<float*>(dr), c.stream()));
    HIP_TRY(c.output(0, rays, dr, n * sizeof(CgrtRay)));
    HIP_TRY(c.finish());
    return CGRT_OK;
}

int cgrt_count_primary(CgrtScene* s, const CgrtCamera* cam, int W, int H, int x0, int y0, int x1, int y1, int rank, int nranks,
                       CgrtCounters* out) {
    if (!s || !cam || !out) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    FrameDev F;
    if (!make_frame(W, H, x0, y0, x1, y1, rank, nranks, trace_block(s->dev), F)) return fail(CGRT_E_ARG, "bad frame rectangle or rank");
    LaneCall c(s);
    int rc = c.begin();
    if (rc) return rc;
    void* dh;
    HIP_TRY(c.scratch(1, (size_t)W * (size_t)H * sizeof(CgrtHit), &dh));
    HIP_TRY(c.zero_counters(8));
    rc = launch_primary(s, make_camera(*cam), F, static_cast<CgrtHitDev*>(dh), nullptr, c.counters(), c.stream());
    if (rc) return rc;
    HIP_TRY(c.read_counters(&out->rays, 8));
    return CGRT_OK;
}

int cgrt_debug_wave_times(CgrtScene* s, const CgrtCamera* cam, int W, int H, uint64_t* out, uint64_t cap_waves) {
    if (!s || !cam || !out) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    FrameDev F;
    if (!make_frame(W, H, 0, 0, W, H, 0, 1, trace_block(s->dev), F)) return fail(CGRT_E_ARG, "bad frame");
    const size_t nwaves = (size_t)F.nblocks * (size_t)(F.block / 64);
    if (cap_waves < nwaves) return fail(CGRT_E_ARG, "output too small");
    HIP_TRY(hipSetDevice(s->device));
    DevBuf dh, ds;
    HIP_TRY(dh.alloc((size_t)W * (size_t)H * sizeof(CgrtHit)));
    HIP_TRY(ds.alloc(nwaves * 128));
    HIP_TRY(hipMemset(ds.p, 0, nwaves * 128));
    std::lock_guard<std::mutex> lk(s->hints.mu);
    {  // the whole frame's order table, when the scene has one in use: the stamps are then those of the ordered launch
        const CgrtScene::FrameOrder& O = s->order;
        const int key[8] = {W, H, 0, 0, W, H, 0, 1};
        if (order_mode() != 0 && O.ready && O.active >= 0 && std::memcmp(key, O.key, sizeof(key)) == 0) {
            HIP_TRY(hipDeviceSynchronize());  // (the builder may be behind a frame on another stream)
            F.order = O.table(O.active);
        }
    }
    for (int rep = 0; rep < 3; rep++)  // warm caches, keep the last
        HIP_TRY(launch_trace_primary_stamped(s->dev, make_camera(*cam), F, dh.as<CgrtHitDev>(), ds.as<unsigned long long>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, ds.p, nwaves * 128, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

// The frame's shadow-list launchers on caller rays (include/cgrt.h).  Only plumbing: the launches are the ones render_impl issues.
int cgrt_debug_trace_shadow(CgrtScene* s, const CgrtRay* rays, const float* dist, uint64_t n, int how, uint32_t dmul, uint64_t capacity,
                            uint64_t expected, const CgrtRay* mirror_rays, uint64_t nmirror, uint64_t mirror_capacity, uint64_t mirror_expected,
                            CgrtHit* mirror_hits, float* mirror_normals, CgrtHit* hits) {
    if (how < 0 || how > 2) return fail(CGRT_E_ARG, "how must be 0 (plain), 1 (length on the device) or 2 (paired with a mirror list)");
    const uint64_t cap = how == 0 ? n : std::max<uint64_t>(n, capacity);
    if (!s || (n && (!rays || !dist)) || (cap && !hits)) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    if (how >= 1) {
        if (dmul == 0 || n % dmul != 0) return fail(CGRT_E_ARG, "n must be a multiple of dmul >= 1");
        if (n / dmul > 0xffffffffull) return fail(CGRT_E_ARG, "n / dmul must fit the device word");
    }
    const uint64_t mcap = std::max<uint64_t>(nmirror, mirror_capacity);
    if (how == 2) {
        if ((nmirror && !mirror_rays) || (mcap && !mirror_hits)) return fail(CGRT_E_ARG, "NULL mirror argument");
        if (nmirror > 0xffffffffull) return fail(CGRT_E_ARG, "nmirror must fit the device word");
        if (!can_trace_pair(s->dev)) return fail(CGRT_E_ARG, "the scene or the forced kernel shape does not allow the paired launch");
    }
    HIP_TRY(hipSetDevice(s->device));
    DevBuf dr, dd, dh, dc, mr, mh, mn;
    HIP_TRY(dr.alloc(cap * sizeof(CgrtRay)));
    HIP_TRY(dd.alloc(cap * sizeof(float)));
    HIP_TRY(dh.alloc(cap * sizeof(CgrtHit)));
    HIP_TRY(dc.alloc(2 * sizeof(uint32_t)));
    // rays past n (the grid covers them, the device word does not) are zero rays: a kernel that read them would not fault
    HIP_TRY(hipMemset(dr.p, 0, cap * sizeof(CgrtRay)));
    HIP_TRY(hipMemset(dd.p, 0, cap * sizeof(float)));
    HIP_TRY(hipMemset(dh.p, 0xA5, cap * sizeof(CgrtHit)));
    HIP_TRY(hipMemcpy(dr.p, rays, n * sizeof(CgrtRay), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dd.p, dist, n * sizeof(float), hipMemcpyHostToDevice));
    const uint32_t words[2] = {how >= 1 ? (uint32_t)(n / dmul) : 0u, (uint32_t)nmirror};
    HIP_TRY(hipMemcpy(dc.p, words, sizeof(words), hipMemcpyHostToDevice));
    uint32_t* const dcount = dc.as<uint32_t>();
    const ShadowList shadows = how == 0 ? ShadowList{dr.as<float>(), dd.as<float>(), n, dh.as<CgrtHitDev>()}
                                        : ShadowList{dr.as<float>(), dd.as<float>(), cap, dh.as<CgrtHitDev>(), dcount, dmul, expected};
    if (how <= 1) {
        HIP_TRY(launch_trace_shadow(s->dev, shadows, nullptr, nullptr));
    } else {
        HIP_TRY(mr.alloc(mcap * sizeof(CgrtRay)));
        HIP_TRY(mh.alloc(mcap * sizeof(CgrtHit)));
        HIP_TRY(mn.alloc(mcap * 12));
        HIP_TRY(hipMemset(mr.p, 0, mcap * sizeof(CgrtRay)));
        HIP_TRY(hipMemset(mh.p, 0xA5, mcap * sizeof(CgrtHit)));
        HIP_TRY(hipMemset(mn.p, 0xA5, mcap * 12));
        HIP_TRY(hipMemcpy(mr.p, mirror_rays, nmirror * sizeof(CgrtRay), hipMemcpyHostToDevice));
        HIP_TRY(launch_trace_pair(s->dev, shadows, RayList{mr.as<float>(), mcap, mh.as<CgrtHitDev>(), mn.as<float>(), dcount + 1, mirror_expected}, nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hits, dh.p, cap * sizeof(CgrtHit), hipMemcpyDeviceToHost));
    if (how == 2 && mcap) {
        HIP_TRY(hipMemcpy(mirror_hits, mh.p, mcap * sizeof(CgrtHit), hipMemcpyDeviceToHost));
        if (mirror_normals) HIP_TRY(hipMemcpy(mirror_normals, mn.p, mcap * 12, hipMemcpyDeviceToHost));
    }
    return CGRT_OK;
}

// SoftDev of the caller's sampling parameters, for SL spherical lights and the unit vectors where they lie on the device; level,
// view_pixels and set_index are the caller's to set
extern "C++" SoftDev cgrt::soft_dev(const CgrtSoftShadows& soft, unsigned SL, const float* lights, const float* units) {
    SoftDev Q{};
    Q.lights = lights, Q.units = units, Q.nlights = SL;
    Q.samples = soft.samples, Q.nunits = soft.nunits, Q.seed = soft.seed;
    return Q;
}
// The frame's soft-shadow launcher on caller items (include/cgrt.h).
int cgrt_debug_soft_lit(CgrtScene* s, const CgrtRay* item_rays, const CgrtHit* item_hits, const int32_t* item_pixels, uint64_t nitems,
                        const CgrtSoftShadows* soft, int level, int anyhit, uint32_t* lit) {
    if (!s || !soft || (nitems && (!item_rays || !item_hits || !item_pixels || !lit))) return fail(CGRT_E_ARG, "NULL argument");
    if (soft->nspherical && (!soft->spherical || !soft->unit_vectors || soft->nunits == 0 || soft->samples == 0 || soft->samples > (1u << 24)))
        return fail(CGRT_E_ARG, "spherical lights need a unit-vector table and 1..2^24 samples");
    if (level < 0) return fail(CGRT_E_ARG, "level must be >= 0");
    NEED_DEVICE(s);
    const uint64_t SL = soft->nspherical;
    if (nitems == 0 || SL == 0) return CGRT_OK;
    HIP_TRY(hipSetDevice(s->device));
    DevBuf dr, dh, dp, dl, du, dlit;
    HIP_TRY(dr.alloc(nitems * sizeof(CgrtRay)));
    HIP_TRY(dh.alloc(nitems * sizeof(CgrtHit)));
    HIP_TRY(dp.alloc(nitems * sizeof(int32_t)));
    HIP_TRY(dl.alloc(SL * 28));
    HIP_TRY(du.alloc((size_t)soft->nunits * 12));
    HIP_TRY(dlit.alloc(nitems * SL * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(dr.p, item_rays, nitems * sizeof(CgrtRay), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dh.p, item_hits, nitems * sizeof(CgrtHit), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dp.p, item_pixels, nitems * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dl.p, soft->spherical, SL * 28, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(du.p, soft->unit_vectors, (size_t)soft->nunits * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dlit.p, 0, nitems * SL * sizeof(uint32_t)));
    SoftDev Q = soft_dev(*soft, (unsigned)SL, dl.as<float>(), du.as<float>());
    Q.level = (uint32_t)level;
    HIP_TRY(launch_soft_shadow(s->dev, Q, dr.as<float>(), dh.as<CgrtHitDev>(), dp.as<int>(), nitems, dlit.as<uint32_t>(), anyhit != 0, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(lit, dlit.p, nitems * SL * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CGRT_OK;
}

}  // extern "C"
