// capi_internal.h -- what the translation units of the C-ABI (capi.cpp, capi_combine.cpp, capi_primary.cpp, capi_frames.cpp,
// capi_frame_entries.cpp, capi_multi.cpp, capi_lanes.cpp, capi_queries.cpp, capi_prims.cpp) share: error reporting, the scene, the helpers
// more than one of them calls, the call lanes.  The shaded frame's units share capi_frames.h besides.  Host code only: no .hip file includes it.
// What it declares in namespace cgrt has hidden visibility: libcgrt.so exports include/cgrt.h's entries, not these.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <linux/futex.h>
#include <map>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "../../include/cgrt.h"
#include "bvh_builder.h"
#include "cgrt_layout.h"
#include "cgrt_math.h"
#include "closest_kernels.h"
#include "crossing_kernels.h"
#include "grad_repro_kernels.h"
#include "grid_field_grad_repro_kernels.h"
#include "grid_field_kernels.h"
#include "isosurface_kernels.h"
#include "neighbor_kernels.h"
#include "point_frame_kernels.h"
#include "point_neighbor_kernels.h"
#include "poisson_kernels.h"
#include "sdf_kernels.h"
#include "surface_grad_repro_kernels.h"
#include "surface_kernels.h"
#include "surface_sample_builder.h"
#include "surface_sample_kernels.h"
#include "trace_kernels.h"
#include "winding_kernels.h"

using namespace cgrt;

#pragma GCC visibility push(hidden)
namespace cgrt {
// Process-wide options (capi.cpp), read atomically by every launch
extern std::atomic<int> g_call_combining;  // cgrt_set_call_combining
extern std::atomic<int> g_render_predict;  // cgrt_set_render_prediction
extern std::atomic<int> g_frame_hints;    // cgrt_set_frame_hints: -1 auto, 0 off, 1 hard tiles first, 2 hard tiles 16 rays per wave
extern std::atomic<unsigned> g_hint_thr_dense, g_hint_thr_sparse;  // cgrt_debug_set_hint_thresholds (0: the defaults)
extern std::atomic<int> g_frame_order;     // cgrt_set_frame_order: -1 = the library's policy (on), 0 = off, 1 = on wherever a frame qualifies
extern std::atomic<int> g_frame_gate;      // cgrt_set_frame_gate: 1 = tiles outside the root box's screen rectangle skip their rays, 0 = off
extern std::atomic<int> g_primary_mode;  // 0 = one wave per tile, 1 = persistent waves with lane refill

// Every failure returns through these: the message is cgrt_last_error()'s, per thread (capi.cpp)
extern thread_local std::string g_err;
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);
#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)
#define CGRT_TRY(expr)              \
    do {                            \
        const int _rc = (expr);     \
        if (_rc) return _rc;        \
    } while (0)

// RAII device buffer for the host-pointer convenience entries.
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

int select_device(int device);
CameraDev make_camera(const CgrtCamera& c);
bool make_frame(int W, int H, int x0, int y0, int x1, int y1, int rank, int nranks, int block, FrameDev& F);
bool make_views_frame(int W, int H, uint32_t nviews, int block, FrameDev& F);
bool frame_gate_rect(const CameraDev& C, const Box6& box, int W, int H, int out[4]);
unsigned long long owned_pixels(const FrameDev& F);
}  // namespace cgrt
#pragma GCC visibility pop

// The slots of a scene's device workspace (CgrtScene::work), by what the shaded frame keeps in them (capi_frames.cpp Wavefront and render_impl).  A
// level's list (rays / hits / normals / pixels) has four buffer sets and its shadow list two; their numbers are not contiguous because
// slots were added as features came.
enum WorkSlotId {
    WS_RAYS0, WS_RAYS1, WS_HITS0, WS_HITS1, WS_NORMALS0, WS_NORMALS1, WS_PIX0, WS_PIX1, WS_IPIX,  // 0..8
    WS_SRAYS0, WS_SHITS0, WS_SDIST0, WS_SSLOT0,                                                   // 9..12
    WS_LIGHTS, WS_LEVELS, WS_RGB, WS_CTR, WS_SLIGHTS, WS_UNITS, WS_LIT, WS_COUNTED,               // 13..20
    WS_RAYS2, WS_HITS2, WS_NORMALS2, WS_PIX2, WS_SRAYS1, WS_SHITS1, WS_SDIST1, WS_SSLOT1,         // 21..28
    WS_SPAWN, WS_RESOLVED, WS_VIEWS, WS_SETS, WS_SETTAB,  // 29..33 (32 and 33: light-set batches only)
    WS_RAYS3, WS_HITS3, WS_NORMALS3, WS_PIX3,             // 34..37: deep frames with geometry buffers only
    WS_SLOTS
};
static_assert(WS_RGB == 15 && WS_RESOLVED == 30 && WS_SLOTS == 38, "the workspace's slot numbers");

struct CgrtScene {
    int device = 0;
    BuiltBvh bvh;
    uint32_t ntris = 0;
    SceneDev dev = [] {
        SceneDev d{};
        d.fast_root = REF_NONE;
        d.root_ref = REF_NONE;
        return d;
    }();
    void* d_records = nullptr;  // [packets | subnodes | tris], 64 B each
    void* d_leaves = nullptr;
    void* d_tri_normals = nullptr;
    void* d_spheres = nullptr;
    void* d_materials = nullptr;  // nmesh x 8 floats, for the shading wavefront
    void* d_tri_leaf = nullptr;   // certified walk: leaf of every record, per-leaf box paths (SceneDev::tri_leaf, paths)
    void* d_paths = nullptr;
    uint32_t fast_root = REF_NONE;  // the scene's fast tree (REF_NONE: none); dev.fast_root is this or REF_NONE by cgrt_scene_set_walk
    uint32_t nmesh = 0;
    unsigned int* d_queues = nullptr;  // ring of 8 queue blocks (CGRT_QUEUE_BLOCK_WORDS u32 each) for the persistent kernel, reset by every launch
    // the persistent kernel's launches take the queue blocks in turn; a block is handed to a new launch only behind the
    // launch that used it last (an event per block), so any number of frames may be in flight on any streams
    std::mutex queue_mutex;
    unsigned launch_seq = 0;
    // Frame hints (cgrt_layout.h HintDev; capi_primary.cpp attach_hints): the hard-tile lists a primary frame leaves for the next frame of
    // the same shape.  Guarded by hints_mutex while a launch is being issued; the buffers themselves are only touched by kernels.
    struct FrameHints {
        std::mutex mu;
        bool ready = false;           // buffers allocated for `key`
        int key[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // W, H, x0, y0, x1, y1, rank, nranks
        int wanted[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // the shape (+ mode, threshold) of the last launches that asked for other buffers
        int wanted_count = 0;         // ... and how many in a row did
        int per_tile = 0;             // 1 / 4 (the policy the buffers were made for)
        unsigned thr[2] = {0, 0};     // the thresholds in the device structs
        uint32_t cap = 0;
        void* mem = nullptr;          // 3 x {flag[ntiles], list[cap], count} + 3 HintDev
        size_t mem_bytes = 0;
        HintDev* phase[3] = {nullptr, nullptr, nullptr};  // device addresses
        HintDev phase_host[3];        // what they hold
        uint32_t* mailbox = nullptr;  // 64 pinned, device-mapped bytes: {generation, length of the list that frame read, threshold}
        uint32_t* mailbox_dev = nullptr;
        uint32_t seen_gen = 0;        // the last mailbox generation the host has looked at
        uint32_t last_listed = 0;     // ... and what it said
        int empty_streak = 0;         // hinted frames in a row whose list was empty
        int dormant = 0;              // frames still to run plain because of that
        uint64_t seq = 0;             // frames issued with these buffers
        bool have_prev = false;       // the set this frame would read was written by frame seq - 1
        hipStream_t last_stream = nullptr;
        bool last_stream_valid = false;
        hipStream_t hint_stream = nullptr;  // the stream of the last launch that used the buffers
        bool hint_stream_valid = false;
        int cooldown = 0;             // frames to run without hints after the caller changed streams
    } hints;
    // Frame order (cgrt_layout.h FrameDev::order; capi_primary.cpp attach_order): the order table the frames of one shape on
    // one stream are launched with, rebuilt on the device behind a profile frame.  Guarded by hints.mu, like the hints, while a launch is
    // being issued; ticks and tables are only touched by kernels and copies on `use_stream`.
    struct FrameOrder {
        bool ready = false;            // buffers allocated for `key`
        int key[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // W, H, x0, y0, x1, y1, rank, nranks
        int wanted[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the shape of the last launches that asked for other buffers
        int wanted_count = 0;          // ... and how many in a row did
        void* mem = nullptr;           // ticks[n_pad] u32 | table 0 [n_pad] u16 | table 1 [n_pad] u16
        size_t mem_bytes = 0;
        uint32_t n_pad = 0;            // positions of the launch: the shape's super-tiles padded to 8
        int active = -1;               // the table frames are launched with (-1: none yet)
        int state = 0;                 // 0 none, 1 profiled (the builder is behind the last launch), 2 active (the last launch read the table)
        int since_profile = 0;         // launches of the shape since its profile frame
        bool installed = false;        // the table is a caller's (cgrt_debug_set_frame_order): used as it is, never profiled
        hipStream_t last_stream = nullptr;  // the stream of the last launch that could have taken a table
        bool last_stream_valid = false;
        hipStream_t use_stream = nullptr;   // the stream of the last launch that touched the buffers
        bool use_stream_valid = false;
        int cooldown = 0;              // launches to run without a table after the caller changed streams or shapes
        uint32_t* ticks() const { return static_cast<uint32_t*>(mem); }
        uint16_t* table(int k) const { return reinterpret_cast<uint16_t*>(ticks() + n_pad) + (size_t)k * n_pad; }
    } order;
    hipEvent_t queue_done[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // Host-pointer entries (cgrt_intersect_batch, cgrt_trace_primary, cgrt_count_*, ...) run on "call lanes": a private
    // stream + device scratch + pinned staging + a counter block, taken from this pool for the duration of one call and
    // kept afterwards.  Concurrent callers (the reference calls intersect from an omp parallel for, main.cpp:653-656) get
    // different lanes; no call allocates, frees or synchronises the device once its lane has grown to the call's size.
    struct CallLane {
        hipStream_t stream = nullptr;
        struct Buf {
            void* p = nullptr;
            size_t cap = 0;
        } dev[5], pin[5];  // rays / hits / normals / light tables / a query's fifth array (per-query radii)
        void* bounce[2] = {nullptr, nullptr};  // pinned halves of the large-transfer pipeline (lane_upload / lane_download), made on first use
        hipEvent_t bounce_ev[2] = {nullptr, nullptr};
        hipEvent_t follow = nullptr;  // lane_follow: the lane's stream waits for the caller's, made on first use
        unsigned long long* d_counters = nullptr;
    };
    std::mutex lanes_mutex;
    std::vector<CallLane*> lanes_free, lanes_all;
    // Call combining (cgrt_intersect_batch with a handful of rays, i.e. BoundingVolumeHierarchy::intersect as the reference's
    // `omp parallel for` issues it, main.cpp:653-656: one ray per call from many threads at once).  A launch per ray costs the
    // GPU round trip per RAY; here concurrent callers append their rays to the open GENERATION of one of two pinned, device-mapped
    // rings; the first caller of a generation is its leader: it closes the generation, launches ONE kernel over all its rays
    // (the kernel reads the rays from and writes the hits to host memory directly: no copy commands), waits for that stream and
    // publishes the results; the other callers wait on the generation's state and copy their own hits out.  While a generation
    // is on the GPU the next one fills up, so the batch size adapts to the load.  Nothing stays resident on the device.
#ifndef CGRT_COMBINE_RINGS
#define CGRT_COMBINE_RINGS 16  // most generations that can be open / in flight at a time; `nrings` of them are used
#endif
    struct Combiner {
        static const int NRINGS = CGRT_COMBINE_RINGS;
        int nrings = 8;  // set before the rings are made (combined_intersect; CGRT_COMBINE_NRINGS)
        static const uint32_t CAP = 32768;       // ray slots per ring
        static const uint32_t MAX_N = 64;        // calls with more rays than this take the direct path
        static const int MAX_CALLERS = 256;      // callers inside the entry at a time (more take the direct path)
        static const uint32_t JOIN_MAX = CAP - MAX_N * MAX_CALLERS;  // a generation is joined while it holds at most this many rays:
                                                                     // MAX_CALLERS joins of MAX_N rays in flight cannot overflow it
        enum State : uint64_t { FREE = 0, OPEN = 1, RUNNING = 2, DONE = 3 };
        // One 64-bit word per ring says everything a caller needs, so joining is ONE atomic add, leader election and closing single
        // compare-and-swaps, and nobody takes a lock on the way in (with a mutex 64 callers formed a convoy: 139 K calls/s):
        //   bits 0..1 state | 2..15 callers that joined | 16..31 rays appended | 32..63 generation number
        // An add that arrives after the generation was closed lands on a RUNNING / DONE / FREE word: the adder sees the old state in
        // the value it gets back and tries again elsewhere; the stray counts are overwritten by the next transition (the leader
        // keeps its own copy of the counts it closed with), and the caller limit keeps them inside their bit fields.
        static uint64_t pack(uint64_t st, uint64_t joined, uint64_t count, uint64_t gen) { return st | (joined << 2) | (count << 16) | (gen << 32); }
        static uint64_t st_of(uint64_t w) { return w & 3u; }
        static uint32_t joined_of(uint64_t w) { return (uint32_t)((w >> 2) & 0x3fffu); }
        static uint32_t count_of(uint64_t w) { return (uint32_t)((w >> 16) & 0xffffu); }
        struct alignas(64) Ring {
            std::atomic<uint64_t> word{0};     // FREE, generation 0
            char pad0[56];
            // what the WAITERS of a generation spin on -- a line of its own, written once per generation: spinning on `word`
            // made every join fight 60 readers for the line (64 callers: 0.46 M calls/s)
            std::atomic<uint32_t> done_gen{0}; // generations of this ring whose results are published
            char pad1[60];
            std::atomic<uint32_t> copied{0};   // joiners whose rays are in the ring (the leader launches when copied == joined)
            std::atomic<uint32_t> readers{0};  // callers that still have to copy their results out (the last one frees the ring)
            char pad2[56];
            void* host = nullptr;  // pinned + mapped: [CgrtRay x CAP | CgrtHit x CAP | normals 3 x CAP]
            void* dev = nullptr;   // the same memory as the device sees it
            hipStream_t stream = nullptr;
            int rc = 0;            // the leader's status for the whole generation (written before done_gen is published)
            std::string err;
        } ring[CGRT_COMBINE_RINGS];
        std::mutex init_mu;
        // Callers that SLEEP (futex) instead of spinning -- taken when more callers are inside than the process has CPUs (see
        // combined_intersect): `epoch` counts rings set free (what callers without a ring wait for), the sleeper counts tell the
        // thread that publishes whether a wake-up call is needed at all.
        alignas(64) std::atomic<uint32_t> epoch{0};
        std::atomic<int> epoch_sleepers{0}, done_sleepers{0};
        alignas(64) std::atomic<int> inside{0};   // callers currently inside the combining entry
        alignas(64) std::atomic<int> ready{0};    // 0 = rings not allocated yet, 1 = usable, -1 = allocation failed (direct path for good)
        // diagnostics (cgrt_debug_combiner_stats): generations launched, rays in them, the largest generation, nanoseconds the
        // leaders spent from closing a generation to its results (launch + kernel + stream wait)
        std::atomic<uint64_t> n_gen{0}, n_rays{0}, max_gen{0}, ns_gpu{0}, ns_launch{0};  // ns_launch: the part of ns_gpu spent issuing the launch
    } comb;
    std::mutex render_mutex;  // cgrt_render* share the workspace below: one frame per scene at a time
    unsigned persistent_blocks = 1024;  // 4 workgroups per CU
    // Device workspace of cgrt_render*: kept between frames (a frame of the same shape then allocates nothing; hipMalloc and
    // hipFree of ~20 buffers cost more than the frame itself), grown on demand, released with the scene.
    struct WorkSlot {
        void* p = nullptr;
        size_t cap = 0;
    } work[WS_SLOTS];
    // pinned host staging of cgrt_render*'s frame (grown on demand, guarded by render_mutex): the device frame comes down with ONE
    // asynchronous copy at PCIe speed; cgrt_render_mapped hands this memory to the caller instead of copying it once more
    void* pin_frame = nullptr;
    size_t pin_frame_cap = 0;
    // streams and events of cgrt_render* (created once per scene, guarded by render_mutex: creating and destroying a stream and
    // five events per frame cost more host time than the Cornell frame's device time)
    struct RenderAux {
        hipStream_t s = nullptr, copy = nullptr;  // second traversal stream; read-backs that must not wait for queued kernels
        hipEvent_t spawned = nullptr, traced = nullptr, e0 = nullptr, e1 = nullptr, primary_done = nullptr;
        hipEvent_t caller = nullptr;     // cgrt_shade_rays*: the frame's streams start behind what the caller's stream held
        // geometry buffers of a blocking frame: the planes are written on a stream of their own, behind `caller`
        // (what the caller's stream held) -- the miss values while the frame is traced, level 0's entries beside the colour export -- and
        // the caller's stream waits for `filled`, recorded behind them
        hipStream_t fill = nullptr;
        hipEvent_t filled = nullptr;
        uint32_t* pin_counts = nullptr;  // 64 pinned bytes for counter read-backs
        SpawnDev spawn_host{};           // what the workspace's SpawnDev (fused level-0 spawn of predicted frames) holds
        bool spawn_valid = false;
    } raux;
    // cgrt_render_device: its export kernel reads the frame (work slot WS_RGB, or WS_RESOLVED with aa) on the CALLER's stream after the call has
    // returned.  This event is recorded behind it, and the next cgrt_render* call on the scene makes every stream it uses wait on it
    // (and waits for it on the host before it reallocates those buffers); the caller's stream handle itself is never kept.
    hipEvent_t export_done = nullptr;
    bool export_pending = false;  // recorded, and no later frame has waited for it yet
    // cgrt_trace_primary_views_device: the camera tables of its launches (CameraDev per view), which return before the kernels run.  Four
    // slots in turn, each a pinned host copy and a device copy; a slot is refilled only once the event recorded behind its last launch
    // has completed, so the copy never reads memory the caller has since reused (the tables come from the caller's stack or array).
    struct ViewTable {
        void* pin = nullptr;
        void* dev = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        bool pending = false;
    } vtab[4];
    unsigned vtab_seq = 0;
    std::mutex vtab_mutex;
    // What the previous cgrt_render* frame of this shape found, per level (entries of the level's compact list): the next frame's
    // launches are sized from it and issued WITHOUT waiting for the device to say how many primary rays hit (render_impl).
    struct RenderPred {
        bool valid = false;
        int W = 0, H = 0, rank = 0, nranks = 0, max_level = 0;
        unsigned L = 0;
        std::vector<uint32_t> counts;
        int last_path = 0;  // how the last frame was drawn: 0 exact, 1 as predicted, 2 predicted, found too small, drawn again exactly
    } rpred;
    // Enqueued frames (cgrt_enqueue_*; capi_frames.cpp enqueue_impl): a ring of ENQ_SLOTS ticket slots, each with pinned
    // staging for the frame's tables (copied to enq_dev by hipMemcpyAsync on the caller's stream), a pinned read-back of its counter block
    // and the events behind it.  A slot is refilled only once its last frame has finished.  Every frame of the scene (enqueued or blocking)
    // starts behind the last enqueued one on the device (enq_done), so all of them share the workspace above.
    static const int ENQ_SLOTS = 8;
    struct EnqSlot {
        void* pin = nullptr;         // lights | spherical lights | unit vectors | SpawnDev | view table
        size_t cap = 0;
        uint32_t* pin_ctr = nullptr;  // the frame's counter block, copied back behind the frame (cgrt_enqueue_stats)
        hipEvent_t done = nullptr, t0 = nullptr, t1 = nullptr;
        bool pending = false;
        uint64_t ticket = 0;          // 0: never used
        // what cgrt_enqueue_stats needs to turn the counters into CgrtRenderStats
        int max_level = 0, fused = 0;
        unsigned L = 0, SL = 0, samples = 0;
        uint64_t primary_rays = 0;
    } eslot[ENQ_SLOTS];
    unsigned enq_count = 0;           // enqueued frames issued (slot = enq_count % ENQ_SLOTS)
    uint64_t frame_seq = 0;           // the scene's frames, blocking and enqueued: an enqueued frame's ticket is its number
    void* enq_dev = nullptr;          // the device copy of the tables (frames are ordered on the device, so one copy serves them all)
    size_t enq_dev_cap = 0;
    hipEvent_t enq_done = nullptr;    // behind the last enqueued frame (one of the slots' `done`)
    bool enq_pending = false;
    uint64_t device_bytes = 0;
    // Surface attributes (cgrt_hit_barycentrics*, cgrt_interpolate_hits*, cgrt_surface_*): the triangles' vertex
    // indices as the caller gave them (host memory only) and, from the first surface call on, the device table prim_id -> {record, three
    // vertex rows} (surface_kernels.h SurfaceLookup).  A scene that makes no such call never allocates it.
    uint32_t nverts = 0;
    std::vector<uint32_t> tri_index;  // ntris x 3
    std::mutex surface_mutex;
    std::atomic<void*> d_surface_lookup{nullptr};
    // Winding numbers (cgrt_winding_numbers*): the cluster tree over the records (winding_builder.h), made on the
    // host by the scene's first winding call under surface_mutex (a host-only scene included: cgrt_debug_get_winding_tree reads it), and
    // its device copy, uploaded once by the first call that launches.  A scene that makes no such call never builds either.
    WindingTree winding;
    std::atomic<bool> winding_built{false};
    std::atomic<void*> d_winding{nullptr};
    // Surface sampling (cgrt_sample_surface*): the areas and thresholds in prim_id order (surface_sample_builder.h),
    // made on the host by the scene's first sampling call under surface_mutex (a host-only scene included: cgrt_triangle_areas and
    // cgrt_debug_get_sample_table read it), and the thresholds' device copy, uploaded once by the first call that launches.
    SampleTable sampling;
    std::atomic<bool> sampling_built{false};
    std::atomic<void*> d_sampling{nullptr};
    ~CgrtScene() {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (void* p = d_surface_lookup.load()) (void)hipFree(p);
        if (void* p = d_winding.load()) (void)hipFree(p);
        if (void* p = d_sampling.load()) (void)hipFree(p);
        for (EnqSlot& e : eslot) {  // (frames in flight complete before anything they use is released)
            if (e.pending) (void)hipEventSynchronize(e.done);
            for (hipEvent_t ev : {e.done, e.t0, e.t1})
                if (ev) (void)hipEventDestroy(ev);
            if (e.pin) (void)hipHostFree(e.pin);
            if (e.pin_ctr) (void)hipHostFree(e.pin_ctr);
        }
        if (enq_dev) (void)hipFree(enq_dev);
        if (export_pending) (void)hipEventSynchronize(export_done);  // (an export may still be reading the workspace)
        if (export_done) (void)hipEventDestroy(export_done);
        for (ViewTable& v : vtab) {
            if (v.pending) (void)hipEventSynchronize(v.done);
            if (v.done) (void)hipEventDestroy(v.done);
            if (v.dev) (void)hipFree(v.dev);
            if (v.pin) (void)hipHostFree(v.pin);
        }
        for (void* p : {d_records, d_leaves, d_tri_normals, d_spheres, d_materials, d_tri_leaf, d_paths, (void*)d_queues, hints.mem, order.mem})
            if (p) (void)hipFree(p);
        if (hints.mailbox) (void)hipHostFree(hints.mailbox);
        if (pin_frame) (void)hipHostFree(pin_frame);
        for (hipEvent_t e : {raux.spawned, raux.traced, raux.e0, raux.e1, raux.primary_done, raux.caller, raux.filled})
            if (e) (void)hipEventDestroy(e);
        for (hipStream_t st : {raux.s, raux.copy, raux.fill})
            if (st) (void)hipStreamDestroy(st);
        if (raux.pin_counts) (void)hipHostFree(raux.pin_counts);
        for (auto& r : comb.ring) {
            if (r.host) (void)hipHostFree(r.host);
            if (r.stream) (void)hipStreamDestroy(r.stream);
        }
        for (CallLane* L : lanes_all) {
            for (auto& b : L->dev)
                if (b.p) (void)hipFree(b.p);
            for (auto& b : L->pin)
                if (b.p) (void)hipHostFree(b.p);
            for (void* b : L->bounce)
                if (b) (void)hipHostFree(b);
            for (hipEvent_t e : L->bounce_ev)
                if (e) (void)hipEventDestroy(e);
            if (L->follow) (void)hipEventDestroy(L->follow);
            if (L->d_counters) (void)hipFree(L->d_counters);
            if (L->stream) (void)hipStreamDestroy(L->stream);
            delete L;
        }
        for (WorkSlot& w : work)
            if (w.p) (void)hipFree(w.p);
        for (hipEvent_t e : queue_done)
            if (e) (void)hipEventDestroy(e);
    }
};

#define NEED_DEVICE(s) \
    if ((s)->device < 0) return fail(CGRT_E_NO_DEVICE, "scene was created host-only (CGRT_DEVICE_NONE); there is no CPU traversal path")

#pragma GCC visibility push(hidden)
namespace cgrt {
// ---- capi.cpp
hipError_t staged_h2d(void* dst, const void* src, size_t bytes);

// ---- capi_primary.cpp
void apply_frame_gate(const CgrtScene* s, const CameraDev& C, FrameDev& F);
SoftDev soft_dev(const CgrtSoftShadows& soft, unsigned SL, const float* lights, const float* units);
int views_extent_args(uint32_t nviews, int W, int H);
int raycams_check(const CgrtRayCamera* cams, uint32_t nviews, int W, int H);
int views_args(const void* cams, uint32_t nviews, int W, int H, const CgrtRayCamera* ray = nullptr);
std::vector<uint8_t> view_table(const CgrtCamera* cams, const CgrtRayCamera* raycams, uint32_t nviews);
int launch_with_view_table(CgrtScene* s, const std::vector<uint8_t>& tab, hipStream_t st, const std::function<hipError_t(const void*)>& launch);

// ---- capi_frame_entries.cpp
int check_device_span(const CgrtScene* s, const void* p, uint64_t bytes, const char* name);
int soft_rules(const CgrtSoftShadows* soft);
int aa_args(const CgrtCamera* cam, const void* out, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
            int max_level, int rank, int nranks);
int export_args(const void* out, int W, int H, int format, uint64_t row_bytes, uint64_t* pitch, uint64_t* extent);

// ---- capi_lanes.cpp
void parallel_copy(void* dst, const void* src, size_t bytes);  // large host copies on a few threads
// A call lane of the scene for the duration of one host-pointer call (RAII).
struct LaneGuard {
    CgrtScene* sc;
    CgrtScene::CallLane* L = nullptr;
    explicit LaneGuard(CgrtScene* s) : sc(s) {}
    ~LaneGuard();
    int acquire();
    // scratch that only grows (geometrically): k = 0 rays, 1 hits, 2 normals, 3 light tables, 4 per-query radii
    hipError_t dev(int k, size_t bytes, void** out);
    hipError_t pin(int k, size_t bytes, void** out);
};
extern const size_t kStageBytes;  // transfers up to this size are staged, larger ones go through the bounce buffers
// The transfers of one host-pointer call on a lane: begin; input / scratch per slot (the slots size the lane's buffers, which persist); the
// launch on stream(); output per result; finish.  A result of up to kStageBytes is only staged by output and reaches the caller's memory in
// finish, behind the stream; a larger one is in place when output returns.  An entry that returns early copies nothing.  The primitives
// (capi_prims.cpp) are written with it directly, the queries with QueryCall below.
struct LaneCall {
    LaneGuard g;
    struct Staged {  // by slot; from: the lane's pinned buffer of the slot, or null (nothing pending)
        void *host = nullptr, *from = nullptr;
        size_t bytes = 0;
    } staged[5];
    explicit LaneCall(CgrtScene* s) : g(s) {}
    hipStream_t stream() const { return g.L->stream; }
    int begin();  // the scene's device becomes current, a lane is taken
    hipError_t scratch(int slot, size_t bytes, void** d) { return g.dev(slot, bytes, d); }
    hipError_t input(int slot, const void* host, size_t bytes, void** d);  // scratch + lane_upload
    hipError_t output(int slot, void* host, const void* d, size_t bytes, const CgrtHit* keep = nullptr, size_t stride = 0);  // lane_download, now
    // counted work: zero the first `words` of the lane's counter block, launch with counters(), read them back (complete on return)
    unsigned long long* counters() const { return g.L->d_counters; }
    hipError_t zero_counters(size_t words);
    hipError_t read_counters(uint64_t* out, size_t words);
    hipError_t finish();  // waits for the stream, then copies the staged results out
};
// One query (capi_queries.cpp) in either form, so that an entry is written once.  Host form: the caller's arrays are host memory and the
// call runs on a lane.  Device form: they are device memory, checked as spans and used in place on the caller's stream, which is not
// waited for.  An entry reads: its argument checks; begin; in / out / inout per array, which yield the device pointer either way (every
// span check passes here, before anything is uploaded or launched: a host form's checks are all argument checks); host_in per host
// table; its launch on stream(); finish.  Zero bytes: the array is not used, the device pointer is null (host form) or the caller's.
struct QueryCall {
    LaneCall c;
    const bool device;
    hipStream_t const caller;
    bool on_lane = false;
    struct Result {  // by slot; bytes 0: none
        void *host = nullptr, *d = nullptr;
        size_t bytes = 0;
    } results[5];
    QueryCall(CgrtScene* s, bool device_form, void* stream) : c(s), device(device_form), caller(static_cast<hipStream_t>(stream)) {}
    hipStream_t stream() const { return on_lane ? c.stream() : caller; }
    int begin();  // the scene's device becomes current; host form: a lane is taken
    int in(int slot, const void* p, uint64_t bytes, const char* name, void** d);
    int out(int slot, void* p, uint64_t bytes, const char* name, void** d);    // host form: downloaded by finish
    int inout(int slot, void* p, uint64_t bytes, const char* name, void** d);  // uploaded, and downloaded by finish
    // a table that is host memory in both forms (lights).  A device-form call that has one runs on a lane behind what the caller's stream
    // held (lane_follow), and its finish blocks; call it after the in / out of the caller's arrays
    int host_in(int slot, const void* p, size_t bytes, void** d);
    // counted work (host form only), as LaneCall's; an entry returns after read_counters, without finish
    unsigned long long* counters() const { return c.counters(); }
    int zero_counters(size_t words);
    int read_counters(uint64_t* out, size_t words);
    int finish();  // on a lane: the results in ascending slot order, then LaneCall::finish; else nothing
};
}  // namespace cgrt
#pragma GCC visibility pop
// The lane's transfers.  libcgrt.so has always exported these four under their plain names (they were written inside the extern "C"
// block); its set of dynamic symbols stays exactly what it was, so they keep that linkage and visibility.
extern "C" {
hipError_t lane_bounce(cgrt::LaneGuard& g);
hipError_t lane_upload(cgrt::LaneGuard& g, int k, void* dst, const void* src, size_t bytes);
hipError_t lane_download(cgrt::LaneGuard& g, int k, void* dst, const void* src, size_t bytes, void** staged, const CgrtHit* keep = nullptr,
                         size_t stride = 0);
hipError_t lane_follow(cgrt::LaneGuard& g, hipStream_t stream);
}
