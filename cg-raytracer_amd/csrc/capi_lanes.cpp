// capi_lanes.cpp -- the call lanes of the host-pointer entries (CgrtScene::CallLane): a lane for the duration of a call, its transfers,
// and the one helper every such entry is written with (LaneCall).
#include "capi_internal.h"

namespace cgrt {
LaneGuard::~LaneGuard() {
    if (!L) return;
    // An entry that returns early (an error after work was queued) must not leave copies in flight into its caller's
    // memory or hand a busy lane's staging buffers to the next caller: a finished stream answers the query at once.
    if (hipSetDevice(sc->device) == hipSuccess && hipStreamQuery(L->stream) != hipSuccess) (void)hipStreamSynchronize(L->stream);
    std::lock_guard<std::mutex> lk(sc->lanes_mutex);
    sc->lanes_free.push_back(L);
}
int LaneGuard::acquire() {
    {
        std::lock_guard<std::mutex> lk(sc->lanes_mutex);
        if (!sc->lanes_free.empty()) {
            L = sc->lanes_free.back();
            sc->lanes_free.pop_back();
            return CGRT_OK;
        }
    }
    CgrtScene::CallLane* n = new (std::nothrow) CgrtScene::CallLane();
    if (!n) return fail(CGRT_E_ALLOC, "host allocation failed");
    hipError_t e = hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&n->d_counters, 8 * sizeof(unsigned long long));
    if (e != hipSuccess) {
        if (n->stream) (void)hipStreamDestroy(n->stream);
        delete n;
        return hip_fail(e, "creating a call lane");
    }
    {
        std::lock_guard<std::mutex> lk(sc->lanes_mutex);
        sc->lanes_all.push_back(n);
    }
    L = n;
    return CGRT_OK;
}
hipError_t LaneGuard::dev(int k, size_t bytes, void** out) {
    auto& b = L->dev[k];
    if (b.cap < bytes) {
        if (b.p) (void)hipFree(b.p);
        b.p = nullptr;
        b.cap = 0;
        const size_t want = std::max<size_t>(bytes, 4096) * 3 / 2;
        const hipError_t e = hipMalloc(&b.p, want);
        if (e != hipSuccess) return e;
        b.cap = want;
    }
    *out = b.p;
    return hipSuccess;
}
hipError_t LaneGuard::pin(int k, size_t bytes, void** out) {
    auto& b = L->pin[k];
    if (b.cap < bytes) {
        if (b.p) (void)hipHostFree(b.p);
        b.p = nullptr;
        b.cap = 0;
        const size_t want = std::max<size_t>(bytes, 4096) * 3 / 2;
        const hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        b.cap = want;
    }
    *out = b.p;
    return hipSuccess;
}
// large host copies on a few threads (one thread moves ~10 GB/s: a 1080p float frame would take as long as 8 device frames)
void parallel_copy(void* dst, const void* src, size_t bytes) {
    const size_t chunk = 2u << 20;
    if (bytes < 2 * chunk) {
        std::memcpy(dst, src, bytes);
        return;
    }
    const unsigned nt = (unsigned)std::min<size_t>(4, bytes / chunk);
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt; t++)
        pool.emplace_back([=] {
            const size_t b = bytes * t / nt, e = bytes * (t + 1) / nt;
            std::memcpy(static_cast<char*>(dst) + b, static_cast<const char*>(src) + b, e - b);
        });
    std::memcpy(dst, src, bytes / nt);
    for (std::thread& th : pool) th.join();
}

// Transfers below this size go through the lane's pinned staging buffers (a pageable hipMemcpyAsync of a few bytes costs
// far more than copying them twice).  Larger ones -- the lists of a host-driven wavefront, whole frames -- are cut into
// kBounceBytes pieces that alternate between two pinned buffers: the host copies piece k+1 (on a few threads) while the DMA engine
// moves piece k.  Handing the runtime a pageable pointer instead moved ~3 GB/s (66 MB of rays + 56 MB of hits and normals for a
// 1080p list: 40-50 ms around a 0.3 ms kernel, profiles/r3_host_mirror.txt).
const size_t kStageBytes = 1u << 20;
const size_t kBounceBytes = 8u << 20;
}  // namespace cgrt

extern "C" {  // (the transfers keep the C names the library has always exported them under: capi_internal.h)
hipError_t lane_bounce(LaneGuard& g) {
    for (int b = 0; b < 2; b++) {
        if (!g.L->bounce[b]) {
            const hipError_t e = hipHostMalloc(&g.L->bounce[b], kBounceBytes, hipHostMallocDefault);
            if (e != hipSuccess) return e;
        }
        if (!g.L->bounce_ev[b]) {
            const hipError_t e = hipEventCreateWithFlags(&g.L->bounce_ev[b], hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

// host -> device on the lane's stream
hipError_t lane_upload(LaneGuard& g, int k, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    if (bytes <= kStageBytes) {
        void* st = nullptr;
        const hipError_t e = g.pin(k, bytes, &st);
        if (e != hipSuccess) return e;
        std::memcpy(st, src, bytes);
        return hipMemcpyAsync(dst, st, bytes, hipMemcpyHostToDevice, g.L->stream);
    }
    hipError_t e = lane_bounce(g);
    if (e != hipSuccess) return e;
    size_t piece = 0;
    for (size_t off = 0; off < bytes; off += kBounceBytes, piece++) {
        const int b = (int)(piece & 1);
        const size_t m = std::min(kBounceBytes, bytes - off);
        if (piece >= 2 && (e = hipEventSynchronize(g.L->bounce_ev[b])) != hipSuccess) return e;  // the DMA out of this half has finished
        parallel_copy(g.L->bounce[b], static_cast<const char*>(src) + off, m);
        if ((e = hipMemcpyAsync(static_cast<char*>(dst) + off, g.L->bounce[b], m, hipMemcpyHostToDevice, g.L->stream)) != hipSuccess) return e;
        if ((e = hipEventRecord(g.L->bounce_ev[b], g.L->stream)) != hipSuccess) return e;
    }
    // the halves are reused by the next transfer of this call: it must not overwrite a piece still being read
    for (int b = 0; b < 2; b++)
        if ((e = hipEventSynchronize(g.L->bounce_ev[b])) != hipSuccess) return e;
    return hipSuccess;
}
// device -> host.  Small: returns the pinned address to copy from after the stream has been synchronised.  Large: the data is in
// dst when the call returns (the stream's earlier work has been waited for), *staged stays null.  `keep` (optional, large path
// only): one flag word per `stride` bytes -- elements whose word is zero are NOT written (normals of rays that missed).
hipError_t lane_download(LaneGuard& g, int k, void* dst, const void* src, size_t bytes, void** staged, const CgrtHit* keep,
                         size_t stride) {
    *staged = nullptr;
    if (bytes == 0) return hipSuccess;
    if (bytes <= kStageBytes && !keep) {
        void* st = nullptr;
        const hipError_t e = g.pin(k, bytes, &st);
        if (e != hipSuccess) return e;
        *staged = st;
        return hipMemcpyAsync(st, src, bytes, hipMemcpyDeviceToHost, g.L->stream);
    }
    hipError_t e = lane_bounce(g);
    if (e != hipSuccess) return e;
    const size_t piece_bytes = stride ? kBounceBytes / stride * stride : kBounceBytes;
    const size_t npieces = (bytes + piece_bytes - 1) / piece_bytes;
    for (size_t piece = 0; piece <= npieces; piece++) {
        if (piece < npieces) {
            const int b = (int)(piece & 1);
            const size_t off = piece * piece_bytes, m = std::min(piece_bytes, bytes - off);
            if ((e = hipMemcpyAsync(g.L->bounce[b], static_cast<const char*>(src) + off, m, hipMemcpyDeviceToHost, g.L->stream)) != hipSuccess) return e;
            if ((e = hipEventRecord(g.L->bounce_ev[b], g.L->stream)) != hipSuccess) return e;
        }
        if (piece >= 1) {  // copy the previous piece out while this one is on the wire
            const int b = (int)((piece - 1) & 1);
            const size_t off = (piece - 1) * piece_bytes, m = std::min(piece_bytes, bytes - off);
            if ((e = hipEventSynchronize(g.L->bounce_ev[b])) != hipSuccess) return e;
            if (!keep) {
                parallel_copy(static_cast<char*>(dst) + off, g.L->bounce[b], m);
            } else {
                const size_t first = off / stride, cnt = m / stride;
                const unsigned nt = cnt >= 65536 ? 4 : 1;
                auto part = [&](unsigned t) {
                    const char* from = static_cast<const char*>(g.L->bounce[b]);
                    char* to = static_cast<char*>(dst) + off;
                    for (size_t i = cnt * t / nt, e2 = cnt * (t + 1) / nt; i < e2; i++)
                        if (keep[first + i].hit) std::memcpy(to + i * stride, from + i * stride, stride);
                };
                std::vector<std::thread> pool;
                for (unsigned t = 1; t < nt; t++) pool.emplace_back(part, t);
                part(0);
                for (std::thread& th : pool) th.join();
            }
        }
    }
    return hipSuccess;
}
// The device forms that read the caller's host light tables run on a call lane, behind everything queued on `stream` before the call (an
// event on `stream` that the lane's stream waits for); they return when the answers are in place.
hipError_t lane_follow(LaneGuard& g, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (!g.L->follow && (e = hipEventCreateWithFlags(&g.L->follow, hipEventDisableTiming)) != hipSuccess) return e;
    if ((e = hipEventRecord(g.L->follow, stream)) != hipSuccess) return e;
    return hipStreamWaitEvent(g.L->stream, g.L->follow, 0);
}
}  // extern "C"

namespace cgrt {
int LaneCall::begin() {
    HIP_TRY(hipSetDevice(g.sc->device));
    return g.acquire();
}
hipError_t LaneCall::input(int slot, const void* host, size_t bytes, void** d) {
    const hipError_t e = g.dev(slot, bytes, d);
    return e != hipSuccess ? e : lane_upload(g, slot, *d, host, bytes);
}
hipError_t LaneCall::output(int slot, void* host, const void* d, size_t bytes, const CgrtHit* keep, size_t stride) {
    staged[slot] = {host, nullptr, bytes};
    return lane_download(g, slot, host, d, bytes, &staged[slot].from, keep, stride);
}
hipError_t LaneCall::zero_counters(size_t words) { return hipMemsetAsync(g.L->d_counters, 0, words * sizeof(unsigned long long), g.L->stream); }
hipError_t LaneCall::read_counters(uint64_t* out, size_t words) {
    unsigned long long h[8];
    hipError_t e = hipMemcpyAsync(h, g.L->d_counters, words * sizeof(h[0]), hipMemcpyDeviceToHost, g.L->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.L->stream);
    for (size_t i = 0; e == hipSuccess && i < words; i++) out[i] = h[i];
    return e;
}
hipError_t LaneCall::finish() {
    const hipError_t e = hipStreamSynchronize(g.L->stream);
    for (const Staged& s : staged)
        if (e == hipSuccess && s.from) std::memcpy(s.host, s.from, s.bytes);
    return e;
}

int QueryCall::begin() {
    HIP_TRY(hipSetDevice(c.g.sc->device));
    if (device) return CGRT_OK;
    on_lane = true;
    return c.g.acquire();
}
int QueryCall::in(int slot, const void* p, uint64_t bytes, const char* name, void** d) {
    *d = device ? const_cast<void*>(p) : nullptr;
    if (device) return check_device_span(c.g.sc, p, bytes, name);
    if (bytes) HIP_TRY(c.input(slot, p, bytes, d));
    return CGRT_OK;
}
int QueryCall::out(int slot, void* p, uint64_t bytes, const char* name, void** d) {
    *d = device ? p : nullptr;
    if (device) return check_device_span(c.g.sc, p, bytes, name);
    if (bytes) HIP_TRY(c.scratch(slot, bytes, d));
    results[slot] = {p, *d, (size_t)bytes};
    return CGRT_OK;
}
int QueryCall::inout(int slot, void* p, uint64_t bytes, const char* name, void** d) {
    CGRT_TRY(in(slot, p, bytes, name, d));
    if (!device) results[slot] = {p, *d, (size_t)bytes};
    return CGRT_OK;
}
int QueryCall::host_in(int slot, const void* p, size_t bytes, void** d) {
    if (!on_lane) {
        CGRT_TRY(c.g.acquire());
        on_lane = true;
        HIP_TRY(lane_follow(c.g, caller));
    }
    HIP_TRY(c.input(slot, p, bytes, d));
    return CGRT_OK;
}
int QueryCall::zero_counters(size_t words) {
    HIP_TRY(c.zero_counters(words));
    return CGRT_OK;
}
int QueryCall::read_counters(uint64_t* out, size_t words) {
    HIP_TRY(c.read_counters(out, words));
    return CGRT_OK;
}
int QueryCall::finish() {
    if (!on_lane) return CGRT_OK;
    for (int k = 0; k < 5; k++)
        if (results[k].bytes) HIP_TRY(c.output(k, results[k].host, results[k].d, results[k].bytes));
    HIP_TRY(c.finish());
    return CGRT_OK;
}
}  // namespace cgrt
