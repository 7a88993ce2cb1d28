// capi_combine.cpp -- the C-ABI's intersect entries for ray lists (cgrt_intersect_batch*, cgrt_count_batch) and the call combiner that
// serves cgrt_intersect_batch's calls of a few rays from many threads (CgrtScene::Combiner, capi_internal.h).
#include "capi_internal.h"

// (the combiner's helpers sit inside the block as they always have: libcgrt.so exports combined_intersect and usable_cpus under their
// plain names, and its set of dynamic symbols stays exactly what it was)
extern "C" {

int cgrt_intersect_batch_device(CgrtScene* s, const CgrtRay* d_rays, uint64_t n, CgrtHit* d_hits, float* d_normals, void* stream) {
    if (!s || (n && (!d_rays || !d_hits))) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_trace_batch(s->dev, RayList{reinterpret_cast<const float*>(d_rays), n, reinterpret_cast<CgrtHitDev*>(d_hits), d_normals}, nullptr,
                               static_cast<hipStream_t>(stream)));
    return CGRT_OK;
}

namespace {
// CPUs this process may use: the affinity mask, cut to the cgroup's quota when /sys/fs/cgroup/cpu.max states one (a container that
// shows 256 hardware threads and grants 16 CPUs throttles a process whose 64 threads all spin).
int usable_cpus() {
    static const int n = [] {
        cpu_set_t set;
        int c = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
        if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
            long long quota = 0, period = 0;
            if (std::fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) c = std::min<long long>(c, (quota + period - 1) / period);
            std::fclose(f);
        }
        return std::max(1, c);
    }();
    return n;
}
inline void futex_wait(std::atomic<uint32_t>& word, uint32_t expected) {  // returns at once when the word no longer holds `expected`
    (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&word), FUTEX_WAIT_PRIVATE, expected, nullptr, nullptr, 0);
}
inline void futex_wake_all(std::atomic<uint32_t>& word) {
    (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&word), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}
inline void cpu_relax(unsigned& spins) {  // a wait of a few microseconds is the common case: spin first, then give the core away
    if (++spins < 4096)
        __builtin_ia32_pause();
    else
        std::this_thread::yield();
}
// Returns 1 when the call was served by a combined generation (rc_out = its status), 0 when the caller should take the direct path.
int combined_intersect(CgrtScene* s, const CgrtRay* rays, uint32_t n, CgrtHit* hits, float* normals, int& rc_out) {
    typedef CgrtScene::Combiner C;
    C& cb = s->comb;
    const size_t off_hits = sizeof(CgrtRay) * C::CAP, off_nrm = off_hits + sizeof(CgrtHit) * C::CAP, total = off_nrm + 12 * (size_t)C::CAP;
    int rdy = cb.ready.load(std::memory_order_acquire);
    if (rdy == 0) {  // first call on this scene: the two rings
        std::lock_guard<std::mutex> lk(cb.init_mu);
        rdy = cb.ready.load(std::memory_order_acquire);
        if (rdy == 0) {
            bool ok = hipSetDevice(s->device) == hipSuccess;
            if (const char* e = getenv("CGRT_COMBINE_NRINGS")) cb.nrings = std::max(1, std::min(atoi(e), (int)C::NRINGS));
            for (int k = 0; k < cb.nrings; k++) {
                C::Ring& r = cb.ring[k];
                if (!ok) break;
                hipError_t e = hipHostMalloc(&r.host, total + 64, hipHostMallocMapped);  // (+ the completion word)
                if (e == hipSuccess) std::memset(static_cast<char*>(r.host) + total, 0, 64);
                if (e == hipSuccess) e = hipHostGetDevicePointer(&r.dev, r.host, 0);
                if (e == hipSuccess) e = hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking);
                ok = e == hipSuccess;  // (whatever was allocated is released with the scene)
            }
            rdy = ok ? 1 : -1;
            cb.ready.store(rdy, std::memory_order_release);
        }
    }
    if (rdy < 0) return 0;
    struct Inside {
        std::atomic<int>& c;
        int before;
        explicit Inside(std::atomic<int>& x) : c(x), before(c.fetch_add(1, std::memory_order_relaxed)) {}
        ~Inside() { c.fetch_sub(1, std::memory_order_relaxed); }
    } inside(cb.inside);
    if (inside.before >= C::MAX_CALLERS) return 0;  // (the bound the word's bit fields and JOIN_MAX rely on)
    // How a caller waits.  With a CPU for every caller, spinning is the fastest hand-over (8 callers: 0.45 M calls/s).  With more
    // callers than CPUs the spinners take the CPUs from the callers that have work to do -- and inside a CPU quota they get the
    // whole process throttled -- so then a caller spins for a moment only and sleeps on a futex; whoever publishes what the
    // sleepers wait for wakes them.  CGRT_COMBINE_SLEEP=0 / 1 forces one or the other.
    static const int sleep_env = [] {
        const char* e = getenv("CGRT_COMBINE_SLEEP");
        return e ? atoi(e) : -1;
    }();
    const bool sleepy = sleep_env >= 0 ? sleep_env != 0 : inside.before + 1 > usable_cpus();
    static const unsigned spin_first = [] {  // pauses before a sleepy caller goes to sleep (a few microseconds)
        const char* e = getenv("CGRT_COMBINE_SPIN");
        return e ? (unsigned)atoi(e) : 20u;
    }();
    // ---- join the open generation, or open a free ring (and lead it) ----
    const int NR = cb.nrings;
    int b = -1;
    uint32_t at = 0;
    uint32_t gen = 0;
    bool leader = false;
    unsigned spins = 0;
    while (b < 0) {
        const uint32_t epoch = cb.epoch.load(std::memory_order_seq_cst);  // (read BEFORE the rings are looked at)
        for (int k = 0; k < NR && b < 0; k++) {
            C::Ring& r = cb.ring[k];
            const uint64_t seen = r.word.load(std::memory_order_acquire);
            if (C::st_of(seen) != C::OPEN || C::count_of(seen) > C::JOIN_MAX) continue;
            const uint64_t w = r.word.fetch_add(((uint64_t)1 << 2) | ((uint64_t)n << 16), std::memory_order_acq_rel);
            if (C::st_of(w) == C::OPEN) {  // joined: the slots [count, count + n) are this caller's
                b = k;
                at = C::count_of(w);
                gen = (uint32_t)(w >> 32);
            }  // else: closed in between -- the stray counts are harmless (see Combiner)
        }
        for (int k = 0; k < NR && b < 0; k++) {
            C::Ring& r = cb.ring[k];
            uint64_t w = r.word.load(std::memory_order_acquire);
            if (C::st_of(w) != C::FREE) continue;
            // (copied == 0 and readers == 0 here: the last reader of the previous generation reset them before it freed the ring)
            if (r.word.compare_exchange_strong(w, C::pack(C::OPEN, 1u, n, w >> 32), std::memory_order_acq_rel, std::memory_order_acquire)) {
                b = k;
                at = 0;
                gen = (uint32_t)(w >> 32);
                leader = true;
            }
        }
        if (b >= 0) break;
        // both rings are on the GPU or being read out: the next generation opens in a moment
        if (sleepy && ++spins > spin_first) {
            bool open = false;  // an OPEN ring that is merely full does not announce itself: keep polling while there is one
            for (int k = 0; k < NR; k++) open |= C::st_of(cb.ring[k].word.load(std::memory_order_relaxed)) == C::OPEN;
            if (!open) {
                cb.epoch_sleepers.fetch_add(1, std::memory_order_seq_cst);
                futex_wait(cb.epoch, epoch);  // until a ring has been set free since `epoch` was read
                cb.epoch_sleepers.fetch_sub(1, std::memory_order_relaxed);
                continue;
            }
        }
        cpu_relax(spins);
    }
    C::Ring& r = cb.ring[b];
    std::memcpy(static_cast<char*>(r.host) + sizeof(CgrtRay) * (size_t)at, rays, sizeof(CgrtRay) * (size_t)n);
    r.copied.fetch_add(1, std::memory_order_release);
    if (leader) {
        // a short grace period while other callers are on their way in (callers parked on the other ring are not coming)
        // -- until everybody inside the entry has joined, or nobody new has for a moment; a few microseconds at most
        uint32_t last = 0, quiet = 0;
        for (unsigned k = 0; k < 1000; k++) {
            int parked = 0;
            for (int k = 0; k < NR; k++) {
                if (k == b) continue;
                const uint64_t ow = cb.ring[k].word.load(std::memory_order_relaxed);
                if (C::st_of(ow) == C::RUNNING || C::st_of(ow) == C::DONE) parked += (int)cb.ring[k].readers.load(std::memory_order_relaxed);
            }
            const uint32_t j = C::joined_of(r.word.load(std::memory_order_relaxed));
            if ((int)j + parked >= cb.inside.load(std::memory_order_relaxed)) break;
            if (j != last) {
                last = j;
                quiet = 0;
            } else if (++quiet > 100) {
                break;
            }
            __builtin_ia32_pause();
        }
        // close: OPEN -> RUNNING fixes the number of rays and of joiners in one step
        uint64_t w = r.word.load(std::memory_order_acquire);
        while (!r.word.compare_exchange_weak(w, C::pack(C::RUNNING, C::joined_of(w), C::count_of(w), w >> 32), std::memory_order_acq_rel,
                                            std::memory_order_acquire)) {
        }
        const uint32_t cnt = C::count_of(w), joined = C::joined_of(w);
        r.readers.store(joined, std::memory_order_relaxed);
        const auto t_closed = std::chrono::steady_clock::now();
        cb.n_gen.fetch_add(1, std::memory_order_relaxed);
        cb.n_rays.fetch_add(cnt, std::memory_order_relaxed);
        for (uint64_t m = cb.max_gen.load(std::memory_order_relaxed); m < cnt && !cb.max_gen.compare_exchange_weak(m, cnt, std::memory_order_relaxed);) {
        }
        unsigned sp = 0;
        while (r.copied.load(std::memory_order_acquire) != joined) cpu_relax(sp);  // every joiner's rays are in the ring
        int rc = CGRT_OK;
        hipError_t e = hipSetDevice(s->device);
        if (e == hipSuccess)
            e = launch_trace_batch(s->dev, RayList{static_cast<const float*>(r.dev), cnt, reinterpret_cast<CgrtHitDev*>(static_cast<char*>(r.dev) + off_hits),
                                                   reinterpret_cast<float*>(static_cast<char*>(r.dev) + off_nrm)}, nullptr, r.stream);
        cb.ns_launch.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_closed).count(),
                               std::memory_order_relaxed);
        if (e == hipSuccess) {
            // How the leader waits.  Sleeping in hipStreamSynchronize serialises the two rings: while one leader sleeps there the
            // other leader's launch call does not return (64 callers: 35 of a generation's 61 us were spent getting the launch
            // out, 2.3 us for a lone caller; profiles/r3_per_ray.txt), and polling hipStreamQuery is worse still.  So a one-thread
            // kernel behind the batch writes the generation's number into the ring's pinned memory and the leader watches that
            // word: no runtime call while it waits.  (A launch that never signals -- a fault -- is caught by the bounded spin:
            // the leader then asks the runtime.)  CGRT_COMBINE_WAIT=1: hipStreamSynchronize, =0: hipStreamQuery polling.
            static const int wait_mode = [] {
                const char* w = getenv("CGRT_COMBINE_WAIT");
                return w ? atoi(w) : 2;
            }();
            if (wait_mode == 1) {
                e = hipStreamSynchronize(r.stream);
            } else if (wait_mode == 0) {
                while ((e = hipStreamQuery(r.stream)) == hipErrorNotReady)
                    for (int k = 0; k < 32; k++) __builtin_ia32_pause();
            } else {
                volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(static_cast<char*>(r.host) + total);
                uint32_t* dflag = reinterpret_cast<uint32_t*>(static_cast<char*>(r.dev) + total);
                const uint32_t token = gen + 1u;  // (the word holds the previous generation's token, never this one's)
                e = launch_signal(dflag, token, r.stream);
                if (e == hipSuccess) {
                    unsigned long long spins = 0;
                    while (*flag != token) {
                        __builtin_ia32_pause();
                        if (++spins > 200000000ull) {  // seconds: something is wrong with the launch -- let the runtime say what
                            e = hipStreamSynchronize(r.stream);
                            break;
                        }
                    }
                    std::atomic_thread_fence(std::memory_order_acquire);
                }
            }
        }
        if (e != hipSuccess) {
            rc = CGRT_E_HIP;
            r.err = std::string("combined launch: ") + hipGetErrorString(e);
        }
        r.rc = rc;
        cb.ns_gpu.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_closed).count(),
                            std::memory_order_relaxed);
        r.word.store(C::pack(C::DONE, joined, cnt, gen), std::memory_order_release);
        r.done_gen.store(gen + 1u, std::memory_order_seq_cst);
        if (cb.done_sleepers.load(std::memory_order_seq_cst) > 0) futex_wake_all(r.done_gen);
    } else {
        unsigned sp = 0;
        for (;;) {
            const uint32_t dg = r.done_gen.load(std::memory_order_seq_cst);
            if ((int32_t)(dg - gen) > 0) break;
            if (sleepy && ++sp > spin_first) {
                cb.done_sleepers.fetch_add(1, std::memory_order_seq_cst);
                futex_wait(r.done_gen, dg);  // (returns at once if the leader has published in between)
                cb.done_sleepers.fetch_sub(1, std::memory_order_relaxed);
            } else {
                cpu_relax(sp);
            }
        }
    }
    rc_out = r.rc;
    if (r.rc == CGRT_OK) {
        const CgrtHit* rh = reinterpret_cast<const CgrtHit*>(static_cast<char*>(r.host) + off_hits) + at;
        const float* rn = reinterpret_cast<const float*>(static_cast<char*>(r.host) + off_nrm) + 3 * (size_t)at;
        std::memcpy(hits, rh, sizeof(CgrtHit) * (size_t)n);
        if (normals)
            for (uint32_t i = 0; i < n; i++)
                if (rh[i].hit) std::memcpy(normals + 3 * (size_t)i, rn + 3 * (size_t)i, 12);  // HitInfo stays untouched on a miss
    } else {
        g_err = r.err;
    }
    if (r.readers.fetch_sub(1, std::memory_order_acq_rel) == 1) {  // last one out: the ring is free for generation gen + 1
        r.copied.store(0, std::memory_order_relaxed);
        r.word.store(C::pack(C::FREE, 0, 0, (uint64_t)(gen + 1u)), std::memory_order_release);
        cb.epoch.fetch_add(1, std::memory_order_seq_cst);
        if (cb.epoch_sleepers.load(std::memory_order_seq_cst) > 0) futex_wake_all(cb.epoch);
    }
    return 1;
}
}  // namespace

int cgrt_debug_combiner_stats(const CgrtScene* s, uint64_t* out4) {  // (five words, see include/cgrt.h)
    if (!s || !out4) return fail(CGRT_E_ARG, "NULL argument");
    out4[0] = s->comb.n_gen.load();
    out4[1] = s->comb.n_rays.load();
    out4[2] = s->comb.max_gen.load();
    out4[3] = s->comb.ns_gpu.load();
    out4[4] = s->comb.ns_launch.load();
    return CGRT_OK;
}
int cgrt_set_call_combining(int enabled) {
    g_call_combining.store(enabled ? 1 : 0);
    return CGRT_OK;
}

int cgrt_intersect_batch(CgrtScene* s, const CgrtRay* rays, uint64_t n, CgrtHit* hits, float* normals) {
    if (!s || (n && (!rays || !hits))) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    if (n == 0) return CGRT_OK;
    if (n <= CgrtScene::Combiner::MAX_N && g_call_combining.load(std::memory_order_relaxed)) {
        static const bool env_off = [] {
            const char* e = getenv("CGRT_COMBINE");  // experiment knob: 0 = every call takes the direct path
            return e && e[0] == '0';
        }();
        int rc = CGRT_OK;
        if (!env_off && combined_intersect(s, rays, (uint32_t)n, hits, normals, rc)) return rc;
    }
    LaneCall c(s);
    int rc = c.begin();
    if (rc) return rc;
    void *dr, *dh, *dn = nullptr;
    HIP_TRY(c.input(0, rays, n * sizeof(CgrtRay), &dr));
    HIP_TRY(c.scratch(1, n * sizeof(CgrtHit), &dh));
    // HitInfo is left untouched on a miss (the kernels write a normal only with a hit): a short list starts from the caller's
    // contents on the device; of a long one only the normals of rays that hit are copied back (lane_download's `keep`)
    const bool big = n * sizeof(CgrtHit) > kStageBytes;
    if (normals) HIP_TRY(big ? c.scratch(2, n * 12, &dn) : c.input(2, normals, n * 12, &dn));
    rc = cgrt_intersect_batch_device(s, static_cast<const CgrtRay*>(dr), n, static_cast<CgrtHit*>(dh), static_cast<float*>(dn), c.stream());
    if (rc) return rc;
    HIP_TRY(c.output(1, hits, dh, n * sizeof(CgrtHit)));
    if (normals) HIP_TRY(c.output(2, normals, dn, n * 12, big ? hits : nullptr, 12));  // big: hits is complete here, only rays that hit
    HIP_TRY(c.finish());
    return CGRT_OK;
}

int cgrt_intersect_brute_batch(CgrtScene* s, const CgrtRay* rays, uint64_t n, int mesh, CgrtHit* hits, float* normals) {
    if (!s || (n && (!rays || !hits))) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    if (mesh >= (int)s->nmesh) return fail(CGRT_E_ARG, "mesh index out of range");
    if (n == 0) return CGRT_OK;
    LaneCall c(s);
    int rc = c.begin();
    if (rc) return rc;
    void *dr, *dh, *dn = nullptr;
    HIP_TRY(c.input(0, rays, n * sizeof(CgrtRay), &dr));
    HIP_TRY(c.scratch(1, n * sizeof(CgrtHit), &dh));
    const bool big = n * sizeof(CgrtHit) > kStageBytes;  // as cgrt_intersect_batch
    if (normals) HIP_TRY(big ? c.scratch(2, n * 12, &dn) : c.input(2, normals, n * 12, &dn));
    HIP_TRY(launch_brute_batch(s->dev, static_cast<const float*>(dr), n, mesh < 0 ? -1 : mesh, static_cast<CgrtHitDev*>(dh), static_cast<float*>(dn),
                               c.stream()));
    HIP_TRY(c.output(1, hits, dh, n * sizeof(CgrtHit)));
    if (normals) HIP_TRY(c.output(2, normals, dn, n * 12, big ? hits : nullptr, 12));  // big: hits is complete here, only rays that hit
    HIP_TRY(c.finish());
    return CGRT_OK;
}

int cgrt_count_batch(CgrtScene* s, const CgrtRay* rays, uint64_t n, CgrtCounters* out) {
    if (!s || !out || (n && !rays)) return fail(CGRT_E_ARG, "NULL argument");
    NEED_DEVICE(s);
    LaneCall c(s);
    int rc = c.begin();
    if (rc) return rc;
    void *dr, *dh;
    HIP_TRY(c.input(0, rays, n * sizeof(CgrtRay), &dr));
    HIP_TRY(c.scratch(1, n * sizeof(CgrtHit), &dh));
    HIP_TRY(c.zero_counters(8));
    HIP_TRY(launch_trace_batch(s->dev, RayList{static_cast<const float*>(dr), n, static_cast<CgrtHitDev*>(dh), nullptr}, c.counters(), c.stream()));
    HIP_TRY(c.read_counters(&out->rays, 8));
    return CGRT_OK;
}

}  // extern "C"
