// capi.cpp -- implementation of the C-ABI declared in include/cgrt.h: what every unit of it shares (errors, options, frames, uploads)
// and the scene's life cycle, info and layout entries.  The other entries: capi_combine.cpp (per-ray and batch intersect),
// capi_primary.cpp (primary frames), capi_frames.cpp and capi_frame_entries.cpp (shaded frames), capi_multi.cpp (replicas),
// capi_queries.cpp, capi_prims.cpp; capi_lanes.cpp has the call lanes.
// Host C++ over the HIP runtime; no torch types, no CPU traversal path: every intersect/trace entry
// launches the gfx950 kernels of trace_kernels.hip and fails loudly when no device is usable.
#include "capi_internal.h"

static_assert(sizeof(CgrtRay) == 28, "CgrtRay must match the reference Ray (ray.h:9-13)");
static_assert(sizeof(CgrtHit) == sizeof(CgrtHitDev), "CgrtHit layout");
static_assert(sizeof(CgrtCounters) == 8 * sizeof(uint64_t), "CgrtCounters is a lane's counter block, word for word (LaneCall::read_counters)");

namespace {

// Process-wide options (cgrt_set_leaf_accel / cgrt_set_fast_tree / cgrt_set_primary_mode).  The build options are copied
// under a mutex when a scene is created; the primary mode is read atomically by every launch.
std::mutex g_options_mutex;
BuildOptions g_build_options;
}  // namespace

namespace cgrt {  // (declared in capi_internal.h, for every translation unit of the C-ABI)
thread_local std::string g_err;
std::atomic<int> g_call_combining{1};  // cgrt_set_call_combining
std::atomic<int> g_render_predict{1};  // cgrt_set_render_prediction
std::atomic<int> g_frame_hints{-1};    // cgrt_set_frame_hints: -1 auto, 0 off, 1 hard tiles first, 2 hard tiles 16 rays per wave
std::atomic<unsigned> g_hint_thr_dense{0}, g_hint_thr_sparse{0};  // cgrt_debug_set_hint_thresholds (0: the defaults)
std::atomic<int> g_frame_order{-1};    // cgrt_set_frame_order: -1 = the library's policy (on), 0 = off, 1 = on wherever a frame qualifies
std::atomic<int> g_frame_gate{1};      // cgrt_set_frame_gate: 1 = tiles outside the root box's screen rectangle skip their rays, 0 = off
std::atomic<int> g_primary_mode{0};  // 0 = one wave per tile, 1 = persistent waves with lane refill

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return CGRT_E_HIP;
}

int select_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(CGRT_E_NO_DEVICE, std::string("no HIP device available (") + hipGetErrorString(e) + ")");
    if (device < 0 || device >= n) return fail(CGRT_E_NO_DEVICE, "device index " + std::to_string(device) + " out of range");
    HIP_TRY(hipSetDevice(device));
    return CGRT_OK;
}

// Ray-independent part of Trackball::generateRay / position (trackball.cpp:70-73, :92-103),
// glm::qua(eulerAngles) as in glm 0.9.9.8 type_quat.inl.
CameraDev make_camera(const CgrtCamera& c) {
    const float hx = c.euler[0] * 0.5f, hy = c.euler[1] * 0.5f, hz = c.euler[2] * 0.5f;
    const float cx = std::cos(hx), cy = std::cos(hy), cz = std::cos(hz);
    const float sx = std::sin(hx), sy = std::sin(hy), sz = std::sin(hz);
    Q4 q;
    q.w = cx * cy * cz + sx * sy * sz;
    q.x = sx * cy * cz - cx * sy * sz;
    q.y = cx * sy * cz + sx * cy * sz;
    q.z = cx * cy * sz - sx * sy * cz;
    const F3 p = add(f3(c.look_at[0], c.look_at[1], c.look_at[2]), quat_rotate(q, f3(0.0f, 0.0f, -c.distance)));
    CameraDev d;
    d.pos[0] = p.x;
    d.pos[1] = p.y;
    d.pos[2] = p.z;
    d.q[0] = q.w;
    d.q[1] = q.x;
    d.q[2] = q.y;
    d.q[3] = q.z;
    d.half_h = std::tan(c.fovy / 2.0f);
    d.half_w = c.aspect * d.half_h;
    return d;
}

bool make_frame(int W, int H, int x0, int y0, int x1, int y1, int rank, int nranks, int block, FrameDev& F) {
    if (W <= 0 || H <= 0 || x0 < 0 || y0 < 0 || x1 > W || y1 > H || x0 > x1 || y0 > y1 || nranks <= 0 || rank < 0 || rank >= nranks)
        return false;
    F.W = W;
    F.H = H;
    F.x0 = x0;
    F.y0 = y0;
    F.x1 = x1;
    F.y1 = y1;
    F.tiles_x = (x1 - x0 + 7) / 8;
    F.tiles_y = (y1 - y0 + 7) / 8;
    F.st_x = (F.tiles_x + ST_TILES - 1) / ST_TILES;
    F.st_y = (F.tiles_y + ST_TILES - 1) / ST_TILES;
    F.rank = rank;
    F.nranks = nranks;
    const uint64_t nst = (uint64_t)F.st_x * (uint64_t)F.st_y;
    F.nst_rank = (uint32_t)((nst + (uint64_t)nranks - 1 - (uint64_t)rank) / (uint64_t)nranks);
    F.block = block;
    F.nblocks = ((F.nst_rank + 7u) / 8u) * 8u * (64u / ((uint32_t)block / 64u));
    F.packed = 0;
    F.hint = nullptr;
    F.hint_blocks = F.hint_rgen = F.hint_wgen = 0;
    F.views = nullptr;
    F.view_st = 0;
    F.gate_x0 = F.gate_y0 = F.gate_x1 = F.gate_y1 = 0;  // no gate (apply_frame_gate)
    F.order = nullptr;
    return true;
}

// A multi-view frame (FrameDev::views): nviews whole W x H frames, one rank, their super-tiles one list (the table is set by the caller).
// False when the list does not fit the launch: more than 2^18 super-tiles (a quad-shape grid of 2^32 workgroups).
bool make_views_frame(int W, int H, uint32_t nviews, int block, FrameDev& F) {
    if (nviews == 0 || !make_frame(W, H, 0, 0, W, H, 0, 1, block, F)) return false;
    const uint64_t view_st = (uint64_t)F.st_x * (uint64_t)F.st_y, nst = view_st * nviews;
    if (nst > (1ull << 18)) return false;
    F.view_st = (uint32_t)view_st;
    F.nst_rank = (uint32_t)nst;
    F.nblocks = ((F.nst_rank + 7u) / 8u) * 8u * (64u / ((uint32_t)block / 64u));
    return true;
}

// Frame gate (FrameDev::gate_*): a pixel rectangle of the W x H frame outside which every primary ray of camera C fails
// the mesh root gate, walk_begin's `starts_in_box(o, lo, hi) || ray_box(lo, hi, o, d, t, tb)` in its float arithmetic.  All in float64:
//   * the box is widened plane by plane by 2^-20 |plane - o|: the gate's six quotients fl(fl(plane - o) / d) are each within 2^-23 of
//     the exact quotient, so the float verdict "enters" implies that the ray (o, d) of the float direction d meets the widened box;
//   * the eight corners of the widened box are taken through the inverse of primary_ray -- M^-1 (corner - o), M the matrix of
//     quat_rotate for the float quaternion as it is (not assumed unit) -- and divided by their depth: the box being convex and
//     wholly in front of the camera plane, a ray that meets it passes the image plane inside the hull of the eight projections, hence
//     inside their bounding rectangle (pixel x samples the plane at ndc fl(x / W) * 2 - 1: no half-pixel offset);
//   * the rectangle is widened by one whole pixel plus 2^-18 W (1 + hw^2 + hh^2) / hw pixels (H, hh for y): d differs from the exact
//     direction of the pixel by less than 2^-20 per component (ndc, normalisation and rotation, about twenty roundings of values <= 2),
//     an angle below 2^-19, which moves the point on the image plane by less than 2^-19 (1 + hw^2 + hh^2), i.e. half the second term.
// No rectangle (false) whenever that argument does not apply as it stands:
//   non-finite camera or box values, half extents outside 2^-40 .. 2^40, coordinates outside the fast_boxes envelope (0 or 2^-40 ..
//   2^40 in magnitude, box and origin); the origin inside or on the widened box, or exactly on one of the six box planes (a zero
//   direction component then makes the gate's quotient 0/0 and its ternaries order-sensitive); a corner behind the camera plane or
//   closer to it than 2^-20 of its distance from the origin.
// The caller adds what is not geometry: scenes with spheres (resolve_hit tests them for rays that failed the gate), scenes without a
// tree (root_ref == REF_NONE), the switch.  out = {x0, y0, x1, y1} clipped to the frame; {0, 0, 0, 0}: every pixel misses.
bool frame_gate_rect(const CameraDev& C, const Box6& box, int W, int H, int out[4]) {
    const double hw = C.half_w, hh = C.half_h;
    // (half extents in 2^-40 .. 2^40, like the coordinates: the float normalisation of (-px hw, py hh, 1) then neither overflows nor loses
    // a component, which the direction bound above takes for granted)
    if (!(hw >= 9.094947017729282e-13) || !(hh >= 9.094947017729282e-13) || !(hw <= 1099511627776.0) || !(hh <= 1099511627776.0) || W <= 0 || H <= 0) return false;
    auto in_envelope = [](float v) {
        const float a = std::fabs(v);
        return v == 0.0f || (a >= 9.094947017729282e-13f && a <= 1099511627776.0f);  // (false for NaN and inf)
    };
    double o[3], lo[3], hi[3];
    bool inside = true;
    for (int k = 0; k < 3; k++) {
        if (!in_envelope(C.pos[k]) || !in_envelope(box.lo[k]) || !in_envelope(box.hi[k]) || !(box.lo[k] <= box.hi[k])) return false;
        if (C.pos[k] == box.lo[k] || C.pos[k] == box.hi[k]) return false;
        o[k] = C.pos[k];
        const double r = 9.5367431640625e-07;  // 2^-20
        lo[k] = (double)box.lo[k] - r * std::fabs((double)box.lo[k] - o[k]);
        hi[k] = (double)box.hi[k] + r * std::fabs((double)box.hi[k] - o[k]);
        inside = inside && lo[k] <= o[k] && o[k] <= hi[k];
    }
    if (inside) return false;
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(C.q[k])) return false;
    // quat_rotate(q, v) = v + 2 (w (q x v) + q x (q x v)): its matrix, column by column, and the inverse by cofactors
    const double w = C.q[0], q[3] = {C.q[1], C.q[2], C.q[3]};
    double M[3][3];
    for (int c = 0; c < 3; c++) {
        double v[3] = {0, 0, 0};
        v[c] = 1.0;
        const double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
        const double uuv[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
        for (int r = 0; r < 3; r++) M[r][c] = v[r] + 2.0 * (w * uv[r] + uuv[r]);
    }
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                       M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    if (!(std::fabs(det) > 0.5) || !std::isfinite(det)) return false;  // (1 for a unit quaternion)
    double I[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const int a = (c + 1) % 3, b = (c + 2) % 3, e = (r + 1) % 3, f = (r + 2) % 3;  // cofactor of M[c][r]
            I[r][c] = (M[a][e] * M[b][f] - M[a][f] * M[b][e]) / det;
        }
    double xmin = HUGE_VAL, xmax = -HUGE_VAL, ymin = HUGE_VAL, ymax = -HUGE_VAL;
    for (int corner = 0; corner < 8; corner++) {
        const double p[3] = {((corner & 1) ? hi[0] : lo[0]) - o[0], ((corner & 2) ? hi[1] : lo[1]) - o[1], ((corner & 4) ? hi[2] : lo[2]) - o[2]};
        double v[3];
        for (int r = 0; r < 3; r++) v[r] = I[r][0] * p[0] + I[r][1] * p[1] + I[r][2] * p[2];
        const double dist = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!(v[2] > 9.5367431640625e-07 * dist) || !std::isfinite(dist)) return false;  // at, behind or too close to the camera plane
        // primary_ray: the camera-space direction is (-px * hw, py * hh, 1), px = x / W * 2 - 1
        const double xf = (-(v[0] / v[2]) / hw + 1.0) * 0.5 * (double)W, yf = ((v[1] / v[2]) / hh + 1.0) * 0.5 * (double)H;
        xmin = std::min(xmin, xf), xmax = std::max(xmax, xf);
        ymin = std::min(ymin, yf), ymax = std::max(ymax, yf);
    }
    const double rel = 3.814697265625e-06 * (1.0 + hw * hw + hh * hh);  // 2^-18 (1 + hw^2 + hh^2)
    const double mx = 1.0 + rel * (double)W / hw, my = 1.0 + rel * (double)H / hh;
    if (!std::isfinite(xmin) || !std::isfinite(xmax) || !std::isfinite(ymin) || !std::isfinite(ymax) || !std::isfinite(mx) || !std::isfinite(my)) return false;
    // pixels x with x < xmin - mx or x > xmax + mx are outside: [floor(xmin - mx), floor(xmax + mx) + 1) keeps the rest
    const double x0 = std::floor(xmin - mx), x1 = std::floor(xmax + mx) + 1.0, y0 = std::floor(ymin - my), y1 = std::floor(ymax + my) + 1.0;
    const double cx0 = std::max(x0, 0.0), cx1 = std::min(x1, (double)W), cy0 = std::max(y0, 0.0), cy1 = std::min(y1, (double)H);
    if (cx0 >= cx1 || cy0 >= cy1) {
        out[0] = out[1] = out[2] = out[3] = 0;
        return true;
    }
    out[0] = (int)cx0, out[1] = (int)cy0, out[2] = (int)cx1, out[3] = (int)cy1;
    return true;
}

// pixels of the rectangle that belong to F.rank (its super-tiles, clipped)
unsigned long long owned_pixels(const FrameDev& F) {
    unsigned long long n = 0;
    const uint64_t nst = (uint64_t)F.st_x * (uint64_t)F.st_y;
    for (uint64_t i = (uint64_t)F.rank; i < nst; i += (uint64_t)F.nranks) {
        const int sx = (int)(i % (uint64_t)F.st_x), sy = (int)(i / (uint64_t)F.st_x);
        const int w = std::min(64, (F.x1 - F.x0) - 64 * sx), h = std::min(64, (F.y1 - F.y0) - 64 * sy);
        n += (unsigned long long)w * (unsigned long long)h;
    }
    return n;
}

// Host -> device for the scene's arrays (113 MB for the 800 K-triangle bench scene): through two alternating 8 MB pinned buffers kept
// for the process, the host copying piece k + 1 on a few threads while the DMA engine moves piece k.  Handing the runtime the
// std::vector's pageable memory took 60-90 ms of the 0.41 s a scene took to create (profiles/r3_build_times.txt).
hipError_t staged_h2d(void* dst, const void* src, size_t bytes) {
    const size_t piece_bytes = 8u << 20;
    if (bytes <= (1u << 20)) return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    static std::mutex mu;
    static void* pin[2] = {nullptr, nullptr};
    static hipEvent_t ev[2] = {nullptr, nullptr};
    std::lock_guard<std::mutex> lk(mu);
    hipError_t e = hipSuccess;
    for (int b = 0; b < 2 && e == hipSuccess; b++) {
        if (!pin[b]) e = hipHostMalloc(&pin[b], piece_bytes, hipHostMallocDefault);
        if (e == hipSuccess && !ev[b]) e = hipEventCreateWithFlags(&ev[b], hipEventDisableTiming);
    }
    if (e != hipSuccess) {  // (no pinned memory to be had: the plain copy still works)
        (void)hipGetLastError();
        return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    }
    size_t piece = 0;
    for (size_t off = 0; off < bytes; off += piece_bytes, piece++) {
        const int b = (int)(piece & 1);
        const size_t m = std::min(piece_bytes, bytes - off);
        if (piece >= 2 && (e = hipEventSynchronize(ev[b])) != hipSuccess) return e;
        parallel_copy(pin[b], static_cast<const char*>(src) + off, m);
        if ((e = hipMemcpyAsync(static_cast<char*>(dst) + off, pin[b], m, hipMemcpyHostToDevice, nullptr)) != hipSuccess) return e;
        if ((e = hipEventRecord(ev[b], nullptr)) != hipSuccess) return e;
    }
    return hipStreamSynchronize(nullptr);
}
}  // namespace cgrt
namespace {
template <class T>
int upload(const std::vector<T>& v, void** dptr, uint64_t& total) {
    const size_t bytes = v.size() * sizeof(T);
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 16));
    if (bytes) HIP_TRY(staged_h2d(*dptr, v.data(), bytes));
    total += bytes;
    return CGRT_OK;
}
}  // namespace

extern "C" {

const char* cgrt_last_error(void) { return g_err.c_str(); }
const char* cgrt_version(void) { return "cgrt-mi355x 0.1 (gfx950)"; }

int cgrt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int cgrt_scene_create(const float* pos_nrm, uint32_t nverts, const uint32_t* tri, const uint32_t* tri_mesh, uint32_t ntris,
                      const float* materials, uint32_t nmesh, const float* spheres, uint32_t nspheres, int device, CgrtScene** out) {
    if (!out) return fail(CGRT_E_ARG, "out is NULL");
    *out = nullptr;
    if ((nverts && !pos_nrm) || (ntris && (!tri || !tri_mesh)) || (nmesh && !materials) || (nspheres && !spheres))
        return fail(CGRT_E_ARG, "NULL array with non-zero count");
    if (ntris && (!nverts || !nmesh)) return fail(CGRT_E_ARG, "triangles without vertices or meshes");
    // device == CGRT_DEVICE_NONE builds the tree on the host only (introspection, builder tests);
    // every trace/intersect entry then fails with CGRT_E_NO_DEVICE -- there is no CPU traversal.
    int rc = (device == CGRT_DEVICE_NONE) ? CGRT_OK : select_device(device);
    if (rc) return rc;

    HostScene hs;
    hs.nverts = nverts;
    hs.ntris = ntris;
    hs.nmesh = nmesh;
    hs.nspheres = nspheres;
    try {
        hs.pos_nrm.assign(pos_nrm, pos_nrm + 6 * (size_t)nverts);
        hs.tri.assign(tri, tri + 3 * (size_t)ntris);
        hs.tri_mesh.assign(tri_mesh, tri_mesh + ntris);
        hs.materials.assign(materials, materials + 8 * (size_t)nmesh);
        if (nspheres) hs.spheres.assign(spheres, spheres + 5 * (size_t)nspheres);
        CgrtScene* s = new CgrtScene();
        s->device = device;
        s->ntris = ntris;
        s->nverts = nverts;
        s->tri_index = hs.tri;
        std::string err;
        BuildOptions bo;
        {
            std::lock_guard<std::mutex> lk(g_options_mutex);
            bo = g_build_options;
        }
        if (const char* e = getenv("CGRT_FAST_OPEN")) bo.fast_open = atoi(e);  // experiment knob
        if (!build_reference_bvh(hs, bo, s->bvh, err)) {
            delete s;
            return fail(err.find("deeper") != std::string::npos ? CGRT_E_LIMIT : CGRT_E_ARG, err);
        }
        if (device == CGRT_DEVICE_NONE) {
            *out = s;
            return CGRT_OK;
        }
        uint64_t total = 0;
        {
            static_assert(sizeof(NodePacket) == 64 && sizeof(SubNode) == 64 && sizeof(TriRecord) == 64, "record size");
            const BuiltBvh& B = s->bvh;
            const size_t nrec = B.packets.size() + B.subnodes.size() + B.tris.size();
            hipError_t e = hipMalloc(&s->d_records, nrec ? nrec * 64 : 64);
            char* base = static_cast<char*>(s->d_records);
            if (e == hipSuccess && !B.packets.empty()) e = staged_h2d(base, B.packets.data(), B.packets.size() * 64);
            if (e == hipSuccess && !B.subnodes.empty())
                e = staged_h2d(base + (size_t)B.sub_base * 64, B.subnodes.data(), B.subnodes.size() * 64);
            if (e == hipSuccess && !B.tris.empty())
                e = staged_h2d(base + (size_t)B.tri_base * 64, B.tris.data(), B.tris.size() * 64);
            if (e != hipSuccess) {
                delete s;
                return hip_fail(e, "uploading the record array");
            }
            total += nrec * 64;
        }
        s->nmesh = nmesh;
        if ((rc = upload(hs.materials, &s->d_materials, total))) {
            delete s;
            return rc;
        }
        if ((rc = upload(s->bvh.leaves, &s->d_leaves, total)) || (rc = upload(s->bvh.tri_normals, &s->d_tri_normals, total)) ||
            (rc = upload(s->bvh.spheres, &s->d_spheres, total)) || (rc = upload(s->bvh.tri_leaf, &s->d_tri_leaf, total)) ||
            (rc = upload(s->bvh.paths, &s->d_paths, total))) {
            delete s;
            return rc;
        }
        hipError_t e = hipMalloc((void**)&s->d_queues, 8 * CGRT_QUEUE_BLOCK_WORDS * sizeof(unsigned int));
        if (e == hipSuccess) e = hipMemset(s->d_queues, 0, 8 * CGRT_QUEUE_BLOCK_WORDS * sizeof(unsigned int));
        if (e != hipSuccess) {
            delete s;
            return hip_fail(e, "hipMalloc(queues)");
        }
        {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
                s->persistent_blocks = (unsigned)prop.multiProcessorCount * 4u;
        }
        s->device_bytes = total;
        SceneDev& D = s->dev;
        D.packets = static_cast<const NodePacket*>(s->d_records);
        D.subnodes = static_cast<const SubNode*>(s->d_records);
        D.tris = static_cast<const TriRecord*>(s->d_records);
        D.tri_base = s->bvh.tri_base;
        D.leaves = static_cast<const LeafRec*>(s->d_leaves);
        D.tri_normals = static_cast<const TriNormals*>(s->d_tri_normals);
        D.spheres = static_cast<const SphereRecord*>(s->d_spheres);
        D.tri_leaf = static_cast<const uint32_t*>(s->d_tri_leaf);
        D.paths = static_cast<const float*>(s->d_paths);
        D.scene_eps = s->bvh.scene_absmax * 1.52587890625e-05f;  // 2^-16
        D.fast_boxes = 1;
        for (const TopoNode& n : s->bvh.nodes)
            for (int k = 0; k < 6; k++) {
                const float c = std::fabs(k < 3 ? n.box.lo[k] : n.box.hi[k - 3]);
                if (!(c == 0.0f || (c >= 9.094947017729282e-13f && c <= 1099511627776.0f))) D.fast_boxes = 0;
            }
        // the certificates use the exact fast division, so they need the box envelope too (RayFast::fd is false without it)
        s->fast_root = D.fast_boxes ? s->bvh.fast_root : REF_NONE;
        D.fast_root = s->fast_root;
        D.root_box = s->bvh.root_box;
        D.root_ref = s->bvh.root_ref;
        D.ntris = ntris;
        D.nspheres = nspheres;
        D.npackets = (uint32_t)s->bvh.packets.size();
        D.nleaves = (uint32_t)s->bvh.leaves.size();
        *out = s;
    } catch (const std::bad_alloc&) {
        return fail(CGRT_E_ALLOC, "host allocation failed");
    }
    return CGRT_OK;
}

void cgrt_scene_destroy(CgrtScene* scene) { delete scene; }

int cgrt_set_leaf_accel(int enabled, int sub_leaf_tris) {
    if (sub_leaf_tris < 0 || sub_leaf_tris > 64) return fail(CGRT_E_ARG, "sub_leaf_tris must be in 0..64 (0 = default)");
    std::lock_guard<std::mutex> lk(g_options_mutex);
    g_build_options.leaf_accel = enabled != 0;
    g_build_options.sub_leaf_tris = sub_leaf_tris ? sub_leaf_tris : SUB_LEAF_TRIS;
    return CGRT_OK;
}
int cgrt_set_primary_mode(int mode) {
    if (mode != 0 && mode != 1) return fail(CGRT_E_ARG, "mode must be 0 (wave per tile) or 1 (persistent waves, lane refill)");
    g_primary_mode.store(mode);
    return CGRT_OK;
}
int cgrt_set_kernel_shape(int mode, uint64_t max_rays) {
    if (mode < -1 || mode > 3) return fail(CGRT_E_ARG, "mode must be -1 (by launch size), 0 (lane per ray, 64 per wave), 1 (quad per ray), 2 (lane per ray, 16 per wave) or 3 (4 rays per wave)");
    set_quad_shape(mode, max_rays);
    return CGRT_OK;
}
int cgrt_get_kernel_shape(int* mode, uint64_t* max_rays) {
    int m = 0;
    unsigned long long r = 0;
    get_quad_shape(&m, &r);
    if (mode) *mode = m;
    if (max_rays) *max_rays = r;
    return CGRT_OK;
}
int cgrt_set_fast_tree(int mode) {
    if (mode < -1 || mode > 1) return fail(CGRT_E_ARG, "mode must be -1 (default policy), 0 (never) or 1 (whenever possible)");
    std::lock_guard<std::mutex> lk(g_options_mutex);
    g_build_options.fast_tree = mode;
    return CGRT_OK;
}
int cgrt_scene_set_walk(CgrtScene* s, int certified) {
    if (!s) return fail(CGRT_E_ARG, "scene is NULL");
    if (certified && s->fast_root == REF_NONE) return fail(CGRT_E_ARG, "the scene has no fast tree");
    s->dev.fast_root = certified ? s->fast_root : REF_NONE;
    return CGRT_OK;
}
int cgrt_scene_build_info(const CgrtScene* s, uint32_t* out4) {
    if (!s || !out4) return fail(CGRT_E_ARG, "NULL argument");
    uint32_t wild = 0;
    for (uint8_t w : s->bvh.leaf_wild) wild += w;
    out4[0] = s->bvh.fast_root != REF_NONE ? 1u : 0u;
    out4[1] = wild;
    out4[2] = s->bvh.geometry_finite ? 1u : 0u;
    out4[3] = (uint32_t)s->bvh.leaves.size();
    return CGRT_OK;
}
int cgrt_scene_walk(const CgrtScene* s) { return s ? (s->dev.fast_root != REF_NONE ? 1 : 0) : fail(CGRT_E_ARG, "scene is NULL"); }
int cgrt_num_subnodes(const CgrtScene* s) { return s ? (int)s->bvh.subnodes.size() : fail(CGRT_E_ARG, "scene is NULL"); }

int cgrt_num_levels(const CgrtScene* s) { return s ? s->bvh.levels : fail(CGRT_E_ARG, "scene is NULL"); }
int cgrt_num_nodes(const CgrtScene* s) { return s ? (int)s->bvh.nodes.size() : fail(CGRT_E_ARG, "scene is NULL"); }
double cgrt_build_seconds(const CgrtScene* s) { return s ? s->bvh.build_seconds : 0.0; }
uint64_t cgrt_device_bytes(const CgrtScene* s) { return s ? s->device_bytes : 0; }

int cgrt_get_nodes(const CgrtScene* s, int32_t* meta, float* boxes) {
    if (!s || !meta || !boxes) return fail(CGRT_E_ARG, "NULL argument");
    for (size_t i = 0; i < s->bvh.nodes.size(); i++) {
        const TopoNode& n = s->bvh.nodes[i];
        meta[5 * i] = n.leaf;
        meta[5 * i + 1] = n.level;
        meta[5 * i + 2] = n.child[0];
        meta[5 * i + 3] = n.child[1];
        meta[5 * i + 4] = (int32_t)n.count;
        std::memcpy(boxes + 6 * i, &n.box, 24);
    }
    return CGRT_OK;
}

int64_t cgrt_leaf_prims(const CgrtScene* s, int node, uint32_t* out, uint32_t cap) {
    if (!s || node < 0 || (size_t)node >= s->bvh.nodes.size()) return fail(CGRT_E_ARG, "bad node");
    const TopoNode& n = s->bvh.nodes[node];
    for (uint32_t k = 0; k < n.count && k < cap; k++) out[k] = s->bvh.order[n.first + k];
    return n.count;
}

// Walks the host copy of the device records and checks every reference: child references of the reference tree, leaf
// references in both encodings (REF_LEAF_ACCEL), accelerator child references and runs, alignment of 4-wide nodes, and
// that every triangle is reachable exactly once through the accelerator of its leaf.  0 = consistent.
int cgrt_set_build_threads(int threads) {
    if (threads < 0 || threads > 256) return fail(CGRT_E_ARG, "threads must be in 0..256 (0 = hardware concurrency)");
    std::lock_guard<std::mutex> lk(g_options_mutex);
    g_build_options.threads = threads;
    return CGRT_OK;
}
int cgrt_debug_layout_hash(const CgrtScene* s, uint64_t* out) {
    if (!s || !out) return fail(CGRT_E_ARG, "NULL argument");
    const BuiltBvh& B = s->bvh;
    uint64_t h = 1469598103934665603ull;  // FNV-1a over every array the device reads, in a fixed order
    auto mix = [&](const void* p, size_t n) {
        const unsigned char* q = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; i++) h = (h ^ q[i]) * 1099511628211ull;
        h = (h ^ (uint64_t)n) * 1099511628211ull;
    };
    mix(B.packets.data(), B.packets.size() * sizeof(NodePacket));
    mix(B.subnodes.data(), B.subnodes.size() * sizeof(SubNode));
    mix(B.tris.data(), B.tris.size() * sizeof(TriRecord));
    mix(B.leaves.data(), B.leaves.size() * sizeof(LeafRec));
    mix(B.tri_normals.data(), B.tri_normals.size() * sizeof(TriNormals));
    mix(B.paths.data(), B.paths.size() * sizeof(float));
    mix(B.tri_leaf.data(), B.tri_leaf.size() * sizeof(uint32_t));
    mix(&B.fast_root, sizeof(B.fast_root));
    mix(&B.root_ref, sizeof(B.root_ref));
    *out = h;
    return CGRT_OK;
}
void cgrt_debug_node_pack(const float* boxes, const uint32_t* refs, uint32_t leaf_index, uint32_t* words) {
    SubNode node[2] = {};
    for (int c = 0; c < SUB_WIDTH; c++) {
        Box6 b;
        std::memcpy(b.lo, boxes + 6 * c, 12);
        std::memcpy(b.hi, boxes + 6 * c + 3, 12);
        sub_box_store(node, c, b);
        sub_child_ref(node, c) = refs[c];
    }
    sub_leaf_index(node) = leaf_index;
    std::memcpy(words, node, sizeof(node));
}
void cgrt_debug_node_unpack(const uint32_t* words, float* boxes, uint32_t* refs, uint32_t* leaf_index) {
    SubNode node[2];
    std::memcpy(node, words, sizeof(node));
    for (int c = 0; c < SUB_WIDTH; c++) {
        const Box6 b = sub_box_load(node, c);
        std::memcpy(boxes + 6 * c, b.lo, 12);
        std::memcpy(boxes + 6 * c + 3, b.hi, 12);
        refs[c] = sub_child_ref(node, c);
    }
    *leaf_index = sub_leaf_index(node);
}
int cgrt_debug_get_subnodes(const CgrtScene* s, uint32_t* words, uint32_t* sub_base, uint32_t* fast_root, uint32_t* leaf_roots, uint32_t* nleaves) {
    if (!s) return fail(CGRT_E_ARG, "NULL scene");
    const BuiltBvh& B = s->bvh;
    if (words && !B.subnodes.empty()) std::memcpy(words, B.subnodes.data(), B.subnodes.size() * sizeof(SubNode));
    if (sub_base) *sub_base = B.sub_base;
    if (fast_root) *fast_root = B.fast_root;
    if (leaf_roots)
        for (size_t i = 0; i < B.leaves.size(); i++) leaf_roots[i] = B.leaves[i].sub_root;
    if (nleaves) *nleaves = (uint32_t)B.leaves.size();
    return CGRT_OK;
}
int cgrt_debug_check_layout(CgrtScene* s) {
    if (!s) return fail(CGRT_E_ARG, "NULL scene");
    const BuiltBvh& B = s->bvh;
    if (B.packets.empty() && B.leaves.empty()) return CGRT_OK;
    const uint32_t npk = (uint32_t)B.packets.size(), nsub = (uint32_t)B.subnodes.size(), ntri = (uint32_t)B.tris.size();
    const uint32_t nleaf = (uint32_t)B.leaves.size();
    if (B.sub_base != npk || B.tri_base != npk + nsub) return fail(CGRT_E_ARG, "record bases do not match the array sizes");
    std::vector<uint8_t> leaf_seen(nleaf, 0);
    std::vector<uint32_t> tri_seen(ntri, 0);
    auto check_leaf_ref = [&](uint32_t r) -> bool {
        uint32_t li;
        if (r & REF_LEAF_ACCEL) {
            const uint32_t root = r & REF_INDEX26;
            if (root < B.sub_base || root >= B.tri_base || ((root - B.sub_base) & 1u)) return false;
            li = sub_leaf_index(&B.subnodes[root - B.sub_base]);
            if (li >= nleaf || B.leaves[li].sub_root != root) return false;
        } else {
            li = r & ~REF_LEAF;
            if (li >= nleaf) return false;
            if (B.leaves[li].sub_root != REF_NONE) return false;  // an accelerated leaf must be referenced directly
        }
        if (leaf_seen[li]) return false;  // a tree: every leaf has one parent
        leaf_seen[li] = 1;
        return true;
    };
    auto check_topo_ref = [&](uint32_t r) -> bool {
        if (r == REF_NONE) return false;
        return (r & REF_LEAF) ? check_leaf_ref(r) : (r < npk);
    };
    // the transposed node (cgrt_layout.h SubNode): an absent child has an empty box (no ray enters it, whichever plane quarter
    // it reads first), and the last quarter holds the leaf index of an accelerator root and zeros
    auto check_node_quarters = [&](const SubNode* N, uint32_t leaf_index) -> bool {
        for (int c = 0; c < SUB_WIDTH; c++) {
            if (sub_child_ref(N, c) != REF_NONE) continue;
            const Box6 b = sub_box_load(N, c);
            for (int a = 0; a < 3; a++)
                if (!(b.lo[a] > b.hi[a])) return false;
        }
        if (sub_leaf_index(N) != leaf_index) return false;
        for (uint32_t w = SUB_LEAF_WORD + 1; w < 32; w++)
            if (sub_word(N, w) != 0u) return false;
        return true;
    };
    if (!check_topo_ref(B.root_ref)) return fail(CGRT_E_ARG, "bad root reference");
    const uint32_t real_packets = (uint32_t)(B.nodes.size() - nleaf);
    for (uint32_t i = 0; i < real_packets; i++)
        if (!check_topo_ref(B.packets[i].left) || !check_topo_ref(B.packets[i].right)) return fail(CGRT_E_ARG, "bad child reference in a node packet");
    for (uint32_t li = 0; li < nleaf; li++) {
        const LeafRec& L = B.leaves[li];
        if (!leaf_seen[li]) return fail(CGRT_E_ARG, "leaf not referenced by the tree");
        if (L.first < B.tri_base || (uint64_t)L.first + L.count > (uint64_t)B.tri_base + ntri) return fail(CGRT_E_ARG, "leaf record range");
        if (L.sub_root == REF_NONE) {
            for (uint32_t k = 0; k < L.count; k++) tri_seen[L.first - B.tri_base + k]++;
            continue;
        }
        // walk the leaf's accelerator
        std::vector<uint32_t> todo{L.sub_root};
        while (!todo.empty()) {
            const uint32_t r = todo.back();
            todo.pop_back();
            if (r == REF_NONE) continue;
            if (r & REF_LEAF) {
                const uint32_t first = r & REF_INDEX26, cnt = ((r >> 26) & 31u) + 1u;
                if (first < L.first || first + cnt > L.first + L.count) return fail(CGRT_E_ARG, "run outside its leaf");
                for (uint32_t k = 0; k < cnt; k++) tri_seen[first - B.tri_base + k]++;
                continue;
            }
            if (r < B.sub_base || r >= B.tri_base) return fail(CGRT_E_ARG, "accelerator node reference out of range");
            if ((r - B.sub_base) & 1u) return fail(CGRT_E_ARG, "4-wide node not 128-byte aligned");
            const SubNode* N = &B.subnodes[r - B.sub_base];
            if (!check_node_quarters(N, r == L.sub_root ? li : 0u)) return fail(CGRT_E_ARG, "accelerator node: absent child or last quarter malformed");
            for (int c = 0; c < SUB_WIDTH; c++) todo.push_back(sub_child_ref(N, c));
        }
    }
    for (uint32_t t = 0; t < ntri; t++)
        if (tri_seen[t] != 1) return fail(CGRT_E_ARG, "a triangle record is reachable " + std::to_string(tri_seen[t]) + " times");
    if (B.fast_root != REF_NONE) {
        // the fast tree: every reference leaf hangs under it exactly once (as its accelerator root, or as the run of its
        // records), at most TOP_MAX_DEPTH levels deep; paths and tri_leaf describe the reference tree
        if (B.tri_leaf.size() != ntri || B.paths.size() != (size_t)nleaf * PATH_BOXES * 6) return fail(CGRT_E_ARG, "fast tree tables have the wrong size");
        std::vector<uint32_t> seen2(ntri, 0);
        std::vector<std::pair<uint32_t, int>> todo{{B.fast_root, 0}};
        while (!todo.empty()) {
            const uint32_t r = todo.back().first;
            const int depth = todo.back().second;
            todo.pop_back();
            if (r == REF_NONE) continue;
            if (r & REF_LEAF) {
                const uint32_t first = r & REF_INDEX26, cnt = ((r >> 26) & 31u) + 1u;
                if (first < B.tri_base || (uint64_t)first - B.tri_base + cnt > ntri) return fail(CGRT_E_ARG, "fast tree: run out of range");
                for (uint32_t k = 0; k < cnt; k++) seen2[first - B.tri_base + k]++;
                continue;
            }
            if (r < B.sub_base || r >= B.tri_base || ((r - B.sub_base) & 1u)) return fail(CGRT_E_ARG, "fast tree: node reference out of range");
            if (depth >= (int)(FAST_STACK_ENTRIES / (SUB_WIDTH - 1))) return fail(CGRT_E_ARG, "fast tree deeper than its stack allows");
            const SubNode* N = &B.subnodes[r - B.sub_base];
            for (int c = 0; c < SUB_WIDTH; c++) todo.push_back({sub_child_ref(N, c), depth + 1});
        }
        for (uint32_t t = 0; t < ntri; t++)
            if (seen2[t] != 1) return fail(CGRT_E_ARG, "fast tree: a triangle record is reachable " + std::to_string(seen2[t]) + " times");
        for (size_t i = 0; i < B.nodes.size(); i++) {
            if (!B.nodes[i].leaf) continue;
            const uint32_t li = (uint32_t)B.node_to_ref_index[i];
            const LeafRec& L = B.leaves[li];
            const uint32_t plen = L.path_len & 0xffu, need = L.path_len >> 8;
            if ((int)plen != B.nodes[i].level) return fail(CGRT_E_ARG, "path length != leaf level");
            if (plen && std::memcmp(&B.paths[((size_t)li * PATH_BOXES + plen - 1) * 6], &B.nodes[i].box, 24) != 0)
                return fail(CGRT_E_ARG, "a path does not end in its leaf's box");
            if (plen && (!(need & (1u << (plen - 1))) || (need >> plen))) return fail(CGRT_E_ARG, "a certificate must test its leaf's box and nothing beyond the path");
            for (uint32_t k = 0; k + 1 < plen; k++) {  // a box the certificate skips contains the next one
                if (need & (1u << k)) continue;
                const float* a = &B.paths[((size_t)li * PATH_BOXES + k) * 6];
                const float* b = a + 6;
                for (int ax = 0; ax < 3; ax++)
                    if (!(a[ax] <= b[ax] && a[3 + ax] >= b[3 + ax])) return fail(CGRT_E_ARG, "a skipped path box does not contain its successor");
            }
            for (uint32_t k = 0; k < L.count; k++)
                if (B.tri_leaf[L.first - B.tri_base + k] != li) return fail(CGRT_E_ARG, "tri_leaf does not match the leaf table");
        }
    }
    return CGRT_OK;
}

void cgrt_record_sizes(uint32_t* node_bytes, uint32_t* tri_bytes, uint32_t* sub_bytes, uint32_t* hit_bytes) {
    if (node_bytes) *node_bytes = sizeof(NodePacket);
    if (tri_bytes) *tri_bytes = sizeof(TriRecord);
    if (sub_bytes) *sub_bytes = sizeof(SubNode) * 2 - 16;  // bytes read per accelerator node visit: four boxes (96 B) + four references (16 B)
    if (hit_bytes) *hit_bytes = sizeof(CgrtHit);
}

}  // extern "C"
