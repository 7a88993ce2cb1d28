// capi.cpp -- implementation of the C-ABI declared in include/cgrt.h.
// Host C++ over the HIP runtime; no torch types, no CPU traversal path: every intersect/trace entry
// launches the gfx950 kernels of trace_kernels.hip and fails loudly when no device is usable.
#include "capi_internal.h"

static_assert(sizeof(CgrtRay) == 28, "CgrtRay must match the reference Ray (ray.h:9-13)");
static_assert(sizeof(CgrtHit) == sizeof(CgrtHitDev), "CgrtHit layout");
static_assert(sizeof(CgrtCounters) == 8 * sizeof(uint64_t), "CgrtCounters is a lane's counter block, word for word (LaneCall::read_counters)");

namespace {

thread_local std::string g_err;
// Process-wide options (cgrt_set_leaf_accel / cgrt_set_fast_tree / cgrt_set_primary_mode).  The build options are copied
// under a mutex when a scene is created; the primary mode is read atomically by every launch.
std::mutex g_options_mutex;
BuildOptions g_build_options;
}  // namespace

namespace cgrt {  // (declared in capi_internal.h, for every translation unit of the C-ABI)
std::atomic<int> g_call_combining{1};  // cgrt_set_call_combining
std::atomic<int> g_render_predict{1};  // cgrt_set_render_prediction
std::atomic<int> g_frame_hints{-1};    // cgrt_set_frame_hints: -1 auto, 0 off, 1 hard tiles first, 2 hard tiles 16 rays per wave
std::atomic<unsigned> g_hint_thr_dense{0}, g_hint_thr_sparse{0};  // cgrt_debug_set_hint_thresholds (0: the defaults)
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
    return true;
}
}  // namespace cgrt

namespace {
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

}  // namespace

namespace cgrt {
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
int cgrt_debug_render_path(const CgrtScene* s) { return s ? s->rpred.last_path : -1; }
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
int cgrt_set_render_prediction(int enabled) {
    g_render_predict.store(enabled ? 1 : 0);
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

// The frame gate of one camera launch (frame_gate_rect): F's rectangle, or none.  What disables it beyond the geometry: the switch, a
// scene with spheres (resolve_hit tests every sphere for a ray that failed the mesh root gate) and a scene without a tree (walk_begin
// returns before the gate).  Nothing else is evaluated for such a ray: finish_ray writes {t as given, no primitive, no material, hit = 0}.
static bool scene_frame_gate(const CgrtScene* s, const CameraDev& C, int W, int H, int out[4]) {
    if (!s->bvh.spheres.empty() || s->bvh.root_ref == REF_NONE) return false;
    return frame_gate_rect(C, s->bvh.root_box, W, H, out);
}
static void apply_frame_gate(const CgrtScene* s, const CameraDev& C, FrameDev& F) {
    int r[4];
    F.gate_x0 = F.gate_y0 = F.gate_x1 = F.gate_y1 = 0;
    if (!g_frame_gate.load() || !scene_frame_gate(s, C, F.W, F.H, r)) return;
    if (r[2] == 0) {  // every pixel misses: a rectangle no pixel is inside of (gate_x1 != 0: the gate is on)
        F.gate_x0 = F.gate_y0 = F.gate_x1 = F.gate_y1 = 0x7fffffff;
        return;
    }
    F.gate_x0 = r[0], F.gate_y0 = r[1], F.gate_x1 = r[2], F.gate_y1 = r[3];
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
static int views_extent_args(uint32_t nviews, int W, int H) {
    if ((unsigned long long)nviews * (unsigned long long)W * (unsigned long long)H > 0x7fffffffull)
        return fail(CGRT_E_ARG, "batch too large: nviews*W*H exceeds 0x7fffffff");
    FrameDev F;
    if (!make_views_frame(W, H, nviews, 64, F)) return fail(CGRT_E_ARG, "batch too large: more than 2^18 64x64 super-tiles over all views");
    return CGRT_OK;
}
// A batch of ray cameras (include/cgrt.h CgrtRayCamera), checked where the Trackball entries check `cams`: every field finite, a direction
// that is not identically zero, offsets that keep x + x_off and y + y_off exactly convertible to f32.
static int raycams_check(const CgrtRayCamera* cams, uint32_t nviews, int W, int H) {
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
// The plan of a checked CgrtLightSets (light_sets_args): distinct slots in order of first appearance, set after set.
static void plan_light_sets(const CgrtLightSets& L, LightSetSrc& P) {
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
// cgrt_shade_rays' rules for the spherical lights, which every frame entry shares; NULL = no spherical lights
extern "C++" int cgrt::soft_rules(const CgrtSoftShadows* soft) {
    if (soft && soft->nspherical &&
        (!soft->spherical || !soft->unit_vectors || soft->nunits == 0 || soft->samples == 0 || soft->samples > (1u << 24)))
        return fail(CGRT_E_ARG, "soft shadows need lights, a unit-vector table and 1..2^24 samples");
    return CGRT_OK;
}

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
static int render_impl(CgrtScene* s, const FrameRequest& R) {
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

// a request with where its driver reports: a blocking frame's stats, an enqueued frame's ticket
static int render_frame(CgrtScene* s, FrameRequest R, CgrtRenderStats* stats) {
    R.stats = stats;
    return render_impl(s, R);
}
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
static int aa_args(const CgrtCamera* cam, const void* out, int W, int H, const float* lights, uint32_t nlights, const CgrtSoftShadows* soft,
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
static int export_args(const void* out, int W, int H, int format, uint64_t row_bytes, uint64_t* pitch, uint64_t* extent) {
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

// ---- enqueued frames (include/cgrt.h cgrt_enqueue_*) ----
// The frame of render_impl's exact path, issued without a host round trip: every list is sized for the worst case (as render_impl
// sizes the workspace anyway), all max_level levels are issued, and every launch after the primary kernel is a capped, count-driven grid
// (GRID_STRIDED) that reads its list's length on the device.  A single camera's level 0 is spawned by the primary kernel
// itself (the predicted frame's fused spawn); views and ray lists run their own primary kernels and a count-driven spawn.  The whole
// frame, export included, is on the caller's stream, behind the scene's previous frames (enq_done, export_done), and nothing is waited
// for on the host unless the workspace grows or every ticket slot is in flight.  Same kernels' expressions on the same entries, each
// scattered back by its pixel: the bytes are the blocking entry's.  The caller has checked the arguments (the blocking entries' checks).
static int enqueue_impl(CgrtScene* s, const FrameRequest& R) {
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

static int enqueue_frame(CgrtScene* s, FrameRequest R, uint64_t* ticket) {
    R.ticket = ticket;
    return enqueue_impl(s, R);
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
