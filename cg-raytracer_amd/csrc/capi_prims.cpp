// capi_prims.cpp -- the element-wise primitives of include/cgrt.h (one test per element, no scene) and two stand-alone debug entries.
#include "capi_internal.h"

namespace {
// One array of an element-wise call: a device buffer of `bytes` (none when 0: the launch gets a null pointer), filled from `in`
// before the launch and copied to `out` after it, each where given.
struct PrimArray {
    const void* in;
    void* out;
    size_t bytes;
};
// select the device; n == 0 is done; else allocate, upload, launch(buffers), wait, download -- in the arrays' order
template <size_t N, class Launch>
int prim_call(int device, uint64_t n, const PrimArray (&a)[N], Launch launch) {
    const int rc = select_device(device);
    if (rc) return rc;
    if (n == 0) return CGRT_OK;
    DevBuf d[N];
    for (size_t i = 0; i < N; i++)
        if (a[i].bytes) HIP_TRY(d[i].alloc(a[i].bytes));
    for (size_t i = 0; i < N; i++)
        if (a[i].bytes && a[i].in) HIP_TRY(hipMemcpy(d[i].p, a[i].in, a[i].bytes, hipMemcpyHostToDevice));
    HIP_TRY(launch(d));
    HIP_TRY(hipDeviceSynchronize());
    for (size_t i = 0; i < N; i++)
        if (a[i].bytes && a[i].out) HIP_TRY(hipMemcpy(a[i].out, d[i].p, a[i].bytes, hipMemcpyDeviceToHost));
    return CGRT_OK;
}
}  // namespace

extern "C" {

int cgrt_ray_triangle_batch(int device, const float* tri, const CgrtRay* rays, uint64_t n, float* t_out, uint8_t* hit, float* normals) {
    if (n && (!tri || !rays || !t_out || !hit)) return fail(CGRT_E_ARG, "NULL argument");
    const PrimArray a[] = {{tri, nullptr, n * 72}, {rays, nullptr, n * 28}, {nullptr, t_out, n * 4}, {nullptr, hit, n}, {normals, normals, normals ? n * 12 : 0}};
    return prim_call(device, n, a, [&](const DevBuf* d) {
        return launch_ray_triangle(d[0].as<float>(), d[1].as<float>(), n, d[2].as<float>(), d[3].as<uint8_t>(), d[4].as<float>(), nullptr);
    });
}

int cgrt_ray_plane_batch(int device, const float* plane, const CgrtRay* rays, uint64_t n, float* t_out, uint8_t* hit) {
    if (n && (!plane || !rays || !t_out || !hit)) return fail(CGRT_E_ARG, "NULL argument");
    const PrimArray a[] = {{plane, nullptr, n * 16}, {rays, nullptr, n * 28}, {nullptr, t_out, n * 4}, {nullptr, hit, n}};
    return prim_call(device, n, a, [&](const DevBuf* d) {
        return launch_ray_plane(d[0].as<float>(), d[1].as<float>(), n, d[2].as<float>(), d[3].as<uint8_t>(), nullptr);
    });
}

int cgrt_ray_box_batch(int device, const float* box, const CgrtRay* rays, uint64_t n, float* t_out, uint8_t* hit, uint8_t* inside) {
    if (n && (!box || !rays || !t_out || !hit)) return fail(CGRT_E_ARG, "NULL argument");
    const PrimArray a[] = {{box, nullptr, n * 24}, {rays, nullptr, n * 28}, {nullptr, t_out, n * 4}, {nullptr, hit, n}, {nullptr, inside, n}};
    return prim_call(device, n, a, [&](const DevBuf* d) {
        return launch_ray_box(d[0].as<float>(), d[1].as<float>(), n, d[2].as<float>(), d[3].as<uint8_t>(), d[4].as<uint8_t>(), nullptr);
    });
}

int cgrt_ray_sphere_batch(int device, const float* sphere, const CgrtRay* rays, uint64_t n, float* t_out, uint8_t* hit, float* normals) {
    if (n && (!sphere || !rays || !t_out || !hit)) return fail(CGRT_E_ARG, "NULL argument");
    const PrimArray a[] = {{sphere, nullptr, n * 16}, {rays, nullptr, n * 28}, {nullptr, t_out, n * 4}, {nullptr, hit, n}, {normals, normals, normals ? n * 12 : 0}};
    return prim_call(device, n, a, [&](const DevBuf* d) {
        return launch_ray_sphere(d[0].as<float>(), d[1].as<float>(), n, d[2].as<float>(), d[3].as<uint8_t>(), d[4].as<float>(), nullptr);
    });
}

int cgrt_triangle_plane_batch(int device, const float* tri, uint64_t n, float* plane) {
    if (n && (!tri || !plane)) return fail(CGRT_E_ARG, "NULL argument");
    const PrimArray a[] = {{tri, nullptr, n * 36}, {nullptr, plane, n * 16}};
    return prim_call(device, n, a, [&](const DevBuf* d) { return launch_triangle_plane(d[0].as<float>(), n, d[1].as<float>(), nullptr); });
}

int cgrt_point_in_triangle_batch(int device, const float* in, uint64_t n, uint8_t* out) {
    if (n && (!in || !out)) return fail(CGRT_E_ARG, "NULL argument");
    const PrimArray a[] = {{in, nullptr, n * 60}, {nullptr, out, n}};
    return prim_call(device, n, a, [&](const DevBuf* d) { return launch_point_in_triangle(d[0].as<float>(), n, d[1].as<uint8_t>(), nullptr); });
}

int cgrt_debug_gather_calibration(int device, uint64_t nrecords, int repeats) {
    // nrecords x 64 B of zeros, each record read exactly once per launch in a scattered order (see k_gather_calib)
    int rc = select_device(device);
    if (rc) return rc;
    if (nrecords < 1024 || repeats < 1) return fail(CGRT_E_ARG, "nrecords >= 1024, repeats >= 1");
    DevBuf table, sink;
    HIP_TRY(table.alloc((size_t)nrecords * 64));
    HIP_TRY(sink.alloc(16));
    HIP_TRY(hipMemset(table.p, 0, (size_t)nrecords * 64));
    unsigned long long mult = 2654435761ull;
    auto gcd = [](unsigned long long a, unsigned long long b) {
        while (b) {
            const unsigned long long t = a % b;
            a = b;
            b = t;
        }
        return a;
    };
    while (gcd(mult, nrecords) != 1) mult += 2;
    for (int r = 0; r < repeats; r++) HIP_TRY(launch_gather_calib(table.p, nrecords, mult, 12345ull + 7919ull * r, sink.as<float>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    return CGRT_OK;
}

int cgrt_debug_fastdiv_check(int device, const float* a, const float* d, uint64_t n, uint64_t* mismatches, float* first_bad) {
    if (n && (!a || !d || !mismatches || !first_bad)) return fail(CGRT_E_ARG, "NULL argument");
    int rc = select_device(device);
    if (rc) return rc;
    if (n == 0) return CGRT_OK;
    DevBuf da, dd, dm, db;
    HIP_TRY(da.alloc(n * 4));
    HIP_TRY(dd.alloc(n * 4));
    HIP_TRY(dm.alloc(8));
    HIP_TRY(db.alloc(16));
    HIP_TRY(hipMemcpy(da.p, a, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dd.p, d, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dm.p, 0, 8));
    HIP_TRY(hipMemset(db.p, 0, 16));
    HIP_TRY(launch_fastdiv_check(da.as<float>(), dd.as<float>(), n, dm.as<unsigned long long>(), db.as<float>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(mismatches, dm.p, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(first_bad, db.p, 16, hipMemcpyDeviceToHost));
    return CGRT_OK;
}

}  // extern "C"
