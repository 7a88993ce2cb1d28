// grid_field_grad_check.cpp -- the host side of the sampler's adjoint (include/cgrt.h "Grid fields, the adjoint of the sampler";
// field_cell and field_adjoint of cg-raytracer_amd/csrc/grid_field_device.h) as a stand-alone program: no GPU, no library, nothing but
// the header the kernel is compiled from.  Two uses:
//   grid_field_grad_check adjoint GRID POINTS GRAD_VALUE GRAD_GRADIENT OUT FLAGS
//       GRID: 3 u32 {nx, ny, nz}, 3 f32 origin, 3 f32 spacing, then nx ny nz f32 -- the PREVIOUS content of grad_values; POINTS: records
//       of 3 f32; GRAD_VALUE: n f32, GRAD_GRADIENT: records of 3 f32, either may be "-" (not given), not both; FLAGS: 0 or 1
//       (CGRT_FIELD_CLAMP).  OUT: nx ny nz f32, the previous content with every non-zero contribution added one by one in f32, points in
//       order, corners in the order x + 2 y + 4 z -- what tests/test_grid_field_grad_cpu.py compares with the numpy restatement's
//       sequential sum, byte for byte
//   grid_field_grad_check --self-test
//       small grids, points and grads of every kind (grid points, faces, outside, huge, NaN, inf): every element index lies inside the
//       grid, an outside point adds nothing, a point on a grid point with grad_value alone adds to one element, scaling the grads by 4
//       scales every contribution by 4; meant to be built with -fsanitize=address,undefined
// Build: c++ -std=c++17 -O2 -ffp-contract=off -I cg-raytracer_amd/csrc tools/grid_field_grad_check.cpp -o grid_field_grad_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "grid_field_device.h"

using namespace cgrt;

struct Grid {
    GridField G;
    std::vector<float> values;
};

static void set_grid(Grid& g, const uint32_t dims[3], const float origin[3], const float spacing[3]) {
    for (int c = 0; c < 3; c++) g.G.origin[c] = origin[c], g.G.spacing[c] = spacing[c], g.G.top[c] = (float)(dims[c] - 1u);
    g.G.nx = dims[0], g.G.ny = dims[1], g.G.nz = dims[2];
    g.values.assign((size_t)dims[0] * dims[1] * dims[2], 0.0f);
    g.G.values = g.values.data();
}

static bool read_grid(const char* path, Grid& g) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint32_t dims[3];
    float os[6];
    bool ok = std::fread(dims, 4, 3, f) == 3 && std::fread(os, 4, 6, f) == 6;
    for (int c = 0; ok && c < 3; c++) ok = dims[c] >= 2 && dims[c] <= (1u << 24) && os[3 + c] != 0.0f;
    ok = ok && (uint64_t)dims[0] * dims[1] * dims[2] <= 0x7fffffffull;
    if (ok) {
        set_grid(g, dims, os, os + 3);
        ok = std::fread(g.values.data(), 4, g.values.size(), f) == g.values.size();
    }
    std::fclose(f);
    return ok;
}

static bool read_floats(const char* path, std::vector<float>& out) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    float rec[256];
    size_t got;
    while ((got = std::fread(rec, 4, 256, f)) > 0) out.insert(out.end(), rec, rec + got);
    std::fclose(f);
    return true;
}

// One point: its non-zero contributions are added to `into` (the grid's element count is checked, not trusted).  Returns the number of
// additions, or -1 if an element index left the grid.
static int add_point(const GridField& G, std::vector<float>& into, const float* p, const float* gv, const float* gg, bool clamp,
                     float (*seen)[8] = nullptr) {
    int ic[3];
    float f[3];
    if (!field_cell(G, p[0], p[1], p[2], clamp, ic, f)) return 0;
    const float none[3] = {0.0f, 0.0f, 0.0f};
    const float g3[3] = {gg ? gg[0] : 0.0f, gg ? gg[1] : 0.0f, gg ? gg[2] : 0.0f};
    float c[8];
    field_adjoint(G.spacing, f, gv != nullptr, gv ? *gv : 0.0f, gg != nullptr, gg ? g3 : none, c);
    if (seen) std::memcpy(*seen, c, sizeof c);
    for (int a = 0; a < 3; a++)
        if (ic[a] < 0 || (uint32_t)ic[a] + 1u >= (a == 0 ? G.nx : a == 1 ? G.ny : G.nz)) return -1;
    const uint64_t base = ((uint64_t)ic[2] * G.ny + (uint64_t)ic[1]) * G.nx + (uint64_t)ic[0];
    int added = 0;
    for (int k = 0; k < 8; k++) {
        const uint64_t at = base + (uint64_t)(k & 1) + (uint64_t)((k >> 1) & 1) * G.nx + (uint64_t)(k >> 2) * G.nx * G.ny;
        if (at >= into.size()) return -1;
        if (c[k] != 0.0f) into[at] += c[k], added++;
    }
    return added;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static float uniform() {  // [-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((double)(rng_state >> 11) / 4503599627370496.0 - 1.0);
}

static int self_test() {
    const float inf = INFINITY, nan = NAN;
    const float odd[] = {0.0f, -0.0f, 1.0f, -1.5f, 0.25f, 3.0e38f, -3.0e38f, 1.0e-45f, inf, -inf, nan};
    const uint32_t shapes[4][3] = {{2, 2, 2}, {3, 2, 2}, {17, 9, 5}, {5, 4, 33}};
    int bad = 0;
    size_t points = 0, adds = 0;
    for (int s = 0; s < 4; s++) {
        Grid g;
        const float origin[3] = {-1.0f, 0.5f, 2.0f}, spacing[3] = {2.0f / (float)(shapes[s][0] - 1), -0.125f, 0.5f};
        set_grid(g, shapes[s], origin, spacing);
        std::vector<float> pts;
        for (int i = 0; i < 3000; i++)
            for (int c = 0; c < 3; c++) pts.push_back(origin[c] + (uniform() * 0.6f + 0.5f) * g.G.top[c] * spacing[c]);
        for (uint32_t z = 0; z < shapes[s][2]; z++)  // the grid points of one row and one column
            for (uint32_t x = 0; x < shapes[s][0]; x++)
                pts.push_back(origin[0] + (float)x * spacing[0]), pts.push_back(origin[1]), pts.push_back(origin[2] + (float)z * spacing[2]);
        const size_t first_grid_point = 3000, first_odd = pts.size() / 3;
        for (float x : odd)
            for (float y : odd)
                for (float z : odd) pts.push_back(x), pts.push_back(y), pts.push_back(z);
        for (size_t i = 0; i < pts.size() / 3; i++)
            for (int clamp = 0; clamp < 2; clamp++)
                for (int combo = 1; combo < 4; combo++) {
                    const float* p = &pts[3 * i];
                    float gv = i % 13 == 5 ? odd[(i / 13) % 11] : uniform() * 8.0f;
                    float gg[3] = {uniform(), i % 17 == 3 ? odd[(i / 17) % 11] : uniform(), uniform()};
                    float c1[8], c4[8];
                    int ic[3];
                    float f[3];
                    const bool in = field_cell(g.G, p[0], p[1], p[2], clamp != 0, ic, f);
                    const int a = add_point(g.G, g.values, p, combo & 1 ? &gv : nullptr, combo & 2 ? gg : nullptr, clamp != 0, &c1);
                    points++;
                    if (a < 0 || a > 8 || (!in && a != 0)) bad++;
                    if (a > 0) adds += (size_t)a;
                    if (clamp && !in && p[0] == p[0] && p[1] == p[1] && p[2] == p[2]) bad++;  // only a NaN stays outside
                    if (in && i >= first_grid_point && i < first_odd && combo == 1 && field_finite(gv) && a != (gv != 0.0f ? 1 : 0))
                        bad++;  // (an infinite gv times a zero weight is a NaN, which is added)
                    if (!in || i >= first_odd || i % 13 == 5 || i % 17 == 3) continue;  // ordinary points and grads: inside the envelope
                    gv *= 4.0f, gg[0] *= 4.0f, gg[1] *= 4.0f, gg[2] *= 4.0f;
                    std::vector<float> scratch(g.values.size(), 0.0f);
                    if (add_point(g.G, scratch, p, combo & 1 ? &gv : nullptr, combo & 2 ? gg : nullptr, clamp != 0, &c4) < 0) bad++;
                    for (int k = 0; k < 8; k++) {
                        const float want = 4.0f * c1[k];
                        const bool normal = std::fabs(c1[k]) > 1.0e-30f && std::fabs(c1[k]) < 1.0e30f;  // (well inside the envelope)
                        if (normal && std::memcmp(&want, &c4[k], 4) != 0) bad++;
                    }
                }
    }
    std::printf("%zu points, %zu additions, %d failures\n", points, adds, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "--self-test") return self_test();
    if (argc == 8 && std::string(argv[1]) == "adjoint") {
        Grid g;
        std::vector<float> pts, gv, gg;
        const bool has_gv = std::string(argv[4]) != "-", has_gg = std::string(argv[5]) != "-";
        if (!has_gv && !has_gg) return 2;
        if (!read_grid(argv[2], g) || !read_floats(argv[3], pts) || pts.size() % 3) return 2;
        const size_t n = pts.size() / 3;
        if (has_gv && (!read_floats(argv[4], gv) || gv.size() != n)) return 2;
        if (has_gg && (!read_floats(argv[5], gg) || gg.size() != 3 * n)) return 2;
        const bool clamp = std::strtoul(argv[7], nullptr, 10) == kFieldClamp;
        for (size_t i = 0; i < n; i++)
            if (add_point(g.G, g.values, &pts[3 * i], has_gv ? &gv[i] : nullptr, has_gg ? &gg[3 * i] : nullptr, clamp) < 0) return 3;
        std::FILE* f = std::fopen(argv[6], "wb");
        if (!f) return 2;
        const bool ok = std::fwrite(g.values.data(), 4, g.values.size(), f) == g.values.size();
        return std::fclose(f) == 0 && ok ? 0 : 2;
    }
    std::fprintf(stderr, "usage: grid_field_grad_check [--self-test | adjoint GRID POINTS GRAD_VALUE GRAD_GRADIENT OUT FLAGS]\n");
    return 2;
}
