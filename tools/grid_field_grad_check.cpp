// grid_field_grad_check.cpp -- the host side of the sampler's adjoint (include/cgrt.h "Grid fields, the adjoint of the sampler";
// field_grad_item and field_corners of cg-raytracer_amd/csrc/grid_field_device.h) as a stand-alone program: no GPU, no library, nothing
// but the header the kernel is compiled from (grid_field_check_common.h holds what the three grid checkers share).  Two uses:
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

#include "grid_field_check_common.h"

using namespace cgrt;

// Point i of the call Q: its non-zero contributions are added to `into`.  Returns the number of additions, or -1 if an element index
// left the grid.
static int add_point(const FieldGradCall& Q, uint32_t i, std::vector<float>& into, float (*seen)[8] = nullptr) {
    uint64_t at[8];
    float c[8];
    int count, added = 0;
    if (!grad_point(Q, i, into.size(), at, c, count)) return -1;
    if (seen && count) std::memcpy(*seen, c, sizeof c);
    for (int k = 0; k < count; k++)
        if (c[k] != 0.0f) into[at[k]] += c[k], added++;
    return added;
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
                    const int a = add_point(grad_call(g, p, 1, combo & 1 ? &gv : nullptr, combo & 2 ? gg : nullptr, clamp != 0), 0, g.values, &c1);
                    points++;
                    if (a < 0 || a > 8 || (!in && a != 0)) bad++;
                    if (a > 0) adds += (size_t)a;
                    if (clamp && !in && p[0] == p[0] && p[1] == p[1] && p[2] == p[2]) bad++;  // only a NaN stays outside
                    if (in && i >= first_grid_point && i < first_odd && combo == 1 && field_finite(gv) && a != (gv != 0.0f ? 1 : 0))
                        bad++;  // (an infinite gv times a zero weight is a NaN, which is added)
                    if (!in || i >= first_odd || i % 13 == 5 || i % 17 == 3) continue;  // ordinary points and grads: inside the envelope
                    gv *= 4.0f, gg[0] *= 4.0f, gg[1] *= 4.0f, gg[2] *= 4.0f;
                    std::vector<float> scratch(g.values.size(), 0.0f);
                    if (add_point(grad_call(g, p, 1, combo & 1 ? &gv : nullptr, combo & 2 ? gg : nullptr, clamp != 0), 0, scratch, &c4) < 0) bad++;
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
        const FieldGradCall Q = grad_call(g, pts.data(), n, has_gv ? gv.data() : nullptr, has_gg ? gg.data() : nullptr, clamp);
        for (size_t i = 0; i < n; i++)
            if (add_point(Q, (uint32_t)i, g.values) < 0) return 3;
        return write_floats(argv[6], g.values) ? 0 : 2;
    }
    std::fprintf(stderr, "usage: grid_field_grad_check [--self-test | adjoint GRID POINTS GRAD_VALUE GRAD_GRADIENT OUT FLAGS]\n");
    return 2;
}
