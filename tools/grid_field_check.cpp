// grid_field_check.cpp -- the host side of cg-raytracer_amd/csrc/grid_field_device.h (include/cgrt.h "Grid fields") as a stand-alone
// program: no GPU, no library, nothing but the header the kernels are compiled from (grid_field_check_common.h holds what the three
// grid checkers share).  Three uses:
//   grid_field_check sample GRID POINTS OUT OUTSIDE FLAGS
//       GRID: 3 u32 {nx, ny, nz}, 3 f32 origin, 3 f32 spacing, then nx ny nz f32 values; POINTS: records of 3 f32; OUTSIDE: the bits of
//       CgrtFieldParams.outside as a decimal u32; FLAGS: 0 or 1 (CGRT_FIELD_CLAMP).  OUT: per point 5 words {value, gradient x y z, inside}
//       as the library stores them -- what tests/test_grid_field_cpu.py compares with the numpy restatement, byte for byte
//   grid_field_check march GRID RAYS OUT ISO RELAX MIN_STEP HIT_EPS MAX_STEPS REFINE FLAGS
//       RAYS: records of 7 f32; the four floats as the decimal u32 of their bits.  OUT: per ray the 8 words of CgrtGridHit, then 3 u64
//       {rays that entered the box, main-loop samples, refinement samples}
//   grid_field_check
//       a self-test over small grids with random, huge, NaN and inf values and points and rays of every kind: no sample reads outside
//       the values, every ray ends within max_steps + refine samples with a known status; meant to be built with
//       -fsanitize=address,undefined
// Build: c++ -std=c++17 -O2 -ffp-contract=off -I cg-raytracer_amd/csrc tools/grid_field_check.cpp -o grid_field_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "grid_field_check_common.h"

using namespace cgrt;

static float from_bits(const char* s) {
    const uint32_t u = (uint32_t)std::strtoul(s, nullptr, 10);
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

static void sample_point(const GridField& G, const float* p, uint32_t outside_bits, bool clamp, uint32_t* out5) {
    float v, g[3];
    const bool in = field_sample<true>(G, p[0], p[1], p[2], clamp, v, g);
    out5[0] = in ? field_bits(v) : outside_bits;
    for (int c = 0; c < 3; c++) out5[1 + c] = in ? field_bits(g[c]) : 0u;
    out5[4] = in ? 1u : 0u;
}

static void march_ray(const GridField& G, const MarchRules& P, const float* ray, uint32_t* out8, uint64_t* work3) {
    MarchResult R;
    uint32_t w[3];
    field_march<true>(G, P, ray, R, w);
    out8[0] = field_bits(R.t), out8[1] = field_bits(R.value), out8[2] = R.steps, out8[3] = R.status;
    for (int c = 0; c < 3; c++) out8[4 + c] = field_bits(R.gradient[c]);
    out8[7] = 0u;
    for (int c = 0; c < 3; c++) work3[c] += w[c];
}

static int self_test() {
    const float inf = INFINITY, nan = NAN;
    const float odd[] = {0.0f, -0.0f, 1.0f, -1.5f, 0.25f, 3.0e38f, -3.0e38f, 1.0e-45f, inf, -inf, nan};
    const uint32_t shapes[4][3] = {{2, 2, 2}, {3, 2, 2}, {17, 9, 5}, {5, 4, 33}};
    int bad = 0;
    size_t samples = 0, rays = 0;
    for (int s = 0; s < 4; s++)
        for (int kind = 0; kind < 3; kind++) {  // smooth, noise, noise with non-finite and huge corners
            Grid g;
            const float origin[3] = {-1.0f, 0.5f, 2.0f}, spacing[3] = {2.0f / (float)(shapes[s][0] - 1), -0.125f, 0.3f};
            set_grid(g, shapes[s], origin, spacing);
            for (size_t i = 0; i < g.values.size(); i++) {
                const float x = (float)(i % shapes[s][0]) * spacing[0] + origin[0];
                g.values[i] = kind == 0 ? x * x - 0.3f : uniform();
                if (kind == 2 && i % 7 == 3) g.values[i] = odd[(i / 7) % 11];
            }
            std::vector<float> pts;
            for (int i = 0; i < 3000; i++)
                for (int c = 0; c < 3; c++) pts.push_back(origin[c] + (uniform() * 0.6f + 0.5f) * g.G.top[c] * spacing[c]);
            for (float x : odd)
                for (float y : odd)
                    for (float z : odd) pts.push_back(x), pts.push_back(y), pts.push_back(z);
            for (size_t i = 0; i < pts.size() / 3; i++)
                for (int clamp = 0; clamp < 2; clamp++) {
                    uint32_t o[5];
                    sample_point(g.G, &pts[3 * i], 0x7fc00123u, clamp != 0, o);
                    samples++;
                    if (o[4] > 1u || (!o[4] && (o[0] != 0x7fc00123u || o[1] || o[2] || o[3]))) bad++;
                    const float* p = &pts[3 * i];
                    if (clamp && !o[4] && p[0] == p[0] && p[1] == p[1] && p[2] == p[2]) bad++;  // only a NaN stays outside
                }
            const MarchRules rules[3] = {{0.1f, 1.0f, 1.0e-3f, 1.0e-4f, 64u, 4u, 0u}, {0.0f, 0.0f, 0.05f, 0.0f, 7u, 32u, 1u},
                                         {-0.2f, 0.5f, 1.0e-4f, 1.0e-3f, 1u, 0u, 0u}};
            for (int i = 0; i < 1500; i++) {
                float ray[7];
                for (int c = 0; c < 3; c++) ray[c] = origin[c] + (uniform() * 1.5f + 0.5f) * g.G.top[c] * spacing[c];
                for (int c = 0; c < 3; c++) ray[3 + c] = uniform() * (i % 5 == 0 ? 0.0f : 2.0f);
                ray[6] = i % 3 ? 3.0e38f : uniform() * 3.0f;
                if (i % 11 == 0) ray[i % 7] = odd[(i / 11) % 11];
                for (const MarchRules& P : rules) {
                    uint32_t o[8];
                    uint64_t w[3] = {0, 0, 0};
                    march_ray(g.G, P, ray, o, w);
                    rays++;
                    if (o[3] > 3u || w[0] > 1u || w[1] > P.max_steps || w[2] > P.refine || o[2] > P.max_steps || o[7]) bad++;
                    if (o[3] == kMarchMiss && (o[0] != 0x7f800000u || o[1] || o[4] || o[5] || o[6])) bad++;
                    if (o[3] == kMarchExhausted && o[2] != P.max_steps) bad++;
                    if (o[3] == kMarchNonfinite && o[1] != kCanonicalNan) bad++;
                    if (!w[0] && (o[3] != kMarchMiss || o[2] || w[1] || w[2])) bad++;
                }
            }
        }
    std::printf("%zu samples, %zu rays, %d failures\n", samples, rays, bad);
    return bad ? 1 : 0;
}

static bool write_out(const char* path, const std::vector<uint32_t>& words, const uint64_t* tail, size_t ntail) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    bool ok = std::fwrite(words.data(), 4, words.size(), f) == words.size();
    if (ntail) ok = ok && std::fwrite(tail, 8, ntail, f) == ntail;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc == 1) return self_test();
    const std::string mode = argv[1];
    Grid g;
    if (mode == "sample" && argc == 7) {
        std::vector<float> pts;
        if (!read_grid(argv[2], g) || !read_floats(argv[3], pts)) return 2;
        const uint32_t outside = (uint32_t)std::strtoul(argv[5], nullptr, 10);
        const bool clamp = std::strtoul(argv[6], nullptr, 10) == kFieldClamp;
        const size_t n = pts.size() / 3;
        std::vector<uint32_t> out(n * 5);
        for (size_t i = 0; i < n; i++) sample_point(g.G, &pts[3 * i], outside, clamp, &out[5 * i]);
        return write_out(argv[4], out, nullptr, 0) ? 0 : 2;
    }
    if (mode == "march" && argc == 12) {
        std::vector<float> rays;
        if (!read_grid(argv[2], g) || !read_floats(argv[3], rays)) return 2;
        const MarchRules P = {from_bits(argv[5]), from_bits(argv[6]), from_bits(argv[7]), from_bits(argv[8]),
                              (uint32_t)std::strtoul(argv[9], nullptr, 10), (uint32_t)std::strtoul(argv[10], nullptr, 10),
                              (uint32_t)std::strtoul(argv[11], nullptr, 10) & kMarchInsideAbove};
        if (P.max_steps < 1u || P.max_steps > 65536u || P.refine > 32u) return 2;
        const size_t n = rays.size() / 7;
        std::vector<uint32_t> out(n * 8);
        uint64_t work[3] = {0, 0, 0};
        for (size_t i = 0; i < n; i++) march_ray(g.G, P, &rays[7 * i], &out[8 * i], work);
        return write_out(argv[4], out, work, 3) ? 0 : 2;
    }
    std::fprintf(stderr, "usage: grid_field_check [sample GRID POINTS OUT OUTSIDE FLAGS | march GRID RAYS OUT ISO RELAX MIN_STEP HIT_EPS MAX_STEPS REFINE FLAGS]\n");
    return 2;
}
