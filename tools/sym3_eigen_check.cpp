// sym3_eigen_check.cpp -- the host side of cg-raytracer_amd/csrc/sym3_eigen.h (include/cgrt.h "Point-set frames", steps 4 to 7) as a
// stand-alone program: no GPU, no library, nothing but the header.  Two uses:
//   sym3_eigen_check IN OUT     IN: records of 10 f32 {xx, xy, xz, yy, yz, zz, oriented (0 or 1), ox, oy, oz}; OUT: per record 13 f32
//                               {lambda0..2, normal, tangent_u, tangent_v, sweeps} with every NaN canonical -- what
//                               tests/test_point_frames_cpu.py compares with the numpy restatement, bit for bit
//   sym3_eigen_check            a self-test over a few thousand matrices (random, diagonal, rank-deficient, zero, huge, NaN and inf ones):
//                               the loop ends within 8 sweeps, finite input of moderate size gives unit vectors; meant to be built with
//                               -fsanitize=address,undefined
// Build: c++ -std=c++17 -O2 -ffp-contract=off -I cg-raytracer_amd/csrc tools/sym3_eigen_check.cpp -o sym3_eigen_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sym3_eigen.h"

using namespace cgrt;

static void solve(const float* in, float* out) {
    const Sym3 S = {in[0], in[1], in[2], in[3], in[4], in[5]};
    Sym3Frame F;
    const int sweeps = sym3_eigen(S, F);
    sym3_signs(F, in[6] != 0.0f, in[7], in[8], in[9]);
    for (int i = 0; i < 3; i++) {
        out[i] = sym3_canonical(F.lambda[i]);
        out[3 + i] = sym3_canonical(F.n[i]);
        out[6 + i] = sym3_canonical(F.u[i]);
        out[9 + i] = sym3_canonical(F.v[i]);
    }
    out[12] = (float)sweeps;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static float uniform() {  // [-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((double)(rng_state >> 11) / 4503599627370496.0 - 1.0);
}

static int self_test() {
    const float inf = INFINITY, nan = NAN;
    std::vector<float> in;
    auto add = [&](float xx, float xy, float xz, float yy, float yz, float zz, float on, float ox, float oy, float oz) {
        const float r[10] = {xx, xy, xz, yy, yz, zz, on, ox, oy, oz};
        in.insert(in.end(), r, r + 10);
    };
    for (int i = 0; i < 4000; i++) {  // covariances of 1 .. 9 random points, at scales 2^-40 .. 2^40
        const int k = 1 + i % 9;
        const float scale = std::ldexp(1.0f, (i % 5 - 2) * 20);
        float p[9][3], c[3] = {0, 0, 0}, a[6] = {0, 0, 0, 0, 0, 0};
        for (int j = 0; j < k; j++)
            for (int x = 0; x < 3; x++) p[j][x] = uniform() * scale, c[x] += p[j][x] / (float)k;
        for (int j = 0; j < k; j++) {
            const float e[3] = {p[j][0] - c[0], p[j][1] - c[1], (i % 7 == 0 ? 0.0f : p[j][2] - c[2])};
            a[0] += e[0] * e[0], a[1] += e[0] * e[1], a[2] += e[0] * e[2], a[3] += e[1] * e[1], a[4] += e[1] * e[2], a[5] += e[2] * e[2];
        }
        add(a[0] / k, a[1] / k, a[2] / k, a[3] / k, a[4] / k, a[5] / k, (float)(i & 1), uniform(), uniform(), uniform());
    }
    const size_t moderate = in.size() / 10;
    const float odd[] = {0.0f, -0.0f, 1.0f, -1.0f, 3.0e38f, -3.0e38f, 1.0e-45f, inf, -inf, nan};
    for (float x : odd)
        for (float y : odd)
            for (float z : odd) {
                add(x, y, z, y, z, x, 1.0f, z, nan, x);
                add(x, 0.0f, 0.0f, y, 0.0f, z, 0.0f, 0.0f, 0.0f, 0.0f);
                add(1.0f, x, y, 1.0f, z, 1.0f, 1.0f, inf, 0.0f, 0.0f);
            }
    const size_t n = in.size() / 10;
    std::vector<float> out(n * 13);
    int bad = 0, most = 0;
    for (size_t i = 0; i < n; i++) {
        solve(&in[i * 10], &out[i * 13]);
        const float* o = &out[i * 13];
        if (!(o[12] >= 1.0f && o[12] <= (float)kSym3Sweeps)) bad++;
        if (i < moderate) {
            most = o[12] > (float)most ? (int)o[12] : most;
            for (int v = 0; v < 3; v++) {
                const float l2 = o[3 + 3 * v] * o[3 + 3 * v] + o[4 + 3 * v] * o[4 + 3 * v] + o[5 + 3 * v] * o[5 + 3 * v];
                if (!(std::fabs(l2 - 1.0f) < 1.0e-5f)) bad++;
            }
            if (!(o[0] <= o[1] && o[1] <= o[2])) bad++;
        }
    }
    std::printf("%zu matrices (%zu of moderate size, at most %d sweeps), %d failures\n", n, moderate, most, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return self_test();
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> in;
    float rec[10];
    while (std::fread(rec, sizeof(float), 10, f) == 10) in.insert(in.end(), rec, rec + 10);
    std::fclose(f);
    const size_t n = in.size() / 10;
    std::vector<float> out(n * 13);
    for (size_t i = 0; i < n; i++) solve(&in[i * 10], &out[i * 13]);
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
