// grid_field_check_common.h -- what the three stand-alone grid-field checkers (grid_field_check.cpp, grid_field_grad_check.cpp,
// grid_field_grad_repro_check.cpp) share: the grid with its storage, the GRID file and flat f32 files, and the self-tests' generator.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "grid_field_device.h"

struct Grid {
    cgrt::GridField G;
    std::vector<float> values;
};

// a grid of zeros
static inline void set_grid(Grid& g, const uint32_t dims[3], const float origin[3], const float spacing[3]) {
    for (int c = 0; c < 3; c++) g.G.origin[c] = origin[c], g.G.spacing[c] = spacing[c], g.G.top[c] = (float)(dims[c] - 1u);
    g.G.nx = dims[0], g.G.ny = dims[1], g.G.nz = dims[2];
    g.values.assign((size_t)dims[0] * dims[1] * dims[2], 0.0f);
    g.G.values = g.values.data();
}

// GRID: 3 u32 {nx, ny, nz}, 3 f32 origin, 3 f32 spacing, then nx ny nz f32
static inline bool read_grid(const char* path, Grid& g) {
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

// every whole f32 of the file; the caller divides by its record width (a trailing part of a record is not a record)
static inline bool read_floats(const char* path, std::vector<float>& out) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    float rec[256];
    size_t got;
    while ((got = std::fread(rec, 4, 256, f)) > 0) out.insert(out.end(), rec, rec + got);
    std::fclose(f);
    return true;
}

static inline bool write_floats(const char* path, const std::vector<float>& v) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), 4, v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static inline uint64_t next_u64() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 11;
}
static inline float uniform() { return (float)((double)next_u64() / 4503599627370496.0 - 1.0); }  // [-1, 1)

// Point i of an adjoint call through the kernels' own field_grad_item, with its eight element offsets (field_corners) checked against the
// grid, not trusted.  count: 0 for an outside point, else 8.  false: an offset left the grid.
static inline bool grad_point(const cgrt::FieldGradCall& Q, uint32_t i, size_t elements, uint64_t (&at)[8], float (&c)[8], int& count) {
    const cgrt::GridField& G = Q.grid;
    uint64_t base;
    count = 0;
    if (!cgrt::field_grad_item(Q, i, base, c)) return true;
    if (base >= elements || base % G.nx + 1u >= G.nx || base / G.nx % G.ny + 1u >= G.ny || base / G.nx / G.ny + 1u >= G.nz) return false;
    cgrt::field_corners(G, base, [&](const int k, const uint64_t e) { at[k] = e; });
    for (int k = 0; k < 8; k++)
        if (at[k] >= elements) return false;
    count = 8;
    return true;
}
// the adjoint call of these points and grads (either of gv, gg may be null) on g
static inline cgrt::FieldGradCall grad_call(const Grid& g, const float* pts, size_t n, const float* gv, const float* gg, bool clamp) {
    cgrt::FieldGradCall Q{};
    Q.grid = g.G;
    Q.points = pts;
    Q.n = (uint32_t)n;
    Q.clamp = clamp ? cgrt::kFieldClamp : 0u;
    Q.grad_value = gv;
    Q.grad_gradient = gg;
    return Q;
}
