// surface_sample_kernels.h -- host-callable launcher of the surface-sampling kernel in surface_sample_kernels.hip (include/cgrt.h
// cgrt_sample_surface*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cgrt_layout.h"
#include "surface_kernels.h"

namespace cgrt {

// The 32 bytes of a sample as the kernel writes them (include/cgrt.h CgrtSurfaceSample).
struct CgrtSurfaceSampleDev {
    float point[3];
    uint32_t mesh_id;
    uint32_t prim_id;
    float bary[3];
};
static_assert(sizeof(CgrtSurfaceSampleDev) == 32, "a sample is two 16-byte stores");

// One call, passed to the kernel by value: no host array is read behind the launch.  All pointers device memory.  Sample i of the launch
// is sample first + i of the stream (seed, strata).  thresholds: the ntris thresholds of surface_sample_builder.h, of which the kernel
// searches the first `last`; last == 0xffffffff: the scene is empty for sampling, nothing but the outputs is touched.  steps =
// ceil(log2(last + 1)): the trip count of the search, the same for every lane.  attr / out_attr: both or neither.
struct SampleArgs {
    const TriRecord* tris;        // SceneDev::tris
    const SurfaceLookup* lookup;  // ntris entries
    const uint32_t* thresholds;
    uint32_t last, steps;
    uint32_t n;                   // samples (<= 0x7fffffff)
    unsigned long long seed, first, strata;
    CgrtSurfaceSampleDev* out;
    const float* attr;            // nverts x channels, or NULL
    uint32_t channels;
    float* out_attr;              // n x channels, or NULL
    int vec4;                     // channels % 4 == 0 and attr, out_attr 16-byte aligned (surface_device.h surface_rows)
};
hipError_t launch_sample_surface(const SampleArgs& A, hipStream_t stream);

}  // namespace cgrt
