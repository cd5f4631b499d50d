// probe_lit.hpp — host entry points of csrc/probe_lit.hip.  Every pointer is device memory; the launches are queued on the stream and return.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include "device_types.hpp"
#include "sh9.hpp"

namespace mi355rt {

// mi355rt_probe_volume as the kernels take it.  Without depth films count and moments are null, R, flags and normal_bias 0 and offsets null: then the corner
// weights are the trilinear factors and nothing but n, usable and sh is read.
struct LitVolume {
    ShGrid grid; const uint32_t* n; const float* sh; const uint8_t* usable; uint32_t R; const uint32_t* count; const float* moments; const float* offsets;
    uint32_t flags; float normal_bias;
};
// mi355rt_probe_lit_outputs of one chunk: any may be null
struct LitOutputs { float *rgb, *light, *indirect, *tuv; uint32_t* prim; uint8_t* ok; };

// The shadow rays of a chunk of cn rays with their closest hits (tuv, prim; prim MISS or < ntri): row li * cn + i = (P + l * 0.01f, l); for a miss a ray that is settled at the root (its verdict is never read).
hipError_t launch_probe_lit_surface(hipStream_t stream, const DScene& sc, const float* rays6, const float* tuv, const uint32_t* prim, uint32_t cn, float* shadow6);
// shade() and the hemisphere mean of the chunk's hits; blocked: the verdicts of the rows above.  Writes the outputs that are not null; tuv on a hit only.
hipError_t launch_probe_lit_shade(hipStream_t stream, const DScene& sc, const LitVolume& vol, bool clamp, const float* rays6, const float* tuv, const uint32_t* prim,
                                  const uint8_t* blocked, uint32_t cn, const LitOutputs& out);
// mi355rt_probe_lit_points: the hemisphere mean at npoints caller-given points and normals
hipError_t launch_probe_lit_points(hipStream_t stream, const LitVolume& vol, bool clamp, const float* points3, const float* normals3, size_t npoints, float* indirect3, uint8_t* ok);

}  // namespace mi355rt
