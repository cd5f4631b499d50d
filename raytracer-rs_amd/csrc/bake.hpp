// bake.hpp — host entry points of csrc/bake.hip.  Every pointer is device memory unless it says otherwise; both calls wait for the stream
// before they return, and free their temporaries (counted into *hbm while they live).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include "device_types.hpp"

namespace mi355rt {

// mi355rt_bake_texels.  tri9: per scene triangle (A, B - A, C - A), read for `points` only; uv: ntri x 6; owner [w * h] and bary [w * h * 2] are always
// written (bary where covered only); ids / points / normals / albedo: the compact lists, any may be null; *ncovered (host memory): their length.
hipError_t bake_texels_device(hipStream_t stream, const DScene& sc, const float* tri9, const float* uv, uint32_t ntri, uint32_t width, uint32_t height, bool flip,
                              uint32_t* owner, float* bary, uint32_t* ids, float* points, float* normals, float* albedo, uint32_t* ncovered, size_t* hbm);
// mi355rt_bake_atlas.  *verdict (host memory): 0, or bit 0: an id >= width * height, bit 1: an id named twice — then nothing was written.
hipError_t bake_atlas_device(hipStream_t stream, const uint32_t* ids, const float* values, uint32_t n, uint32_t width, uint32_t height, uint32_t dilate,
                             float* atlas, uint8_t* valid, uint32_t* verdict, size_t* hbm);

}  // namespace mi355rt
