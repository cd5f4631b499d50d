// probes_vis.hpp — host entry points of csrc/probes_vis.hip.  Every pointer is device memory; the launches are queued on the stream and return.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include "sh9.hpp"

namespace mi355rt {

// The depth reduce of mi355rt_probes_gather_depth over one chunk of gather's chunk loop: cp points from point0 on x cs samples, entry s * cp + i.  rays6 (the
// directions), tuv and prim are the chunk's buffers; bins is a chunk temporary of cp * cs entries of 8 bytes (texel index, dist); out_count (npoints x R * R)
// and out_moments (npoints x R * R x 2) the caller's whole arrays (fresh: they start from 0).
hipError_t launch_probes_depth(hipStream_t stream, uint32_t point0, uint32_t cp, uint32_t cs, bool fresh, uint32_t R, float max_distance, const float* rays6, const float* tuv,
                               const uint32_t* prim, uint2* bins, uint32_t* out_count, float* out_moments);
// mi355rt_probes_lookup_vis: nq queries (points3, dirs3, normals3 or null) into rgb3 (and ok, which may be null); usable may be null
hipError_t launch_probes_lookup_vis(hipStream_t stream, const ShGrid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, uint32_t R, const uint32_t* count,
                                    const float* moments, uint32_t flags, float normal_bias, const float* points3, const float* dirs3, const float* normals3, size_t nq,
                                    uint32_t mode, float* rgb3, uint8_t* ok);

}  // namespace mi355rt
