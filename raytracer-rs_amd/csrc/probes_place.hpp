// probes_place.hpp — host entry points of csrc/probes_place.hip.  Every pointer is device memory; the launches are queued on the stream and return.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include "sh9.hpp"

namespace mi355rt {

struct PlaceConfig;      // probe_place.hpp: the layout of mi355rt_probe_place_config

// The survey reduce of mi355rt_probes_survey over one chunk of gather's chunk loop: cp points from point0 on x cs samples, entry s * cp + i.  rays6 (the
// directions) is the chunk's buffer, tuv and prim the closest hits of those rays (prim MISS or < ntri; tuv is read only for a hit), normals4 the scene's
// float4 per triangle.  The six outputs are the caller's whole arrays (fresh: they start empty); a record is 4 floats and its array 16-byte aligned.
hipError_t launch_probes_survey(hipStream_t stream, uint32_t point0, uint32_t cp, uint32_t cs, bool fresh, bool flip, float max_distance, uint32_t ntri, const float* rays6,
                                const float* tuv, const uint32_t* prim, const void* normals4, uint32_t* out_n, uint32_t* out_back, uint32_t* out_front, float* out_near_back,
                                float* out_near_front, float* out_far);
// mi355rt_probes_place: offsets (null: zero) -> new_offsets (may be offsets itself), verdict and state of nprobes probes; any of the three outputs may be null
hipError_t launch_probes_place(hipStream_t stream, const ShGrid& grid, const PlaceConfig& cfg, uint32_t nprobes, const uint32_t* n, const uint32_t* back, const uint32_t* front,
                               const float* near_back, const float* near_front, const float* far, const float* offsets, float* new_offsets, uint8_t* verdict, uint8_t* state);
// mi355rt_probes_lookup_placed: launch_probes_lookup_vis with the probes' offsets (nprobes x 3, may be null)
hipError_t launch_probes_lookup_placed(hipStream_t stream, const ShGrid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, uint32_t R, const uint32_t* count,
                                       const float* moments, const float* offsets, uint32_t flags, float normal_bias, const float* points3, const float* dirs3,
                                       const float* normals3, size_t nq, uint32_t mode, float* rgb3, uint8_t* ok);

}  // namespace mi355rt
