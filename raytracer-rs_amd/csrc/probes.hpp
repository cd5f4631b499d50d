// probes.hpp — host entry points of csrc/probes.hip.  Every pointer is device memory; both launches are queued on the stream and return.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include "sh9.hpp"

namespace mi355rt {

// The reduce of mi355rt_probes_gather over one chunk of gather's chunk loop: cp points from point0 on x cs samples, entry s * cp + i.  rays6 (the directions),
// rgb, tuv and prim are the chunk's buffers, out_* the caller's whole arrays (any may be null; fresh: they start from 0).  rgb is read only for out_sh, tuv and
// prim only for out_hits / out_near.
hipError_t launch_probes_project(hipStream_t stream, uint32_t point0, uint32_t cp, uint32_t cs, bool fresh, float near_distance, const float* rays6, const float* rgb,
                                 const float* tuv, const uint32_t* prim, uint32_t* out_n, uint32_t* out_hits, uint32_t* out_near, float* out_sh);
// mi355rt_probes_lookup: nq queries (points3, dirs3) into rgb3 (and ok, which may be null); usable may be null
hipError_t launch_probes_lookup(hipStream_t stream, const ShGrid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, const float* points3, const float* dirs3,
                                size_t nq, uint32_t mode, float* rgb3, uint8_t* ok);

}  // namespace mi355rt
