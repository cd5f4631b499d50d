// probes.hip — the device side of probes (include/mi355rt.h, "PROBES"): the projection of a gather chunk's traced samples onto the nine
// real spherical harmonics up to band 2 (mi355rt_probes_gather), and the trilinear lookup of a probe grid (mi355rt_probes_lookup).  The arithmetic is
// csrc/sh9.hpp, the statement raytracer-rs_amd/probes.py.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "probes.hpp"
#include "sh9.hpp"

namespace mi355rt {
namespace {
constexpr int kProbesBlock = 256;
constexpr uint32_t kProbeMiss = 0xFFFFFFFFu;      // prim of a ray that hit nothing, as the ray-fed pass writes it
}  // namespace

// The shape is the opposite of gather's: few points, many samples.  One lane per point would leave 4 096 probes on 64 waves, each walking its samples alone.
// Every sum (point, k, c) is independent of every other one, so the lanes split the COEFFICIENTS, not the samples: one lane per (point, k) with the three
// channel sums in registers walks the chunk's samples in order, and the order (hence the bits) of every sum is the statement's.  The nine lanes of a point
// read the same 12-byte direction and the same 12-byte rgb; a wave covers seven or eight neighbouring points, whose entries are adjacent in the chunk.
// Lane k == 0 also counts n, hits and near.  fresh: the outputs start from 0.  Any output may be null.
__global__ __launch_bounds__(kProbesBlock) void probes_project_kernel(uint32_t point0, uint32_t cp, uint32_t cs, int fresh, float near_distance,
                                                                     const float* __restrict__ rays6, const float* __restrict__ rgb, const float* __restrict__ tuv,
                                                                     const uint32_t* __restrict__ prim, uint32_t* out_n, uint32_t* out_hits, uint32_t* out_near, float* out_sh)
{
    const uint64_t e = (uint64_t)blockIdx.x * kProbesBlock + threadIdx.x;
    if (e >= (uint64_t)cp * 9u) return;
    const uint32_t i = (uint32_t)(e / 9u), k = (uint32_t)(e - 9ull * i);
    const size_t gp = (size_t)point0 + i;
    const bool first = k == 0u, hitq = first && (out_hits != nullptr || out_near != nullptr);
    float* o = out_sh != nullptr ? out_sh + (gp * 9u + k) * 3u : nullptr;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    uint32_t n = 0u, hits = 0u, near = 0u;
    if (!fresh) {
        if (o) { s0 = o[0]; s1 = o[1]; s2 = o[2]; }
        if (first) {
            if (out_n) n = out_n[gp];
            if (out_hits) hits = out_hits[gp];
            if (out_near) near = out_near[gp];
        }
    }
    for (uint32_t s = 0; s < cs; ++s) {
        const size_t q = (size_t)s * cp + i;
        if (o) {
            const float b = sh9_basis_at(k, rays6[6 * q + 3], rays6[6 * q + 4], rays6[6 * q + 5]);
            s0 += b * rgb[3 * q]; s1 += b * rgb[3 * q + 1]; s2 += b * rgb[3 * q + 2];
        }
        if (hitq && prim[q] != kProbeMiss) {
            hits += 1u;
            if (tuv[3 * q] < near_distance) near += 1u;
        }
    }
    n += cs;
    if (o) { o[0] = s0; o[1] = s1; o[2] = s2; }
    if (first) {
        if (out_n) out_n[gp] = n;
        if (out_hits) out_hits[gp] = hits;
        if (out_near) out_near[gp] = near;
    }
}

// One lane per query: sh9_lookup with the corner loop outside and the 27 running values in registers.  Neighbouring queries share corners, so the eight
// 108-byte coefficient blocks of a cell come through the caches for most of a wave.
__global__ __launch_bounds__(kProbesBlock) void probes_lookup_kernel(ShGrid grid, const uint32_t* __restrict__ n, const float* __restrict__ sh, const uint8_t* __restrict__ usable,
                                                                    const float* __restrict__ points3, const float* __restrict__ dirs3, uint64_t nq, uint32_t mode,
                                                                    float* __restrict__ rgb3, uint8_t* __restrict__ ok)
{
    const uint64_t q = (uint64_t)blockIdx.x * kProbesBlock + threadIdx.x;
    if (q >= nq) return;
    const float p[3] = { points3[3 * q], points3[3 * q + 1], points3[3 * q + 2] };
    const float d[3] = { dirs3[3 * q], dirs3[3 * q + 1], dirs3[3 * q + 2] };
    float rgb[3];
    const bool used = sh9_lookup(grid, [n](size_t j) { return n[j]; }, [sh](size_t j, int c) { return sh[27 * j + c]; }, usable != nullptr,
                                 [usable](size_t j) { return usable[j] != 0; }, p, d, mode, rgb);
    rgb3[3 * q] = rgb[0]; rgb3[3 * q + 1] = rgb[1]; rgb3[3 * q + 2] = rgb[2];
    if (ok != nullptr) ok[q] = used ? 1 : 0;
}

hipError_t launch_probes_project(hipStream_t stream, uint32_t point0, uint32_t cp, uint32_t cs, bool fresh, float near_distance, const float* rays6, const float* rgb,
                                 const float* tuv, const uint32_t* prim, uint32_t* out_n, uint32_t* out_hits, uint32_t* out_near, float* out_sh)
{
    if (cp == 0) return hipSuccess;
    const uint64_t lanes = (uint64_t)cp * 9u;
    hipLaunchKernelGGL(probes_project_kernel, dim3((unsigned)((lanes + kProbesBlock - 1) / kProbesBlock)), dim3(kProbesBlock), 0, stream, point0, cp, cs, fresh ? 1 : 0, near_distance,
                       rays6, rgb, tuv, prim, out_n, out_hits, out_near, out_sh);
    return hipGetLastError();
}

hipError_t launch_probes_lookup(hipStream_t stream, const ShGrid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, const float* points3, const float* dirs3,
                                size_t nq, uint32_t mode, float* rgb3, uint8_t* ok)
{
    if (nq == 0) return hipSuccess;
    if ((nq + kProbesBlock - 1) / kProbesBlock > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probes_lookup_kernel, dim3((unsigned)((nq + kProbesBlock - 1) / kProbesBlock)), dim3(kProbesBlock), 0, stream, grid, n, sh, usable, points3, dirs3,
                       (uint64_t)nq, mode, rgb3, ok);
    return hipGetLastError();
}

}  // namespace mi355rt
