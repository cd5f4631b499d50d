// probes_vis.hip — the device side of probe visibility (include/mi355rt.h, "PROBE VISIBILITY"): the depth film of a gather chunk's traced
// samples over an octahedral map per probe (mi355rt_probes_gather_depth), and the visibility-weighted lookup of a probe grid (mi355rt_probes_lookup_vis).  The
// arithmetic is csrc/oct_vis.hpp and, for the lookup, csrc/sh9.hpp; the statement raytracer-rs_amd/probes.py.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "probes_vis.hpp"
#include "oct_vis.hpp"

namespace mi355rt {
namespace {
constexpr int kVisBlock = 256;
constexpr uint32_t kVisMiss = 0xFFFFFFFFu;      // prim of a ray that hit nothing, as the ray-fed pass writes it
}  // namespace

// Phase (a) of the depth reduce: one lane per chunk entry q computes the texel its direction falls into and the distance it records, once, into the chunk
// temporary.  Coalesced: 12 + 4 + 4 bytes in, 8 bytes out per lane.
__global__ __launch_bounds__(kVisBlock) void probes_depth_bin_kernel(uint32_t count, uint32_t R, float max_distance, const float* __restrict__ rays6, const float* __restrict__ tuv,
                                                                    const uint32_t* __restrict__ prim, uint2* __restrict__ bins)
{
    const uint32_t q = blockIdx.x * kVisBlock + threadIdx.x;
    if (q >= count) return;
    const size_t at = q;
    const uint32_t k = oct_texel(rays6[6 * at + 3], rays6[6 * at + 4], rays6[6 * at + 5], R);
    const float dist = oct_depth(prim[at] != kVisMiss, tuv[3 * at], max_distance);
    bins[at] = make_uint2(k, __float_as_uint(dist));
}

// Phase (b): the shape problem is probes_project_kernel's — few points, many samples, f32 sums that must keep sample order — and so is the answer: the lanes
// split the SUMS, not the samples.  One lane per (point, texel) walks the chunk's samples of its point in order and adds those whose texel is its own, with
// count, m0 and m1 in registers; it loads and stores its 12 bytes once per chunk.  The R * R lanes of a point read the same 8-byte entry, so at R = 8 a wave
// issues one uniform load per sample and at R = 16 a block does.  fresh: the outputs start from 0.
__global__ __launch_bounds__(kVisBlock) void probes_depth_sum_kernel(uint32_t point0, uint32_t cp, uint32_t cs, int fresh, uint32_t RR, const uint2* __restrict__ bins,
                                                                    uint32_t* out_count, float* out_moments)
{
    const uint64_t e = (uint64_t)blockIdx.x * kVisBlock + threadIdx.x;
    if (e >= (uint64_t)cp * RR) return;
    const uint32_t i = (uint32_t)(e / RR), k = (uint32_t)(e - (uint64_t)i * RR);
    const size_t o = ((size_t)point0 + i) * RR + k;
    uint32_t c = 0u;
    float m0 = 0.0f, m1 = 0.0f;
    if (!fresh) { c = out_count[o]; m0 = out_moments[2 * o]; m1 = out_moments[2 * o + 1]; }
    for (uint32_t s = 0; s < cs; ++s) {
        const uint2 b = bins[(size_t)s * cp + i];
        if (b.x == k) {
            const float dist = __uint_as_float(b.y);
            c += 1u; m0 += dist; m1 += dist * dist;
        }
    }
    out_count[o] = c; out_moments[2 * o] = m0; out_moments[2 * o + 1] = m1;
}

// One lane per query: sh9_lookup_vis with the corner loop outside and the 27 running values in registers, as probes_lookup_kernel.  Per corner it adds three
// subtractions, a square root, the encode's two divisions and four 12-byte texel reads; neighbouring queries share corners and, with them, texels.
__global__ __launch_bounds__(kVisBlock) void probes_lookup_vis_kernel(ShGrid grid, const uint32_t* __restrict__ n, const float* __restrict__ sh, const uint8_t* __restrict__ usable,
                                                                     uint32_t R, const uint32_t* __restrict__ count, const float* __restrict__ moments, uint32_t flags,
                                                                     float normal_bias, const float* __restrict__ points3, const float* __restrict__ dirs3,
                                                                     const float* __restrict__ normals3, uint64_t nq, uint32_t mode, float* __restrict__ rgb3,
                                                                     uint8_t* __restrict__ ok)
{
    const uint64_t q = (uint64_t)blockIdx.x * kVisBlock + threadIdx.x;
    if (q >= nq) return;
    const float p[3] = { points3[3 * q], points3[3 * q + 1], points3[3 * q + 2] };
    const float d[3] = { dirs3[3 * q], dirs3[3 * q + 1], dirs3[3 * q + 2] };
    float nr[3] = { 0.0f, 0.0f, 0.0f };
    if (normals3 != nullptr) { nr[0] = normals3[3 * q]; nr[1] = normals3[3 * q + 1]; nr[2] = normals3[3 * q + 2]; }
    const size_t RR = (size_t)R * R;
    float rgb[3];
    const bool used = sh9_lookup_vis(grid, [n](size_t j) { return n[j]; }, [sh](size_t j, int c) { return sh[27 * j + c]; }, usable != nullptr,
                                     [usable](size_t j) { return usable[j] != 0; }, R, [count, RR](size_t j, uint32_t k) { return count[j * RR + k]; },
                                     [moments, RR](size_t j, uint32_t k, int m) { return moments[2 * (j * RR + k) + m]; }, flags, normal_bias, p, d,
                                     normals3 != nullptr, nr, mode, rgb);
    rgb3[3 * q] = rgb[0]; rgb3[3 * q + 1] = rgb[1]; rgb3[3 * q + 2] = rgb[2];
    if (ok != nullptr) ok[q] = used ? 1 : 0;
}

hipError_t launch_probes_depth(hipStream_t stream, uint32_t point0, uint32_t cp, uint32_t cs, bool fresh, uint32_t R, float max_distance, const float* rays6, const float* tuv,
                               const uint32_t* prim, uint2* bins, uint32_t* out_count, float* out_moments)
{
    if (cp == 0) return hipSuccess;
    const uint32_t entries = cp * cs, RR = R * R;              // entries < 2^32: the chunk is one ray-fed pass
    hipLaunchKernelGGL(probes_depth_bin_kernel, dim3((entries + kVisBlock - 1) / kVisBlock), dim3(kVisBlock), 0, stream, entries, R, max_distance, rays6, tuv, prim, bins);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint64_t lanes = (uint64_t)cp * RR;
    if ((lanes + kVisBlock - 1) / kVisBlock > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probes_depth_sum_kernel, dim3((unsigned)((lanes + kVisBlock - 1) / kVisBlock)), dim3(kVisBlock), 0, stream, point0, cp, cs, fresh ? 1 : 0, RR, bins, out_count,
                       out_moments);
    return hipGetLastError();
}

hipError_t launch_probes_lookup_vis(hipStream_t stream, const ShGrid& grid, const uint32_t* n, const float* sh, const uint8_t* usable, uint32_t R, const uint32_t* count,
                                    const float* moments, uint32_t flags, float normal_bias, const float* points3, const float* dirs3, const float* normals3, size_t nq,
                                    uint32_t mode, float* rgb3, uint8_t* ok)
{
    if (nq == 0) return hipSuccess;
    if ((nq + kVisBlock - 1) / kVisBlock > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probes_lookup_vis_kernel, dim3((unsigned)((nq + kVisBlock - 1) / kVisBlock)), dim3(kVisBlock), 0, stream, grid, n, sh, usable, R, count, moments, flags,
                       normal_bias, points3, dirs3, normals3, (uint64_t)nq, mode, rgb3, ok);
    return hipGetLastError();
}

}  // namespace mi355rt
