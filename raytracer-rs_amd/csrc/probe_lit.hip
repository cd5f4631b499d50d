// probe_lit.hip — the device side of probe-lit shading (include/mi355rt.h, "PROBE-LIT"): the shadow rays of a chunk of closest hits, the
// reference's shade() at every hit plus the hemisphere mean of a probe volume there (mi355rt_probe_lit_rays), and that mean at caller-given surface points
// (mi355rt_probe_lit_points).  The arithmetic is csrc/probe_lit_math.hpp, the statement raytracer-rs_amd/probe_lit.py.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "probe_lit.hpp"
#include "probe_lit_math.hpp"
#include "bake_raster.hpp"
#include "device_math.hpp"

namespace mi355rt {
namespace {
constexpr int kLitBlock = 256;
constexpr uint32_t kLitMiss = 0xFFFFFFFFu;      // prim of a ray that hit nothing, as intersect_kernel writes it
constexpr float kLitNowhere = 1e30f;            // where the shadow-ray row of a miss starts: beyond every scene, finite

__device__ __forceinline__ bool lit_hemi(const LitVolume& v, bool clamp, const float* p, const float* nrm, float* out)
{
    const uint32_t* n = v.n; const float* sh = v.sh; const uint8_t* usable = v.usable; const uint32_t* count = v.count; const float* moments = v.moments; const float* offsets = v.offsets;
    const size_t RR = (size_t)v.R * v.R;
    return hemi_one(v.grid, [n](size_t j) { return n[j]; }, [sh](size_t j, int c) { return sh[27 * j + c]; }, usable != nullptr, [usable](size_t j) { return usable[j] != 0; }, v.R,
                    [count, RR](size_t j, uint32_t k) { return count[j * RR + k]; }, [moments, RR](size_t j, uint32_t k, int m) { return moments[2 * (j * RR + k) + m]; },
                    offsets != nullptr, [offsets](size_t j, int a) { return offsets[3 * j + a]; }, v.flags, v.normal_bias, p, nrm, clamp, out);
}
}  // namespace

// One lane per ray of the chunk: P from (ray, t), then per light the row li * cn + i of the chunk's shadow-ray buffer.  A wave writes 64 consecutive 24-byte
// rows per light.  Nobody reads the verdict of a miss's row, so it only has to be cheap to trace: it starts at kLitNowhere on every axis and runs away from the
// scene along (1, 1, 1), so every box lies behind it and the walk ends at the root.  A row of zeros is the costly choice: to the box tests a null direction
// passes every box (traverse.hpp, ray_init), so such a row walks the whole tree (measured on thai2: DESIGN.md §3r).
__global__ __launch_bounds__(kLitBlock) void probe_lit_surface_kernel(const DLight* __restrict__ lights, uint32_t nlights, uint32_t ntri, const float* __restrict__ rays6,
                                                                     const float* __restrict__ tuv, const uint32_t* __restrict__ prim, uint32_t cn, float* __restrict__ shadow6)
{
    const uint32_t i = blockIdx.x * kLitBlock + threadIdx.x;
    if (i >= cn) return;
    const uint32_t p = prim[i];
    const bool hit = p != kLitMiss && p < ntri;
    float P[3] = { 0.0f, 0.0f, 0.0f };
    if (hit) {
        const float o[3] = { rays6[6ull * i], rays6[6ull * i + 1], rays6[6ull * i + 2] }, d[3] = { rays6[6ull * i + 3], rays6[6ull * i + 4], rays6[6ull * i + 5] };
        lit_point(o, d, tuv[3ull * i], P);
    }
    for (uint32_t li = 0; li < nlights; ++li) {
        float r[6] = { kLitNowhere, kLitNowhere, kLitNowhere, 1.0f, 1.0f, 1.0f };
        if (hit) {
            const DLight lt = lights[li];
            const float lp[3] = { lt.px, lt.py, lt.pz };
            lit_shadow_ray(P, lp, r);
        }
        float* dst = shadow6 + 6ull * ((size_t)li * cn + i);
        for (int k = 0; k < 6; ++k) dst[k] = r[k];
    }
}

// One lane per ray of the chunk, consecutive lanes on consecutive rows: the ray, its hit and its lights' verdicts come in whole cache lines; the triangle's
// float4 normal, its material and (where textured) one texel are the scattered reads of shade(), and per used corner hemi_one reads n, usable, three offset
// words, the depth texels of oct_visibility and the first 48 bytes of the probe's coefficients.  Twelve running values; no LDS.
__global__ __launch_bounds__(kLitBlock) void probe_lit_shade_kernel(DScene sc, LitVolume vol, int clamp, const float* __restrict__ rays6, const float* __restrict__ tuv,
                                                                   const uint32_t* __restrict__ prim, const uint8_t* __restrict__ blocked, uint32_t cn, LitOutputs out)
{
    const uint32_t i = blockIdx.x * kLitBlock + threadIdx.x;
    if (i >= cn) return;
    const uint32_t p = prim[i];
    const bool hit = p != kLitMiss && p < sc.ntri;
    float light[3] = { 0.0f, 0.0f, 0.0f }, ind[3] = { 0.0f, 0.0f, 0.0f };
    bool used = false;
    if (hit) {
        const float o[3] = { rays6[6ull * i], rays6[6ull * i + 1], rays6[6ull * i + 2] }, d[3] = { rays6[6ull * i + 3], rays6[6ull * i + 4], rays6[6ull * i + 5] };
        const float t = tuv[3ull * i], u = tuv[3ull * i + 1], v = tuv[3ull * i + 2];
        float P[3];
        lit_point(o, d, t, P);
        const float4 nq = reinterpret_cast<const float4*>(sc.normals)[p];
        const float N[3] = { nq.x, nq.y, nq.z };
        if (out.rgb != nullptr || out.light != nullptr) {
            const DMaterial m = sc.materials[__float_as_uint(nq.w)];
            float diffuse[3] = { m.r, m.g, m.b };
            if (m.kind_tex & 0x80000000u) {
                const DTexture tx = sc.textures[m.kind_tex & 0x7FFFFFFFu];
                const float* q = sc.texels + 3ull * (tx.offset + bake_texel_index(tx.width, tx.height, u, v));
                diffuse[0] = q[0]; diffuse[1] = q[1]; diffuse[2] = q[2];
            }
            const DLight* lights = sc.lights;
            shade_one(P, N, d, diffuse, sc.nlights,
                      [lights](uint32_t li, float* lp, float* lc) { const DLight lt = lights[li]; lp[0] = lt.px; lp[1] = lt.py; lp[2] = lt.pz; lc[0] = lt.cr; lc[1] = lt.cg; lc[2] = lt.cb; },
                      [blocked, cn, i](uint32_t li) { return blocked[(size_t)li * cn + i] != 0; }, [](float x) { return pow32(x); }, light);
        }
        if (out.rgb != nullptr || out.indirect != nullptr || out.ok != nullptr) used = lit_hemi(vol, clamp != 0, P, N, ind);
        if (out.tuv != nullptr) { out.tuv[3ull * i] = t; out.tuv[3ull * i + 1] = u; out.tuv[3ull * i + 2] = v; }
    }
    if (out.rgb != nullptr) { out.rgb[3ull * i] = light[0] + ind[0]; out.rgb[3ull * i + 1] = light[1] + ind[1]; out.rgb[3ull * i + 2] = light[2] + ind[2]; }
    if (out.light != nullptr) { out.light[3ull * i] = light[0]; out.light[3ull * i + 1] = light[1]; out.light[3ull * i + 2] = light[2]; }
    if (out.indirect != nullptr) { out.indirect[3ull * i] = ind[0]; out.indirect[3ull * i + 1] = ind[1]; out.indirect[3ull * i + 2] = ind[2]; }
    if (out.prim != nullptr) out.prim[i] = hit ? p : kLitMiss;
    if (out.ok != nullptr) out.ok[i] = used ? 1 : 0;
}

// One lane per point: hemi_one at the caller's point and normal.
__global__ __launch_bounds__(kLitBlock) void probe_lit_points_kernel(LitVolume vol, int clamp, const float* __restrict__ points3, const float* __restrict__ normals3, uint64_t nq,
                                                                    float* __restrict__ indirect3, uint8_t* __restrict__ ok)
{
    const uint64_t q = (uint64_t)blockIdx.x * kLitBlock + threadIdx.x;
    if (q >= nq) return;
    const float p[3] = { points3[3 * q], points3[3 * q + 1], points3[3 * q + 2] };
    const float nr[3] = { normals3[3 * q], normals3[3 * q + 1], normals3[3 * q + 2] };
    float ind[3];
    const bool used = lit_hemi(vol, clamp != 0, p, nr, ind);
    indirect3[3 * q] = ind[0]; indirect3[3 * q + 1] = ind[1]; indirect3[3 * q + 2] = ind[2];
    if (ok != nullptr) ok[q] = used ? 1 : 0;
}

hipError_t launch_probe_lit_surface(hipStream_t stream, const DScene& sc, const float* rays6, const float* tuv, const uint32_t* prim, uint32_t cn, float* shadow6)
{
    if (cn == 0 || sc.nlights == 0) return hipSuccess;
    hipLaunchKernelGGL(probe_lit_surface_kernel, dim3((cn + kLitBlock - 1) / kLitBlock), dim3(kLitBlock), 0, stream, sc.lights, sc.nlights, sc.ntri, rays6, tuv, prim, cn, shadow6);
    return hipGetLastError();
}

hipError_t launch_probe_lit_shade(hipStream_t stream, const DScene& sc, const LitVolume& vol, bool clamp, const float* rays6, const float* tuv, const uint32_t* prim,
                                  const uint8_t* blocked, uint32_t cn, const LitOutputs& out)
{
    if (cn == 0) return hipSuccess;
    hipLaunchKernelGGL(probe_lit_shade_kernel, dim3((cn + kLitBlock - 1) / kLitBlock), dim3(kLitBlock), 0, stream, sc, vol, clamp ? 1 : 0, rays6, tuv, prim, blocked, cn, out);
    return hipGetLastError();
}

hipError_t launch_probe_lit_points(hipStream_t stream, const LitVolume& vol, bool clamp, const float* points3, const float* normals3, size_t npoints, float* indirect3, uint8_t* ok)
{
    if (npoints == 0) return hipSuccess;
    if ((npoints + kLitBlock - 1) / kLitBlock > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probe_lit_points_kernel, dim3((unsigned)((npoints + kLitBlock - 1) / kLitBlock)), dim3(kLitBlock), 0, stream, vol, clamp ? 1 : 0, points3, normals3,
                       (uint64_t)npoints, indirect3, ok);
    return hipGetLastError();
}

}  // namespace mi355rt
