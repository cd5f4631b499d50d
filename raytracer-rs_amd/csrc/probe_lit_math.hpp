// probe_lit_math.hpp — the arithmetic of probe-lit shading (include/mi355rt.h, "PROBE-LIT"): the hemisphere mean of a probe volume at one
// surface point and the reference's shade() at one hit.  ONE statement, compiled for the host (mi355rt_probe_lit_one) and for the device
// (csrc/probe_lit.hip): f32, unfused (every file that includes this is built with -ffp-contract=off), expression for expression what
// raytracer-rs_amd/probe_lit.py writes in numpy.  hemi_one needs only + - x / sqrt, comparisons and integer conversions; shade_one adds the caller's pow32.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "sh9.hpp"
#include "oct_vis.hpp"

namespace mi355rt {

constexpr uint32_t kProbeLitClamp = 1u;                      // MI355RT_PROBE_LIT_CLAMP
constexpr float kHemiBand1 = 0.5f;                           // the uniform hemisphere mean as a zonal convolution: band factors 1, 1/2, 0

// The uniform mean over the hemisphere of nrm of the radiance field a probe grid holds, at p.  The corners are sh9_corners' (sh9.hpp) with offsets and
// dir = normal = nrm; with flags 0 nothing of the depth films or the offsets is read and wj is t.  Of a used corner only coefficients 0 .. 3 are read:
// sh(probe, k * 3 + c) is asked for k * 3 + c < 12 only.  The read-out is its own: band factors 1, 1/2, 0.  Returns ok; out is 0 when no corner was used.
// clamp: a value that is not >= 0 (a NaN too) becomes +0.
template <class N, class Sh, class Usable, class Cnt, class Mom, class Off>
__host__ __device__ __forceinline__ bool hemi_one(const ShGrid& grid, N n, Sh sh, bool has_usable, Usable usable, uint32_t R, Cnt count, Mom moment, bool has_off, Off offset,
                                                  uint32_t flags, float normal_bias, const float* p, const float* nrm, bool clamp, float* out)
{
    return sh9_corners<12, true, true>(grid, n, sh, has_usable, usable, R, count, moment, has_off, offset, flags, normal_bias, p, true, nrm, nullptr, 0u, nullptr,
                                       [&](bool any, const float* C, float wsum) {
        if (!any) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; return; }
        float b[9];
        sh9_basis(nrm[0], nrm[1], nrm[2], b);
        for (int ch = 0; ch < 3; ++ch) {
            float m = 0.0f;
            m += C[ch] * b[0];
            for (int k = 1; k < 4; ++k) m += (kHemiBand1 * C[3 * k + ch]) * b[k];
            const float x = m / wsum;
            out[ch] = clamp ? (x >= 0.0f ? x : 0.0f) : x;
        }
    });
}

// the hit point of a ray (o, d) at t: one multiply and one add per axis (mod.rs:212)
__host__ __device__ __forceinline__ void lit_point(const float* o, const float* d, float t, float* P)
{
    P[0] = o[0] + t * d[0]; P[1] = o[1] + t * d[1]; P[2] = o[2] + t * d[2];
}

// l = light - P and the shadow ray (P + l * 0.01f, l) of mod.rs:215, 224-225
__host__ __device__ __forceinline__ void lit_shadow_ray(const float* P, const float* light, float* ray6)
{
    for (int a = 0; a < 3; ++a) {
        const float l = light[a] - P[a];
        ray6[a] = P[a] + l * 0.01f;
        ray6[3 + a] = l;
    }
}

// shade() of the reference (mod.rs:207-261) at a hit: P the hit point, N the triangle's normal, d the ray's direction as given, diffuse the material's colour or
// its texel.  light(li, pos3, colour3) fills a light, blocked(li) is mi355rt_occluded_rays' verdict of its shadow ray (asked only for a light with ndl >= 0 or
// a NaN ndl), pow32(x) is x.powf(32.0): five squarings in f64 and one rounding.  The sum runs from +0.0f over the lights in scene order, vecmath.rs operation
// order throughout.
template <class Light, class Blocked, class Pow>
__host__ __device__ __forceinline__ void shade_one(const float* P, const float* N, const float* d, const float* diffuse, uint32_t nlights, Light light, Blocked blocked, Pow pow32,
                                                   float* out)
{
    float acc[3] = { 0.0f, 0.0f, 0.0f };
    const float dl = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float view[3] = { d[0] / dl, d[1] / dl, d[2] / dl };                              // mod.rs:251
    for (uint32_t li = 0; li < nlights; ++li) {
        float lp[3], lc[3];
        light(li, lp, lc);
        const float l[3] = { lp[0] - P[0], lp[1] - P[1], lp[2] - P[2] };                    // mod.rs:215
        const float len = sqrtf(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
        const float ln[3] = { l[0] / len, l[1] / len, l[2] / len };
        const float ndl = N[0] * ln[0] + N[1] * ln[1] + N[2] * ln[2];                       // mod.rs:216
        if (ndl < 0.0f) continue;                                                           // mod.rs:218
        if (blocked(li)) continue;                                                          // mod.rs:226-232
        const float k = 2.0f * ndl;
        const float refl[3] = { k * N[0] - ln[0], k * N[1] - ln[1], k * N[2] - ln[2] };     // mod.rs:252-253
        const float spec = pow32(view[0] * refl[0] + view[1] * refl[1] + view[2] * refl[2]);   // mod.rs:255, SPECULAR = white
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (diffuse[c] * ndl + spec) * lc[c];    // mod.rs:254-257
    }
    out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2];
}

}  // namespace mi355rt
