// sh9.hpp — the arithmetic of probes (include/mi355rt.h, "PROBES"): the real spherical-harmonic basis up to band 2 and the lookup of one
// query in a probe grid.  ONE statement, compiled for the host (mi355rt_sh9_basis, mi355rt_probes_lookup_one, mi355rt_probe_grid_points) and for the device
// (csrc/probes.hip): f32, unfused (every file that includes this is built with -ffp-contract=off), expression for expression what
// raytracer-rs_amd/probes.py writes in numpy.  The basis is polynomial in the direction: no transcendental function, so host and device agree on the bits.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace mi355rt {

constexpr uint32_t kShRadiance = 0u, kShIrradiance = 1u;      // MI355RT_SH_*
constexpr float kSh0 = 0.282094792f, kSh1 = 0.488602512f, kSh2 = 1.092548431f, kSh3 = 0.315391565f, kSh4 = 0.546274215f;
constexpr float kShA0 = 3.14159265f, kShA1 = 2.09439510f, kShA2 = 0.785398163f;      // the cosine lobe's band factors: pi, 2 pi / 3, pi / 4
constexpr float kShSphere = 12.566370614f;                   // 4 pi: the sphere's area over which the table is uniform

struct ShGrid { float origin[3], spacing[3]; uint32_t counts[3]; };      // the layout of mi355rt_probe_grid

// b_0 .. b_8 of d = (x, y, z), used as given
__host__ __device__ __forceinline__ void sh9_basis(float x, float y, float z, float* b)
{
    b[0] = kSh0;
    b[1] = kSh1 * y;
    b[2] = kSh1 * z;
    b[3] = kSh1 * x;
    b[4] = kSh2 * (x * y);
    b[5] = kSh2 * (y * z);
    b[6] = kSh3 * (3.0f * (z * z) - 1.0f);
    b[7] = kSh2 * (x * z);
    b[8] = kSh4 * (x * x - y * y);
}

// b_k for a k that differs between the lanes of a wave: all nine, then selects — no branch and no indexed array
__host__ __device__ __forceinline__ float sh9_basis_at(uint32_t k, float x, float y, float z)
{
    float b[9];
    sh9_basis(x, y, z, b);
    return k == 0u ? b[0] : k == 1u ? b[1] : k == 2u ? b[2] : k == 3u ? b[3] : k == 4u ? b[4] : k == 5u ? b[5] : k == 6u ? b[6] : k == 7u ? b[7] : b[8];
}

// where probe i of one axis sits
__host__ __device__ __forceinline__ float sh9_probe_pos(float origin, float spacing, uint32_t i) { return origin + (float)i * spacing; }

// one axis of a query: the lower probe index i and the fraction f towards i + 1.  A NaN coordinate becomes 0: no index is ever made from a NaN
__host__ __device__ __forceinline__ void sh9_axis(float p, float origin, float spacing, uint32_t count, uint32_t& i, float& f)
{
    float g = (p - origin) / spacing;
    g = g >= 0.0f ? g : 0.0f;
    const float top = (float)(count - 1u);
    g = g <= top ? g : top;
    i = (uint32_t)g;
    if (count >= 2u && i > count - 2u) i = count - 2u;
    f = g - (float)i;
    if (count == 1u) { i = 0u; f = 0.0f; }
}

// The lookup of one query (p, dir).  n(probe) -> u32, sh(probe, k * 3 + c) -> f32, usable(probe) -> bool (asked only with has_usable).  The corner loop is
// outside and the 27 running values stay in registers.  A skipped corner is never read into a sum.  Returns ok; rgb is 0 when no corner was used.
template <class N, class Sh, class Usable>
__host__ __device__ __forceinline__ bool sh9_lookup(const ShGrid& grid, N n, Sh sh, bool has_usable, Usable usable, const float* p, const float* dir, uint32_t mode, float* rgb)
{
    uint32_t i[3]; float f[3];
    for (int a = 0; a < 3; ++a) sh9_axis(p[a], grid.origin[a], grid.spacing[a], grid.counts[a], i[a], f[a]);
    float C[27];
    for (int q = 0; q < 27; ++q) C[q] = 0.0f;
    float wsum = 0.0f;
    bool any = false;
    for (uint32_t j = 0; j < 8u; ++j) {
        uint32_t c[3]; float w[3];
        for (int a = 0; a < 3; ++a) {
            const bool up = ((j >> a) & 1u) != 0u;
            c[a] = up ? (i[a] + 1u <= grid.counts[a] - 1u ? i[a] + 1u : grid.counts[a] - 1u) : i[a];
            w[a] = up ? f[a] : 1.0f - f[a];
        }
        const float t = (w[0] * w[1]) * w[2];
        if (t == 0.0f) continue;
        const size_t probe = ((size_t)c[2] * grid.counts[1] + c[1]) * grid.counts[0] + c[0];
        const uint32_t nj = n(probe);
        if (nj == 0u) continue;
        if (has_usable && !usable(probe)) continue;
        any = true;
        wsum += t;
        const float s = t * (kShSphere / (float)nj);
        for (int q = 0; q < 27; ++q) C[q] += s * sh(probe, q);
    }
    if (!any) { rgb[0] = 0.0f; rgb[1] = 0.0f; rgb[2] = 0.0f; return false; }
    float b[9];
    sh9_basis(dir[0], dir[1], dir[2], b);
    float r[3] = { 0.0f, 0.0f, 0.0f };
    if (mode == kShIrradiance) {
        for (int k = 0; k < 9; ++k) {
            const float A = k == 0 ? kShA0 : k < 4 ? kShA1 : kShA2;
            for (int ch = 0; ch < 3; ++ch) r[ch] += (A * C[3 * k + ch]) * b[k];
        }
    } else {
        for (int k = 0; k < 9; ++k)
            for (int ch = 0; ch < 3; ++ch) r[ch] += C[3 * k + ch] * b[k];
    }
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = r[ch] / wsum;
    return true;
}

}  // namespace mi355rt
