// oct_vis.hpp — the arithmetic of probe visibility (include/mi355rt.h, "PROBE VISIBILITY"): the octahedral map of a direction, the bin of a
// depth sample, and the two factors a probe's view of a query adds to its weight in a lookup: the Chebyshev weight and the facing term.  The lookup that
// uses them is sh9_corners (sh9.hpp, which includes this file).  ONE statement, compiled for the host (mi355rt_oct_encode, mi355rt_oct_texel,
// mi355rt_probe_visibility_one, mi355rt_probes_lookup_vis_one) and for the device (csrc/probes_vis.hip, probes_place.hip, probe_lit.hip): f32, unfused (every file that includes this is built with -ffp-contract=off), expression for expression what raytracer-rs_amd/probes.py writes in numpy.  Only
// + - x / sqrt, comparisons and integer conversions: no floor, no pow, no transcendental function, so host and device agree on the bits.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace mi355rt {

constexpr uint32_t kVisChebyshev = 1u, kVisFacing = 2u;      // MI355RT_VIS_*
constexpr uint32_t kOctResMin = 2u, kOctResMax = 16u;
constexpr float kOctMaxDistanceTop = 1e12f;                  // D^2 times 2^32 samples stays finite in f32

// a direction (x, y, z), used as given, on the unit square
__host__ __device__ __forceinline__ void oct_encode(float x, float y, float z, float& u, float& w)
{
    const float s = (__builtin_fabsf(x) + __builtin_fabsf(y)) + __builtin_fabsf(z);
    float px = x / s, py = y / s;
    if (z < 0.0f) {                                           // the lower half folds outwards, both from the old values
        const float fx = (1.0f - __builtin_fabsf(py)) * (x >= 0.0f ? 1.0f : -1.0f);
        const float fy = (1.0f - __builtin_fabsf(px)) * (y >= 0.0f ? 1.0f : -1.0f);
        px = fx; py = fy;
    }
    u = px * 0.5f + 0.5f;
    w = py * 0.5f + 0.5f;
}

// one axis of the bin of a sample.  u is in [0, 1] or a NaN, which becomes 0: no index is ever made from a NaN
__host__ __device__ __forceinline__ uint32_t oct_texel_axis(float u, uint32_t R)
{
    float g = u * (float)R;
    g = g >= 0.0f ? g : 0.0f;
    const uint32_t i = (uint32_t)g;
    return i < R - 1u ? i : R - 1u;
}

// the texel index iy * R + ix of a sample with direction (x, y, z)
__host__ __device__ __forceinline__ uint32_t oct_texel(float x, float y, float z, uint32_t R)
{
    float u, w;
    oct_encode(x, y, z, u, w);
    return oct_texel_axis(w, R) * R + oct_texel_axis(u, R);
}

// the distance a depth sample records: a miss and anything at or beyond D (a NaN t too) count as D
__host__ __device__ __forceinline__ float oct_depth(bool hit, float t, float D) { return hit ? (t < D ? t : D) : D; }

// an index pair outside [0, R - 1]^2 on the texel the octahedral map puts there: the x rule, then the y rule applied to its result
__host__ __device__ __forceinline__ void oct_wrap(int32_t R, int32_t& i, int32_t& j)
{
    if (i < 0) { i = 0; j = R - 1 - j; } else if (i >= R) { i = R - 1; j = R - 1 - j; }
    if (j < 0) { j = 0; i = R - 1 - i; } else if (j >= R) { j = R - 1; i = R - 1 - i; }
}

__host__ __device__ __forceinline__ float oct_length(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }
// a positive finite number: not 0, not a NaN, not an overflow to infinity
__host__ __device__ __forceinline__ bool oct_length_fine(float r) { return r > 0.0f && r <= 3.402823466e+38f; }

// The Chebyshev weight of one probe for v = (x, y, z) of length r (oct_length).  count(k) -> u32, moment(k, c) -> f32 of texel k.  A texel with zero weight
// or zero count is never read into a sum.
template <class Cnt, class Mom>
__host__ __device__ __forceinline__ float oct_visibility(uint32_t R, Cnt count, Mom moment, float x, float y, float z, float r)
{
    if (!oct_length_fine(r)) return 1.0f;
    float u, w;
    oct_encode(x, y, z, u, w);
    const float gx = u * (float)R + 0.5f, gy = w * (float)R + 0.5f;          // in [0.5, R + 0.5]: r is fine, so neither is a NaN
    const uint32_t ix = (uint32_t)gx, iy = (uint32_t)gy;
    const float fx = gx - (float)ix, fy = gy - (float)iy;
    float ws = 0.0f, a = 0.0f, b = 0.0f;
    for (int dj = 0; dj < 2; ++dj)
        for (int di = 0; di < 2; ++di) {
            const float wt = (di ? fx : 1.0f - fx) * (dj ? fy : 1.0f - fy);
            if (wt == 0.0f) continue;
            int32_t i = (int32_t)ix - 1 + di, j = (int32_t)iy - 1 + dj;
            oct_wrap((int32_t)R, i, j);
            const uint32_t k = (uint32_t)j * R + (uint32_t)i;
            const uint32_t c = count(k);
            if (c == 0u) continue;
            ws += wt;
            a += wt * (moment(k, 0) / (float)c);
            b += wt * (moment(k, 1) / (float)c);
        }
    if (ws == 0.0f) return 1.0f;                              // no information
    const float mean = a / ws, mean2 = b / ws;
    if (r <= mean) return 1.0f;
    const float var = __builtin_fabsf(mean2 - mean * mean), dd = r - mean;
    const float c = var / (var + dd * dd);
    return (c * c) * c;
}

// how much a surface with normal (nx, ny, nz) at distance r along v = (x, y, z) from a probe faces it
__host__ __device__ __forceinline__ float oct_facing(float x, float y, float z, float r, float nx, float ny, float nz)
{
    float q = ((((-x) * nx + (-y) * ny) + (-z) * nz) / r + 1.0f) * 0.5f;
    q = q >= 0.0001f ? q : 0.0001f;
    return q * q + 0.2f;
}

}  // namespace mi355rt
