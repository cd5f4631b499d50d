// oct_vis.hpp — the arithmetic of probe visibility (include/mi355rt.h, "PROBE VISIBILITY"): the octahedral map of a direction, the bin of a
// depth sample, the Chebyshev weight of one probe for one query and the weighted lookup of one query in a probe grid.  ONE statement, compiled for the host
// (mi355rt_oct_encode, mi355rt_oct_texel, mi355rt_probe_visibility_one, mi355rt_probes_lookup_vis_one) and for the device (csrc/probes_vis.hip): f32,
// unfused (every file that includes this is built with -ffp-contract=off), expression for expression what raytracer-rs_amd/probes.py writes in numpy.  Only
// + - x / sqrt, comparisons and integer conversions: no floor, no pow, no transcendental function, so host and device agree on the bits.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "sh9.hpp"

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

// sh9_lookup with the weight of corner j  wj = (t * vis) * face  in the place of t.  The probes' helpers, the corner order and the read-out are sh9.hpp's.
// count(probe, k) -> u32, moment(probe, k, c) -> f32; without has_nrm nrm is not read (p_b = p and face = 1).  The cell and the fractions come from p.  A corner with
// t == 0, n == 0 or usable == 0 is skipped before anything of it is read, one whose wj is 0 like them.  Returns ok; rgb is 0 when no corner was used.
template <class N, class Sh, class Usable, class Cnt, class Mom>
__host__ __device__ __forceinline__ bool sh9_lookup_vis(const ShGrid& grid, N n, Sh sh, bool has_usable, Usable usable, uint32_t R, Cnt count, Mom moment, uint32_t flags,
                                                        float normal_bias, const float* p, const float* dir, bool has_nrm, const float* nrm, uint32_t mode, float* rgb)
{
    uint32_t i[3]; float f[3], pb[3];
    for (int a = 0; a < 3; ++a) {
        sh9_axis(p[a], grid.origin[a], grid.spacing[a], grid.counts[a], i[a], f[a]);
        pb[a] = has_nrm ? p[a] + normal_bias * nrm[a] : p[a];
    }
    const bool cheb = (flags & kVisChebyshev) != 0u, facing = (flags & kVisFacing) != 0u && has_nrm;
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
        float vis = 1.0f, face = 1.0f;
        if (cheb || facing) {
            const float vx = pb[0] - sh9_probe_pos(grid.origin[0], grid.spacing[0], c[0]);
            const float vy = pb[1] - sh9_probe_pos(grid.origin[1], grid.spacing[1], c[1]);
            const float vz = pb[2] - sh9_probe_pos(grid.origin[2], grid.spacing[2], c[2]);
            const float r = oct_length(vx, vy, vz);
            if (cheb) vis = oct_visibility(R, [&](uint32_t k) { return count(probe, k); }, [&](uint32_t k, int m) { return moment(probe, k, m); }, vx, vy, vz, r);
            if (facing && oct_length_fine(r)) face = oct_facing(vx, vy, vz, r, nrm[0], nrm[1], nrm[2]);
        }
        const float wj = (t * vis) * face;
        if (wj == 0.0f) continue;
        any = true;
        wsum += wj;
        const float s = wj * (kShSphere / (float)nj);
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
