// sh9.hpp — the arithmetic of probes (include/mi355rt.h, "PROBES"): the real spherical-harmonic basis up to band 2 and the lookup of one
// query in a probe grid.  The lookup is written ONCE for the whole probe family: sh9_corners is the corner loop of sh9_lookup, sh9_lookup_vis (both below),
// sh9_lookup_placed (probe_place.hpp) and hemi_one (probe_lit_math.hpp), and it ends in the 27-coefficient read-out of the three lookups; the four differ in
// sh9_corners' compile-time parameters alone.  ONE statement, compiled for the host (mi355rt_sh9_basis, mi355rt_probes_lookup*_one, mi355rt_probe_grid_points)
// and for the device (csrc/probes.hip, probes_vis.hip, probes_place.hip, probe_lit.hip): f32, unfused (every file that includes this is built with
// -ffp-contract=off), expression for expression what raytracer-rs_amd/probes.py writes in numpy.  The basis is polynomial in the direction: no transcendental
// function, so host and device agree on the bits.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "oct_vis.hpp"

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

// The corner loop of every lookup: the cell and the fractions of p, the eight corners in the order of j with their clamping, the skip rules and per used corner
//   wj = (t * vis) * face,  wsum += wj,  C[q] += (wj * (4 pi / n)) * sh(probe, q)  for q < kCoef.
// n(probe) -> u32, sh(probe, k * 3 + c) -> f32, usable(probe) -> bool (asked only with has_usable).  A corner with t == 0, n == 0 or usable == 0 is skipped before
// anything else of it is read, one whose wj is 0 like them: a skipped corner is never read into a sum.  The loop is outside and the kCoef running values stay in
// registers: they are this function's own array (summed into a caller's array behind a pointer, the device compiler leaves the corner loop rolled).  Returns
// any: whether a corner was used.  What follows the last corner depends on kCoef:
//   27: the read-out of the three lookups, written here: the basis of dir against the sums, as radiance or through the cosine lobe (mode), over wsum, into rgb,
//     which is 0 when no corner was used; use is not called.  It is not a function of its own: with any function around it, however its 27 inputs are
//     passed, probes_lookup_kernel comes out a tenth longer (profiles/probe_fold_kernel_resources.txt).
//   else: the caller's own read-out, use(any, C, wsum), called once; dir, mode and rgb are not touched.
//   kWeighted: vis and face exist (oct_vis.hpp): count(probe, k) -> u32, moment(probe, k, c) -> f32 of the probe's depth film of R x R texels, flags the
//     MI355RT_VIS_* bits.  v = p_b - position with p_b = p + normal_bias * nrm; without has_nrm nrm is not read (p_b = p and face = 1).  Without kWeighted
//     none of R .. nrm is touched and wj is t.
//   kOffsets: probes may have moved: position = (origin_a + (float)i_a * spacing_a) + offset_a, offset(probe, a) -> f32, asked only with has_off.  The cell,
//     the fractions and t stay the grid's.
template <int kCoef, bool kWeighted, bool kOffsets, class N, class Sh, class Usable, class Cnt, class Mom, class Off, class Use>
__host__ __device__ __forceinline__ bool sh9_corners(const ShGrid& grid, N n, Sh sh, bool has_usable, Usable usable, uint32_t R, Cnt count, Mom moment, bool has_off, Off offset,
                                                     uint32_t flags, float normal_bias, const float* p, bool has_nrm, const float* nrm, const float* dir, uint32_t mode, float* rgb,
                                                     Use use)
{
    uint32_t i[3]; float f[3], pb[3];
    for (int a = 0; a < 3; ++a) {
        sh9_axis(p[a], grid.origin[a], grid.spacing[a], grid.counts[a], i[a], f[a]);
        if constexpr (kWeighted) pb[a] = has_nrm ? p[a] + normal_bias * nrm[a] : p[a];
    }
    const bool cheb = kWeighted && (flags & kVisChebyshev) != 0u, facing = kWeighted && (flags & kVisFacing) != 0u && has_nrm;
    float C[kCoef];
    for (int q = 0; q < kCoef; ++q) C[q] = 0.0f;
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
        float wj = t;
        if constexpr (kWeighted) {
            float vis = 1.0f, face = 1.0f;
            if (cheb || facing) {
                float vx, vy, vz;                             // v = p_b - position, spelt per kOffsets as each kernel's parent spelt it, so that each keeps its code
                if constexpr (kOffsets) {
                    float pos[3];
                    for (int a = 0; a < 3; ++a) {
                        pos[a] = sh9_probe_pos(grid.origin[a], grid.spacing[a], c[a]);
                        if (has_off) pos[a] = pos[a] + offset(probe, a);
                    }
                    vx = pb[0] - pos[0]; vy = pb[1] - pos[1]; vz = pb[2] - pos[2];
                } else {
                    vx = pb[0] - sh9_probe_pos(grid.origin[0], grid.spacing[0], c[0]);
                    vy = pb[1] - sh9_probe_pos(grid.origin[1], grid.spacing[1], c[1]);
                    vz = pb[2] - sh9_probe_pos(grid.origin[2], grid.spacing[2], c[2]);
                }
                const float r = oct_length(vx, vy, vz);
                if (cheb) vis = oct_visibility(R, [&](uint32_t k) { return count(probe, k); }, [&](uint32_t k, int m) { return moment(probe, k, m); }, vx, vy, vz, r);
                if (facing && oct_length_fine(r)) face = oct_facing(vx, vy, vz, r, nrm[0], nrm[1], nrm[2]);
            }
            wj = (t * vis) * face;
            if (wj == 0.0f) continue;
        }
        any = true;
        wsum += wj;
        const float s = wj * (kShSphere / (float)nj);
        for (int q = 0; q < kCoef; ++q) C[q] += s * sh(probe, q);
    }
    if constexpr (kCoef != 27) {                                  // some other read-out: the caller's
        use(any, C, wsum);
        return any;
    } else {                                                      // the read-out of the three lookups
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
}

// The lookup of one query (p, dir): the trilinear weight alone.  Returns ok.
template <class N, class Sh, class Usable>
__host__ __device__ __forceinline__ bool sh9_lookup(const ShGrid& grid, N n, Sh sh, bool has_usable, Usable usable, const float* p, const float* dir, uint32_t mode, float* rgb)
{
    return sh9_corners<27, false, false>(grid, n, sh, has_usable, usable, 0u, nullptr, nullptr, false, nullptr, 0u, 0.0f, p, false, nullptr, dir, mode, rgb, nullptr);
}

// The lookup with the probes' depth films: every corner weighted by what the probe sees of the query.  Returns ok.
template <class N, class Sh, class Usable, class Cnt, class Mom>
__host__ __device__ __forceinline__ bool sh9_lookup_vis(const ShGrid& grid, N n, Sh sh, bool has_usable, Usable usable, uint32_t R, Cnt count, Mom moment, uint32_t flags,
                                                        float normal_bias, const float* p, const float* dir, bool has_nrm, const float* nrm, uint32_t mode, float* rgb)
{
    return sh9_corners<27, true, false>(grid, n, sh, has_usable, usable, R, count, moment, false, nullptr, flags, normal_bias, p, has_nrm, nrm, dir, mode, rgb, nullptr);
}

}  // namespace mi355rt
