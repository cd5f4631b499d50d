// probe_place.hpp — the arithmetic of probe placement (include/mi355rt.h, "PROBE PLACEMENT"): what one sample adds to a probe's survey, where
// a surveyed probe moves, the state it is given, and the lookup of one query in a grid whose probes have moved (sh9_corners of sh9.hpp with offsets).  ONE statement, compiled for the host
// (mi355rt_probe_place_one, mi355rt_probes_lookup_placed_one) and for the device (csrc/probes_place.hip): f32, unfused (every file that includes this is built
// with -ffp-contract=off), expression for expression what raytracer-rs_amd/probes.py writes in numpy.  Only + - x / sqrt, comparisons and integer conversions.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "sh9.hpp"
#include "oct_vis.hpp"

namespace mi355rt {

constexpr uint32_t kSurveyFlip = 1u;                                                         // MI355RT_SURVEY_FLIP
constexpr uint32_t kProbeUnknown = 0u, kProbeBuried = 1u, kProbeIdle = 2u, kProbeActive = 3u;   // MI355RT_PROBE_*
// MI355RT_PLACE_*: the branch that decided a probe's move, and bit 3 when its candidate was refused
constexpr uint32_t kPlaceUnsampled = 0u, kPlaceThrough = 1u, kPlaceAway = 2u, kPlaceStay = 3u, kPlaceBack = 4u, kPlaceRest = 5u, kPlaceRefused = 8u;
constexpr float kPlaceInf = __builtin_inff();

struct SurveyRecord { float dist, x, y, z; };               // a distance and the direction of the sample that set it: 16 bytes, the layout of the arrays
struct SurveyState { uint32_t n, back, front; SurveyRecord near_back, near_front, far; };
struct PlaceConfig { float back_share, max_offset, min_front, max_distance; };      // the layout of mi355rt_probe_place_config

__host__ __device__ __forceinline__ SurveyState survey_empty()
{
    return SurveyState{ 0u, 0u, 0u, { kPlaceInf, 0.0f, 0.0f, 0.0f }, { kPlaceInf, 0.0f, 0.0f, 0.0f }, { -kPlaceInf, 0.0f, 0.0f, 0.0f } };
}

// One sample of a probe, in sample order.  found: the ray's prim is not MISS; t is read only then, (nx, ny, nz) only for a hit.  A record is replaced on a
// strict comparison only: the first sample of a distance keeps it.
template <class Normal>
__host__ __device__ __forceinline__ void survey_sample(SurveyState& s, bool found, float t, float dx, float dy, float dz, Normal normal, bool flip, float D)
{
    s.n += 1u;
    const bool hit = found && t > 0.0f && t <= 3.402823466e+38f;       // a positive finite number: a NaN, 0, a negative and an infinite t are misses
    float dist = D;
    if (hit) {
        float nx, ny, nz;
        normal(nx, ny, nz);
        if (flip) { nx = -nx; ny = -ny; nz = -nz; }
        if ((dx * nx + dy * ny) + dz * nz > 0.0f) {                      // a back hit; a NaN dot is a front hit
            s.back += 1u;
            if (t < s.near_back.dist) s.near_back = SurveyRecord{ t, dx, dy, dz };
            return;
        }
        s.front += 1u;
        if (t < s.near_front.dist) s.near_front = SurveyRecord{ t, dx, dy, dz };
        dist = t < D ? t : D;
    }
    if (dist > s.far.dist) s.far = SurveyRecord{ dist, dx, dy, dz };
}

__host__ __device__ __forceinline__ bool place_record_set(const SurveyRecord& r) { return r.dist < kPlaceInf; }      // an empty near record holds +inf (a NaN counts as empty)

// The state of a surveyed probe.
__host__ __device__ __forceinline__ uint32_t place_state(const SurveyState& s, const PlaceConfig& cfg)
{
    if (s.n == 0u) return kProbeUnknown;
    if ((float)s.back / (float)s.n > cfg.back_share) return kProbeBuried;
    if (!(s.near_front.dist < cfg.max_distance)) return kProbeIdle;     // no front hit within reach: nothing there to light
    return kProbeActive;
}

// Where a surveyed probe goes: off -> out (both relative to the grid point).  spacing, counts: the grid's; an axis with one probe has spacing 0 in the bound.
// Returns the MI355RT_PLACE_* verdict.  A candidate is accepted only if every component c satisfies |c| < max_offset * spacing_a or c == 0; one that is not
// finite fails both, so an overflow or a NaN anywhere on the way refuses the candidate and the offset stays.
__host__ __device__ __forceinline__ uint32_t place_one(const SurveyState& s, const float* off, const float* spacing, const uint32_t* counts, const PlaceConfig& cfg, float* out)
{
    out[0] = off[0]; out[1] = off[1]; out[2] = off[2];
    if (s.n == 0u) return kPlaceUnsampled;
    const float share = (float)s.back / (float)s.n;
    const SurveyRecord &nb = s.near_back, &nf = s.near_front, &fr = s.far;
    float c[3];
    uint32_t branch;
    if (share > cfg.back_share && place_record_set(nb)) {               // through the nearest back face and a little beyond
        branch = kPlaceThrough;
        const float len = nb.dist + 0.5f * cfg.min_front;
        c[0] = off[0] + nb.x * len; c[1] = off[1] + nb.y * len; c[2] = off[2] + nb.z * len;
    } else if (place_record_set(nf) && nf.dist < cfg.min_front) {       // against a surface: away from it, towards the farthest free direction
        const float dot = (nf.x * fr.x + nf.y * fr.y) + nf.z * fr.z;
        const float ln = sqrtf((nf.x * nf.x + nf.y * nf.y) + nf.z * nf.z), lf = sqrtf((fr.x * fr.x + fr.y * fr.y) + fr.z * fr.z);
        if (!(dot <= (0.5f * ln) * lf)) return kPlaceStay;              // the farthest direction is within 60 degrees of the surface's: no step
        branch = kPlaceAway;
        const float m = fr.dist < cfg.min_front ? fr.dist : cfg.min_front;
        c[0] = off[0] + (fr.x * m) / lf; c[1] = off[1] + (fr.y * m) / lf; c[2] = off[2] + (fr.z * m) / lf;
    } else if (off[0] != 0.0f || off[1] != 0.0f || off[2] != 0.0f) {    // free again: back towards the grid point, as far as the nearest front face allows
        branch = kPlaceBack;
        const float lo = sqrtf((off[0] * off[0] + off[1] * off[1]) + off[2] * off[2]);
        const float room = nf.dist - cfg.min_front;
        if (place_record_set(nf) && room < lo) {
            c[0] = off[0] + ((-off[0]) * room) / lo; c[1] = off[1] + ((-off[1]) * room) / lo; c[2] = off[2] + ((-off[2]) * room) / lo;
        } else { c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f; }               // the whole way
    } else return kPlaceRest;
    for (int a = 0; a < 3; ++a) {
        const float bound = cfg.max_offset * (counts[a] == 1u ? 0.0f : spacing[a]);
        if (!(__builtin_fabsf(c[a]) < bound || c[a] == 0.0f)) return branch | kPlaceRefused;
    }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
    return branch;
}

// sh9_lookup_vis (sh9.hpp) for probes that have moved: offset(probe, a) -> f32 enters the position a corner is seen from.  Without has_off this is
// sh9_lookup_vis on every bit, with neither flag the offsets are never read and it is sh9_lookup.
template <class N, class Sh, class Usable, class Cnt, class Mom, class Off>
__host__ __device__ __forceinline__ bool sh9_lookup_placed(const ShGrid& grid, N n, Sh sh, bool has_usable, Usable usable, uint32_t R, Cnt count, Mom moment, bool has_off, Off offset,
                                                           uint32_t flags, float normal_bias, const float* p, const float* dir, bool has_nrm, const float* nrm, uint32_t mode,
                                                           float* rgb)
{
    return sh9_corners<27, true, true>(grid, n, sh, has_usable, usable, R, count, moment, has_off, offset, flags, normal_bias, p, has_nrm, nrm, dir, mode, rgb, nullptr);
}

}  // namespace mi355rt
