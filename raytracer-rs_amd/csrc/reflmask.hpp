// reflmask.hpp — per-triangle direction masks that prove reflection rays free (sixth row).
// A reflection ray (mod.rs:178-196) starts on the triangle T its parent ray hit and leaves in a direction of the hemisphere of T's normal.  The
// mask holds, per triangle and per direction bin of a cube map (face-major, B x B bins per face, the face and bin arithmetic of the lights' depth
// maps), one bit: SET = "trace the ray".  A bit is CLEAR only if every direction of the (padded) bin rises above T's plane by kReflMinCos and
// misses every other triangle from every point of T that the kernel's guard admits — then no intersector can find a hit, the ray contributes
// black (mod.rs:160-171) and is never made (kernels.hip, reflection_proves_miss).  Like the BVH's boxes and the lights' depth maps the mask
// only removes work whose outcome is known.
#pragma once
#include <cstdint>
#include <vector>

namespace mi355rt {

// The margins (derivation: DESIGN.md §3a "Margins of the reflection masks"; census: profiles/reflmask_census.txt)
constexpr double kReflMinCos = 0.05;      // a clear bin's directions rise above the triangle's plane by at least this cosine
constexpr double kReflPadAngle = 1e-3;    // angular pad (radians) around every bin and every occluder's cone
constexpr float kReflBary = 0.02f;        // the guard: the hit's barycentrics lie inside the triangle by this much (the builder shrinks T by half of it)
constexpr double kReflHeightUlps = 16.0;  // the guard: the ray's f32 origin lies above T's plane by this many ulps (2^-24) of T's longest edge, times longest edge / smallest height
constexpr uint32_t kReflBins = 16;        // bins per face edge: 1536 bits + the guard's 4 words = 208 B per triangle (8: 64 B; MI355RT_REFLECT_MASK_BINS)
constexpr uint32_t kReflGuardWords = 4;   // per triangle, behind the bits: v0.xyz (f32 bits) and the height margin

struct ReflMask {
    uint32_t bins = 0;                    // per face edge; 0: no mask (switched off, over budget, no triangles)
    uint32_t stride = 0;                  // 32-bit words per triangle: 6 * bins^2 / 32 + kReflGuardWords (a multiple of 4: records are 16-byte aligned)
    std::vector<uint32_t> words;          // ntri * stride
    double build_ms = 0.0;
    uint64_t work = 0;                    // tree nodes visited + exact cone tests
    uint64_t exact_tests = 0;             // the cone tests among them
    uint64_t clear_bits = 0;
};

inline uint32_t refl_mask_stride(uint32_t bins) { return 6u * bins * bins / 32u + kReflGuardWords; }

// tri_verts: ntri * 9 world-space floats (original triangle order: the mask is indexed by the prim of a hit record).  pad: the world-space padding of
// far occluders (the project's 2e-4 of the scene diagonal).  work_budget: past this many work units the build is abandoned and false returned (out.bins = 0).
// min_cos, pad_angle: the builder's two margins (others than the shipped ones only for the census of tests/test_reflmask.py).
bool build_reflect_mask(const float* tri_verts, uint32_t ntri, double pad, uint32_t bins, uint64_t work_budget, ReflMask& out,
                        double min_cos = kReflMinCos, double pad_angle = kReflPadAngle);

}  // namespace mi355rt
