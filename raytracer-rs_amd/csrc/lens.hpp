// lens.hpp — the ray of a sample under a lens model (include/mi355rt.h, "LENS MODELS").  ONE statement of the arithmetic, compiled for the
// host (mi355rt_lens_ray) and for the device (primary_sample, guides_kernel, lens_rays_kernel): f32, unfused (every file that includes this is built with
// -ffp-contract=off), IEEE divide on both sides, expression for expression what raytracer-rs_amd/cameras.py writes in numpy.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include "device_types.hpp"

namespace mi355rt {

// The lens block of a camera: the handle's lens and what the models derive from it and the camera alone (DLens), in the expressions of cameras.py.
inline DLens lens_derive(uint32_t model, float radius, float focus, float width_world, const float* rot, float max_x, float max_y, uint32_t width, uint32_t height)
{
    DLens l{};
    l.model = model; l.radius = radius; l.focus = focus; l.width_world = width_world;
    l.mx2 = 2.0f * max_x; l.my2 = 2.0f * max_y;
    if (model == kLensOrtho) {
        l.hw = width_world * 0.5f;
        l.hh = l.hw * ((float)height / (float)width);
        l.hw2 = 2.0f * l.hw; l.hh2 = 2.0f * l.hh;
        for (int k = 0; k < 3; ++k) l.axis[k] = rot[8 + k] + rot[12 + k];
    }
    return l;
}

// rot: the 16 words of the rotation matrix; origin: orientation * (0, 0, 0, 1); flags bit 0: FIX_ROW_INDEX (PINHOLE and THIN; ORTHO always takes the true row).
// (xi1, xi2): the jitter in the pixel, (l1, l2): the lens sample; all in [0, 1).  lens: validated by whoever set it, derived by lens_derive.
// MODEL: the model when the caller knows it at compile time (the instantiations of the render kernels), else kLensAny: lens.model decides (wave-uniform).
constexpr uint32_t kLensAny = 0xFFFFFFFFu;
template <uint32_t MODEL = kLensAny>
__host__ __device__ __forceinline__ void lens_ray(const float* rot, const float* origin, float max_x, float max_y, uint32_t width, uint32_t height, uint32_t flags,
                                                  const DLens& lens, uint32_t pixel, float xi1, float xi2, float l1, float l2,
                                                  float& ox, float& oy, float& oz, float& dx, float& dy, float& dz)
{
    const uint32_t model = MODEL == kLensAny ? lens.model : MODEL;
    const uint32_t cu = pixel % width;
    if (model == kLensOrtho) {                                        // cameras.orthographic
        const uint32_t cv = pixel / width;
        const float sx = -lens.hw + lens.hw2 * (((float)cu + xi1) / (float)width);
        const float sy = -lens.hh + lens.hh2 * (((float)cv + xi2) / (float)height);
        ox = (origin[0] + sx * rot[0]) + (-sy) * rot[4];
        oy = (origin[1] + sx * rot[1]) + (-sy) * rot[5];
        oz = (origin[2] + sx * rot[2]) + (-sy) * rot[6];
        dx = lens.axis[0]; dy = lens.axis[1]; dz = lens.axis[2];
        return;
    }
    // the pinhole ray, camera.rs:80-90 as pixel_ray (kernels.hip) and cameras._pinhole_parts evaluate it
    const uint32_t cv = (flags & 1u) ? pixel / width : pixel / height;
    const float dir_x = -max_x + lens.mx2 * (((float)cu + xi1) / (float)width);
    const float dir_y = -max_y + lens.my2 * (((float)cv + xi2) / (float)height);
    const float vx = dir_x, vy = -dir_y, one = 1.0f;
    dx = vx * rot[0] + vy * rot[4] + one * rot[8] + one * rot[12];
    dy = vx * rot[1] + vy * rot[5] + one * rot[9] + one * rot[13];
    dz = vx * rot[2] + vy * rot[6] + one * rot[10] + one * rot[14];
    ox = origin[0]; oy = origin[1]; oz = origin[2];
    if (model != kLensThin) return;
    // cameras.thin_lens: a point of the square lens of half-width radius around o, through o + focus * d
    const float lx = 2.0f * l1 - 1.0f, ly = 2.0f * l2 - 1.0f;
    const float fx = lens.radius * (lx * rot[0] + ly * rot[4]);
    const float fy = lens.radius * (lx * rot[1] + ly * rot[5]);
    const float fz = lens.radius * (lx * rot[2] + ly * rot[6]);
    ox = ox + fx; oy = oy + fy; oz = oz + fz;
    dx = lens.focus * dx - fx; dy = lens.focus * dy - fy; dz = lens.focus * dz - fz;
}

}  // namespace mi355rt
