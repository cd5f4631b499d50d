// display.hpp — the host rules of the display read-out (include/mi355rt.h): the sRGB threshold table the device searches and the
// exposure a luminance histogram gives.  IEEE double throughout; no device.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/mi355rt.h"

namespace mi355rt {

// out[k - 1] = T[k], k = 1..255: the linear value at which the sRGB code steps from k - 1 to k
inline void display_srgb_thresholds(float out[255])
{
    for (int k = 1; k <= 255; ++k) {
        const double e = ((double)k - 0.5) / 255.0;
        out[k - 1] = (float)(e <= 0.04045 ? e / 12.92 : std::pow((e + 0.055) / 1.055, 2.4));
    }
}

// key * 2^-(mean log2 luminance of the pixels ranked [floor(low N), ceil(high N)) of the N binned ones), each at its bin's centre; 1 when none is kept
inline float display_auto_exposure(const mi355rt_luminance_histogram& h, float key, float low, float high)
{
    uint64_t N = 0;
    for (uint32_t b = 0; b < MI355RT_HIST_BINS; ++b) N += h.bins[b];
    const double lo = std::floor((double)low * (double)N), hi = std::ceil((double)high * (double)N);
    uint64_t C = 0;
    double K = 0.0, acc = 0.0;
    for (uint32_t b = 0; b < MI355RT_HIST_BINS; ++b) {
        const double first = std::fmax((double)C, lo), last = std::fmin((double)(C + h.bins[b]), hi);     // N < 2^40: exact in double
        C += h.bins[b];
        if (last <= first) continue;
        const double kept = last - first, centre = ((double)b + 856.5) / 8.0 - 127.0;
        acc += kept * centre;
        K += kept;
    }
    if (K == 0.0) return 1.0f;
    return (float)((double)key * std::exp2(-(acc / K)));
}

}  // namespace mi355rt
