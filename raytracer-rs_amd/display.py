"""The display read-out (include/mi355rt.h) restated in numpy.

The library builds the luminance histogram and maps the image on the device (kernels.hip, display_hist_kernel / display_pack_kernel) and
derives the exposure on the host (csrc/display.hpp); this is the same contract, operation for operation: f32 where the device computes
(numpy does not fuse), IEEE double where the host does.  Every device output is an integer, so the two must agree exactly.  The source
image `c` is float32[npix, 3]: RayTracer.film.get_pixels(), or the rgb of RayTracer.get_denoised_pixels(); `n` is the film's counts."""
import math

import numpy as np

F = np.float32
SOURCE_FILM, SOURCE_DENOISED, SOURCE_DENOISED_SPLIT = 0, 1, 2
CURVE_REINHARD, CURVE_REINHARD_WHITE, CURVE_ACES, CURVE_CLAMP = 0, 1, 2, 3
TRANSFER_REFERENCE, TRANSFER_SRGB = 0, 1
HIST_BINS = 256
CURVES = {"reinhard": CURVE_REINHARD, "reinhard-white": CURVE_REINHARD_WHITE, "aces": CURVE_ACES, "clamp": CURVE_CLAMP}
DEFAULTS = dict(source=SOURCE_FILM, curve=CURVE_REINHARD, transfer=TRANSFER_REFERENCE, auto_exposure=0, exposure=1.0, white=4.0,
                key=0.18, low=0.0, high=1.0)                                  # mi355rt_display_default_config


def _image(c):
    c = np.asarray(c)
    assert c.dtype == np.float32, c.dtype
    return c.reshape(-1, 3)


def luminance(c):
    """L = (0.2126 r + 0.7152 g) + 0.0722 b in f32, the denoiser's own L"""
    c = _image(c)
    with np.errstate(all="ignore"):
        return ((F(0.2126) * c[:, 0] + F(0.7152) * c[:, 1]) + F(0.0722) * c[:, 2]).astype(np.float32)


def histogram(c, n):
    """dict(bins uint32[256], empty, nan, nonpositive, max_bits) of the image c with the film counts n (mi355rt_display_histogram)"""
    n = np.asarray(n).reshape(-1)
    assert n.dtype == np.uint32, n.dtype
    L = luminance(c)
    assert L.size == n.size
    empty = n == 0
    isnan = ~empty & np.isnan(L)
    with np.errstate(invalid="ignore"):
        nonpos = ~empty & ~isnan & (L <= F(0))
    binned = ~(empty | isnan | nonpos)
    bits = L[binned].view(np.uint32)
    b = np.clip((bits >> np.uint32(20)).astype(np.int64) - 856, 0, HIST_BINS - 1)
    return dict(bins=np.bincount(b, minlength=HIST_BINS).astype(np.uint32), empty=int(empty.sum()), nan=int(isnan.sum()),
                nonpositive=int(nonpos.sum()), max_bits=int(bits.max()) if bits.size else 0)


def auto_exposure(hist, key, low, high):
    """the exposure (a float32) mi355rt_display_auto_exposure derives from a histogram: IEEE double, bins in ascending order"""
    bins = [int(x) for x in np.asarray(hist["bins"] if isinstance(hist, dict) else hist).reshape(-1)]
    assert len(bins) == HIST_BINS
    key, low, high = float(F(key)), float(F(low)), float(F(high))
    if not (math.isfinite(key) and key > 0.0 and 0.0 <= low < high <= 1.0):
        raise ValueError("key > 0 finite and 0 <= low < high <= 1 are required")
    N = sum(bins)
    lo, hi = math.floor(low * float(N)), math.ceil(high * float(N))
    C, K, acc = 0, 0, 0.0
    for b, cnt in enumerate(bins):
        kept = max(0, min(C + cnt, hi) - max(C, lo))
        C += cnt
        if kept:
            acc += float(kept) * ((b + 856.5) / 8.0 - 127.0)
            K += kept
    if K == 0:
        return F(1.0)
    return F(key * float(np.exp2(np.float64(-(acc / float(K))))))


def srgb_thresholds():
    """T[1..255] as float32[255]: T[k] is the linear value at which the sRGB code steps from k - 1 to k (mi355rt_display_srgb_thresholds)"""
    out = np.zeros(255, np.float32)
    for k in range(1, 256):
        e = (k - 0.5) / 255.0
        out[k - 1] = F(e / 12.92 if e <= 0.04045 else ((e + 0.055) / 1.055) ** 2.4)
    return out


def srgb_oetf(z):
    """the sRGB encoding of linear z in float64 (what the thresholds invert)"""
    z = np.asarray(z, np.float64)
    return np.where(z <= 0.0031308, 12.92 * z, 1.055 * np.power(np.maximum(z, 0.0), 1.0 / 2.4) - 0.055)


def tone_curve(c, exposure, curve, white=DEFAULTS["white"]):
    """z float32[npix, 3]: exposure, tone curve and clamp of the display mapping (a NaN becomes 1)"""
    c = _image(c)
    E, w = F(exposure), F(white)
    with np.errstate(all="ignore"):
        x = c * E
        if curve == CURVE_REINHARD:
            y = x / (F(1) + x)
        elif curve == CURVE_REINHARD_WHITE:
            y = (x * (F(1) + x / (w * w))) / (F(1) + x)
        elif curve == CURVE_ACES:
            y = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
        elif curve == CURVE_CLAMP:
            y = x
        else:
            raise ValueError("unknown curve %r" % (curve,))
        return np.fmax(np.fmin(y.astype(np.float32), F(1)), F(0)).astype(np.float32)


def display(c, exposure=DEFAULTS["exposure"], curve=CURVE_REINHARD, transfer=TRANSFER_REFERENCE, white=DEFAULTS["white"], thresholds=None):
    """uint32[npix] 0xAARRGGBB of the image c (mi355rt_get_display_pixels with auto_exposure 0); thresholds: srgb_thresholds() or the library's"""
    z = tone_curve(c, exposure, curve, white)
    if transfer == TRANSFER_REFERENCE:
        u = (z * F(255)).astype(np.uint32) & np.uint32(0xFF)
    elif transfer == TRANSFER_SRGB:
        T = srgb_thresholds() if thresholds is None else np.asarray(thresholds, np.float32).reshape(255)
        u = np.searchsorted(T, z.reshape(-1), side="right").reshape(z.shape).astype(np.uint32)      # the number of k with T[k] <= z
    else:
        raise ValueError("unknown transfer %r" % (transfer,))
    return (u[:, 2] | (u[:, 1] << np.uint32(8)) | (u[:, 0] << np.uint32(16)) | np.uint32(0xFF000000)).astype(np.uint32)
