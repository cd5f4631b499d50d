"""The denoised read-out without a GPU: the new entry points are exported, the config struct agrees with the header, the default config is
the documented one, calls without a handle or a config are rejected, and the numpy statement of the filter (raytracer_rs_amd.denoise)
has the properties the contract in include/mi355rt.h implies, on hand-made films and guides."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_denoise_default_config", "mi355rt_get_denoised_pixels", "mi355rt_get_guides"]
F = np.float32


@pytest.fixture(scope="module")
def dn(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.denoise")


def test_denoise_symbols_are_exported(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)


def test_denoise_struct_layout_matches_the_header(pkg, tmp_path):
    src = tmp_path / "dsizes.c"
    body = "".join('printf("%%zu\\n", offsetof(mi355rt_denoise_config, %s));' % f for f, _ in pkg.DenoiseConfig._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355rt.h"\nint main(void){printf("%zu\\n", sizeof(mi355rt_denoise_config));'
                   + body + 'return 0;}\n')
    exe = tmp_path / "dsizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(pkg.DenoiseConfig)] + [getattr(pkg.DenoiseConfig, f).offset for f, _ in pkg.DenoiseConfig._fields_]
    assert got == want
    assert C.sizeof(pkg.DenoiseConfig) == 20


def test_denoise_default_config_is_the_documented_one(pkg, dn):
    c = pkg.DenoiseConfig()
    pkg.lib().mi355rt_denoise_default_config(C.byref(c))
    assert (c.iterations, c.normal_power_log2) == (5, 7)
    assert (F(c.sigma_luminance), F(c.sigma_depth), F(c.sigma_albedo)) == (F(1.0), F(0.1), F(0.1))
    assert {f: (F(getattr(c, f)) if isinstance(getattr(c, f), float) else getattr(c, f)) for f, _ in c._fields_} == \
        {k: (F(v) if isinstance(v, float) else v) for k, v in dn.DEFAULTS.items()}
    c2 = pkg.denoise_config(iterations=2)
    assert (c2.iterations, c2.normal_power_log2) == (2, 7)
    with pytest.raises(TypeError):
        pkg.denoise_config(sigma=3)


def test_denoise_calls_without_a_handle_or_config_are_rejected(pkg):
    c = pkg.denoise_config()
    rgb = np.zeros(3, np.float32); px = np.zeros(1, np.uint32)
    L = pkg.lib()
    assert L.mi355rt_get_denoised_pixels(None, C.byref(c), rgb.ctypes.data_as(C.POINTER(C.c_float)), px.ctypes.data_as(C.POINTER(C.c_uint32)), 1) == -1
    assert L.mi355rt_get_denoised_pixels(None, None, None, None, 0) == -1
    assert L.mi355rt_get_guides(None, None, None, None, None, 0) == -1
    L.mi355rt_denoise_default_config(None)          # a NULL config is ignored, not written


# ---- the numpy statement on hand-made inputs ----------------------------------------------------------------------------------------
def film(samples):
    """per-pixel lists of RGB samples -> (sum, sumsq, n) accumulated in f32 in sample order, as PixelData::add_sample does"""
    s = np.zeros((len(samples), 3), np.float32); q = np.zeros_like(s); n = np.zeros(len(samples), np.uint32)
    for i, smp in enumerate(samples):
        for c in smp:
            c = np.asarray(c, np.float32)
            s[i] = s[i] + c; q[i] = q[i] + c * c; n[i] += 1
    return s, q, n


def flat_guides(npix, normal=(0.0, 0.0, 1.0), depth=2.0, albedo=(0.5, 0.5, 0.5), prim=0):
    return dict(depth=np.full(npix, depth, np.float32), normal=np.tile(np.asarray(normal, np.float32), (npix, 1)),
                albedo=np.tile(np.asarray(albedo, np.float32), (npix, 1)), prim=np.full(npix, prim, np.uint32))


CFG = dict(normal_power_log2=7, sigma_luminance=4.0, sigma_depth=0.1, sigma_albedo=0.1)


def noisy_film(w, h, spp, seed, mean=0.4):
    rng = np.random.default_rng(seed)
    smp = (mean + 0.3 * rng.standard_normal((w * h, spp, 3))).astype(np.float32)
    return film([list(p) for p in smp])


def test_zero_iterations_is_the_identity(dn):
    w, h = 7, 5
    s, q, n = noisy_film(w, h, 3, 1)
    n[4] = 0; s[4] = 0; q[4] = 0
    rgb, packed = dn.denoise(s, q, n, flat_guides(w * h), w, h, iterations=0, **CFG)
    with np.errstate(all="ignore"):
        want = s * (F(1) / n.astype(np.float32)[:, None])
    assert np.array_equal(rgb.view(np.uint32), want.view(np.uint32))
    assert np.isnan(rgb[4]).all() and packed[4] == 0xFFFFFFFF           # empty: NaN, white once packed
    # pack() is the tone map of get_tonemapped_pixels: c/(1+c), truncated to u8
    c = np.array([[0.0, 1.0, 3.0], [np.inf, 0.25, 1e-3]], np.float32)
    assert dn.pack(c).tolist() == [0xFF007FBF, 0xFFFF3300]


def test_empty_pixels_pass_through_and_are_never_a_tap(dn):
    w, h = 9, 6
    s, q, n = noisy_film(w, h, 4, 2)
    g = flat_guides(w * h)
    rgb0, _ = dn.denoise(s, q, n, g, w, h, iterations=3, **CFG)
    # empty every pixel of column 4 and row 2: those stay NaN, and no other pixel can see them (no NaN leaks anywhere)
    e = np.zeros((h, w), bool); e[:, 4] = True; e[2, :] = True; e = e.reshape(-1)
    s2, q2, n2 = s.copy(), q.copy(), n.copy()
    s2[e] = 0; q2[e] = 0; n2[e] = 0
    rgb, packed = dn.denoise(s2, q2, n2, g, w, h, iterations=3, **CFG)
    assert np.isnan(rgb[e]).all() and (packed[e] == 0xFFFFFFFF).all()
    assert np.isfinite(rgb[~e]).all()
    # an empty pixel's own film (garbage sums with n = 0) does not matter to its neighbours either
    s3 = s2.copy(); s3[e] = 1e30
    rgb3, _ = dn.denoise(s3, q2, n2, g, w, h, iterations=3, **CFG)
    assert np.array_equal(rgb3[~e].view(np.uint32), rgb[~e].view(np.uint32))
    assert not np.array_equal(rgb0[~e].view(np.uint32), rgb[~e].view(np.uint32))


def test_a_constant_image_stays_constant(dn):
    """every pixel has the same samples: a weighted mean of equal values.  S / W with W the sum of the same weights rounds at most a
    few ulp away from the value; the bound used is 8 ulp of 0.3 after 5 iterations."""
    w, h = 23, 17
    s, q, n = film([[(0.3, 0.2, 0.7), (0.1, 0.4, 0.5), (0.2, 0.3, 0.6)]] * (w * h))
    rgb, _ = dn.denoise(s, q, n, flat_guides(w * h), w, h, iterations=5, **CFG)
    c0 = s[0] * (F(1) / F(3))
    ulp = np.spacing(np.abs(c0)).astype(np.float32)
    assert np.all(np.abs(rgb - c0) <= 8 * ulp), np.abs(rgb - c0).max(axis=0) / ulp


def test_nothing_leaks_across_a_normal_discontinuity(dn):
    """left half faces +z, right half -z: d = -1, wn = 0, so each half is filtered alone -- exactly as if the other half were empty"""
    w, h = 16, 8
    s, q, n = noisy_film(w, h, 4, 3)
    g = flat_guides(w * h)
    right = (np.arange(w * h) % w) >= w // 2
    g["normal"][right] = (0.0, 0.0, -1.0)
    s[right] += np.float32(5.0)          # the right half is much brighter: any leak would show
    rgb, _ = dn.denoise(s, q, n, g, w, h, iterations=4, **CFG)
    for half in (right, ~right):
        s2, q2, n2 = s.copy(), q.copy(), n.copy()
        s2[~half] = 0; q2[~half] = 0; n2[~half] = 0
        alone, _ = dn.denoise(s2, q2, n2, flat_guides(w * h), w, h, iterations=4, **CFG)
        assert np.array_equal(rgb[half].view(np.uint32), alone[half].view(np.uint32))
    # misses and hits do not mix either, and two misses filter together (g = 1)
    g2 = flat_guides(w * h); g2["prim"][right] = dn.MISS
    rgb2, _ = dn.denoise(s, q, n, g2, w, h, iterations=4, **CFG)
    assert np.array_equal(rgb2[~right].view(np.uint32), rgb[~right].view(np.uint32))
    assert rgb2[right].std() < (s[right] / n[right, None]).std()


def test_unknown_variance_gives_wl_1(dn):
    """with n == 1 everywhere the colour weight is 1: the filter is the plain edge-stopped a-trous blur, whatever sigma_luminance is"""
    w, h = 12, 9
    s, q, n = noisy_film(w, h, 1, 4)
    g = flat_guides(w * h)
    a, _ = dn.denoise(s, q, n, g, w, h, iterations=2, **dict(CFG, sigma_luminance=1e-3))
    b, _ = dn.denoise(s, q, n, g, w, h, iterations=2, **dict(CFG, sigma_luminance=1e3))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ... and it is the B3-spline blur of the means: one iteration by hand at an interior pixel
    c, _ = dn.film_inputs(s, q, n)
    y, x = 4, 5
    W = F(0); S = np.zeros(3, np.float32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            k = dn.K1[dx + 2] * dn.K1[dy + 2]
            S = S + k * c[(y + dy) * w + x + dx]; W = W + k
    one, _ = dn.denoise(s, q, n, g, w, h, iterations=1, **CFG)
    assert np.array_equal(one[y * w + x].view(np.uint32), (S / W).view(np.uint32))
    # with known variance, a small sigma_luminance does change the result
    s2, q2, n2 = noisy_film(w, h, 4, 4)
    a2, _ = dn.denoise(s2, q2, n2, g, w, h, iterations=2, **dict(CFG, sigma_luminance=1e-3))
    b2, _ = dn.denoise(s2, q2, n2, g, w, h, iterations=2, **dict(CFG, sigma_luminance=1e3))
    assert not np.array_equal(a2, b2)


def test_variance_of_the_mean_and_its_propagation(dn):
    s, q, n = film([[(0.0, 0.0, 0.0), (1.0, 2.0, 0.0)], [(0.5, 0.5, 0.5)], []])
    c, var = dn.film_inputs(s, q, n)
    # per channel (n q - s^2) / (n^2 (n - 1)): 0.25, 1.0, 0 -> 1.25; n == 1 and n == 0: 0
    assert var.tolist() == [1.25, 0.0, 0.0]
    assert dn.pos(np.array([np.nan, -1.0, 2.0], np.float32)).tolist() == [0.0, 0.0, 2.0]
