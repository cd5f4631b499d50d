"""The direct film and the split denoised read-out without a GPU (include/mi355rt.h): the header declares, the library
exports, and the ctypes mirror, the C++ mirror and the Rust shim list the two entry points and the flag value 128; calls without a handle
are rejected; the numpy statement of the split filter (raytracer_rs_amd.denoise.denoise_split) has the properties the contract implies,
on hand-made films and guides."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_film_get_direct", "mi355rt_get_denoised_pixels_split"]
F = np.float32


@pytest.fixture(scope="module")
def dn(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.denoise")


def test_direct_film_symbols_and_flag_are_declared_everywhere(pkg):
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    header_nc = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"#define\s+MI355RT_FLAG_DIRECT_FILM\s+128u\b", header_nc)
    assert pkg.FLAG_DIRECT_FILM == 128
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    rust = open(os.path.join(ROOT, "raytracer-rs_amd", "integration", "rust_shim", "src", "lib.rs")).read()
    cpp = open(os.path.join(ROOT, "raytracer-rs_amd", "csrc", "raytracer_lib.hpp")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header_nc), name
        assert " T %s\n" % name in exported, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)
        assert re.search(r"fn\s+%s\s*\(" % name, rust), name
        assert name + "(" in cpp, name
    assert re.search(r"MI355RT_FLAG_DIRECT_FILM\s*:\s*u32\s*=\s*128\s*;", rust)
    # the shim's denoise config lists the header's fields in the header's order
    m = re.search(r"struct\s+mi355rt_denoise_config\s*\{(.*?)\}", rust, re.S)
    fields = [f.split(":")[0].replace("pub", "").strip() for f in m.group(1).split(",") if ":" in f]
    assert fields == [f for f, _ in pkg.DenoiseConfig._fields_]
    proto = {n: (r, a) for n, r, a in pkg.ABI}
    assert proto["mi355rt_get_denoised_pixels_split"] == proto["mi355rt_get_denoised_pixels"]
    assert proto["mi355rt_film_get_direct"][0] is C.c_int and len(proto["mi355rt_film_get_direct"][1]) == 2


def test_direct_film_calls_without_a_handle_are_rejected(pkg):
    L = pkg.lib()
    c = pkg.denoise_config()
    d = np.full(3, 7.0, np.float32); px = np.full(1, 5, np.uint32)
    assert L.mi355rt_film_get_direct(None, d.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert L.mi355rt_film_get_direct(None, None) == -1
    assert L.mi355rt_get_denoised_pixels_split(None, C.byref(c), d.ctypes.data_as(C.POINTER(C.c_float)), px.ctypes.data_as(C.POINTER(C.c_uint32)), 1) == -1
    assert L.mi355rt_get_denoised_pixels_split(None, None, None, None, 0) == -1
    assert (d == 7.0).all() and px[0] == 5


# ---- the numpy statement on hand-made inputs ----------------------------------------------------------------------------------------
def film(samples):
    """per-pixel lists of (total, direct) RGB samples -> (sum, sumsq, n, direct) accumulated in f32 in sample order"""
    s = np.zeros((len(samples), 3), np.float32); q = np.zeros_like(s); d = np.zeros_like(s); n = np.zeros(len(samples), np.uint32)
    for i, smp in enumerate(samples):
        for c, l0 in smp:
            c = np.asarray(c, np.float32)
            s[i] = s[i] + c; q[i] = q[i] + c * c; n[i] += 1
            d[i] = d[i] + np.asarray(l0, np.float32)
    return s, q, n, d


def flat_guides(npix):
    return dict(depth=np.full(npix, 2.0, np.float32), normal=np.tile(np.asarray((0.0, 0.0, 1.0), np.float32), (npix, 1)),
                albedo=np.tile(np.asarray((0.5, 0.5, 0.5), np.float32), (npix, 1)), prim=np.zeros(npix, np.uint32))


CFG = dict(normal_power_log2=7, sigma_luminance=1.0, sigma_depth=0.1, sigma_albedo=0.1)


def noisy_film(w, h, spp, seed):
    """a noiseless direct part that varies from pixel to pixel (an edge down the middle) under a noisy indirect part"""
    rng = np.random.default_rng(seed)
    direct = np.where((np.arange(w * h) % w < w // 2)[:, None], F(0.8), F(0.1)).astype(np.float32) * np.ones(3, np.float32)
    ind = np.abs(0.2 + 0.2 * rng.standard_normal((w * h, spp, 3))).astype(np.float32)
    return film([[(direct[p] + ind[p, k], direct[p]) for k in range(spp)] for p in range(w * h)])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("iterations", [0, 1, 3, 5])
def test_no_direct_light_is_the_plain_filter(dn, iterations):
    w, h = 11, 7
    s, q, n, d = noisy_film(w, h, 4, 1)
    n[5] = 0; s[5] = 0; q[5] = 0; n[9] = 1
    g = flat_guides(w * h)
    rgb, packed = dn.denoise_split(s, q, n, np.zeros_like(d), g, w, h, iterations=iterations, **CFG)
    want, want_packed = dn.denoise(s, q, n, g, w, h, iterations=iterations, **CFG)
    ok = n != 0
    assert np.array_equal(rgb[ok], want[ok]) and np.isnan(rgb[~ok]).all() and np.isnan(want[~ok]).all()
    assert np.array_equal(packed, want_packed)


@pytest.mark.parametrize("iterations", [1, 2, 5, 8])
def test_all_direct_light_comes_back_exactly(dn, iterations):
    """d == s: the indirect part is exactly zero, the filter of zeros is zero, and the read-out is s * (1 / n) to the bit"""
    w, h = 11, 7
    s, q, n, _ = noisy_film(w, h, 3, 2)
    rgb, packed = dn.denoise_split(s, q, n, s.copy(), flat_guides(w * h), w, h, iterations=iterations, **CFG)
    want = s * (F(1) / n.astype(np.float32)[:, None])
    assert np.array_equal(bits(rgb), bits(want))
    assert np.array_equal(packed, dn.pack(want))


def test_empty_pixels_come_back_nan_and_are_never_a_tap(dn):
    w, h = 9, 6
    s, q, n, d = noisy_film(w, h, 4, 3)
    g = flat_guides(w * h)
    e = np.zeros((h, w), bool); e[:, 4] = True; e[2, :] = True; e = e.reshape(-1)
    s[e] = 0; q[e] = 0; n[e] = 0
    rgb, packed = dn.denoise_split(s, q, n, d, g, w, h, iterations=3, **CFG)
    assert np.isnan(rgb[e]).all() and (packed[e] == 0xFFFFFFFF).all()      # NaN packs to white
    assert np.isfinite(rgb[~e]).all()
    # whatever an empty pixel's sums hold does not reach its neighbours
    d2 = d.copy(); d2[e] = 1e30; s2 = s.copy(); s2[e] = -1e30
    rgb2, _ = dn.denoise_split(s2, q, n, d2, g, w, h, iterations=3, **CFG)
    assert np.array_equal(bits(rgb2[~e]), bits(rgb[~e]))


def test_zero_iterations_ignores_the_direct_film(dn):
    w, h = 7, 5
    s, q, n, d = noisy_film(w, h, 3, 4)
    n[4] = 0; s[4] = 0; q[4] = 0
    g = flat_guides(w * h)
    a, pa = dn.denoise_split(s, q, n, d, g, w, h, iterations=0, **CFG)
    b, pb = dn.denoise_split(s, q, n, np.full_like(d, 123.0), g, w, h, iterations=0, **CFG)
    with np.errstate(all="ignore"):
        want = s * (F(1) / n.astype(np.float32)[:, None])
    assert np.array_equal(bits(a), bits(want)) and np.array_equal(bits(b), bits(want))       # not cd + (c - cd)
    assert np.array_equal(pa, pb) and np.array_equal(pa, dn.pack(want))


def test_the_direct_part_is_not_filtered(dn):
    """a sharp edge in the direct light under indirect noise: the plain filter smears the edge (the guides are flat), the split one keeps
    the direct step to within the filtered indirect part"""
    w, h = 16, 8
    s, q, n, d = noisy_film(w, h, 4, 5)
    g = flat_guides(w * h)
    cfg = dict(CFG, sigma_luminance=1e3)                 # the colour weight cannot stop at the edge
    plain, _ = dn.denoise(s, q, n, g, w, h, iterations=4, **cfg)
    split, _ = dn.denoise_split(s, q, n, d, g, w, h, iterations=4, **cfg)
    x = np.arange(w * h) % w

    def step(im):
        return float(im[x == w // 2 - 1].mean() - im[x == w // 2].mean())
    assert abs(step(split) - 0.7) < 0.1 and step(plain) < 0.35
