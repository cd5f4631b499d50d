"""Light films without a GPU (include/mi355rt.h "LIGHT FILMS"): the flag and the entries exist and agree across the header, the Python
package and the Rust shim; calls without a handle are rejected; the numpy statement of the relit read-out (raytracer_rs_amd.relight) does what the
header writes on hand-made planes; the CLI names its options."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_light_films_get", "mi355rt_light_films_set", "mi355rt_light_films_add", "mi355rt_get_relit_pixels", "mi355rt_light_count"]
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def relight(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.relight")


@pytest.fixture(scope="module")
def dp(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.display")


def test_light_film_symbols_are_exported(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    rust = open(os.path.join(ROOT, "raytracer-rs_amd", "integration", "rust_shim", "src", "lib.rs")).read()
    mirror = open(os.path.join(ROOT, "raytracer-rs_amd", "csrc", "raytracer_lib.hpp")).read()
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)
        assert re.search(r"\b%s\(" % name, header), name
        assert re.search(r"fn %s\(" % name, rust), name
        assert name in mirror, name


def test_light_film_constants_agree(pkg):
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    rust = open(os.path.join(ROOT, "raytracer-rs_amd", "integration", "rust_shim", "src", "lib.rs")).read()
    assert re.search(r"#define\s+MI355RT_FLAG_LIGHT_FILMS\s+256u\b", header)
    assert re.search(r"#define\s+MI355RT_LIGHT_FILMS_MAX_LIGHTS\s+8u\b", header)
    assert pkg.FLAG_LIGHT_FILMS == 256 and pkg.LIGHT_FILMS_MAX_LIGHTS == 8
    assert "pub const MI355RT_FLAG_LIGHT_FILMS: u32 = 256;" in rust
    flags = [int(v) for v in re.findall(r"#define\s+MI355RT_FLAG_\w+\s+(\d+)u", header)]
    assert len(set(flags)) == len(flags) and all(v & (v - 1) == 0 for v in flags)        # one bit each, none shared


def test_light_film_calls_without_a_handle_are_rejected(pkg):
    L = pkg.lib()
    assert L.mi355rt_light_films_get(None, None, 0, 0) == -1
    assert L.mi355rt_light_films_set(None, None, 0, 0) == -1
    assert L.mi355rt_light_films_add(None, None, 0, 0) == -1
    assert L.mi355rt_get_relit_pixels(None, None, 0, None, None, None, 0, None) == -1
    assert L.mi355rt_light_count(None) == 0


def test_the_cli_names_its_options(pkg):
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    text = subprocess.check_output([exe, "--help"], text=True)
    for opt in ("--light-films", "--relight W0,W1,...", "--out-lights PREFIX"):
        assert opt in text, opt
    for args, word in ((["--relight", "1,2"], "--light-films"), (["--out-lights", "x"], "--light-films"), (["--light-films"], "--spp"),
                       (["--light-films", "--spp", "1", "--gpus", "2"], "--gpus"), (["--light-films", "--spp", "1", "--relight", "1,x"], "--relight"),
                       (["--light-films", "--spp", "1", "--relight", "1", "--denoise"], "--denoise")):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("Error:") and word in r.stderr, (args, r.stderr)


# ---- the numpy statement against a float64 evaluation on hand-made planes --------------------------------------------------------------
def reference(light, n, w3):
    """the header's formula with every f32 operation carried out exactly in float64 and rounded once: the product of two f32 values and the sum of two
    f32 values are exact in float64 up to one rounding to f32 (24 + 24 < 53 bits; a sum of two f32 rounds correctly through float64)"""
    nl, npix, _ = light.shape
    out = np.zeros((npix, 3), np.float32)
    with np.errstate(all="ignore"):
        inv = (1.0 / n.astype(np.float32).astype(np.float64)).astype(np.float32)
        for p in range(npix):
            for ch in range(3):
                c = np.float32(0.0)
                for li in range(nl):
                    m = np.float32(np.float64(light[li, p, ch]) * np.float64(inv[p]))
                    t = np.float32(np.float64(w3[li, ch]) * np.float64(m))
                    c = np.float32(np.float64(c) + np.float64(t))
                out[p, ch] = c
    return out


def same(a, b):
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


@pytest.mark.parametrize("weights", [[1.0, 1.0], [0.0, 0.0], [-2.5, 0.75], [[1.0, 0.5, 0.25], [-1.0, 0.0, 3.0]]])
def test_relit_equals_a_float64_evaluation(relight, weights):
    light = np.array([[[3.0, 0.1, 7.5], [1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [np.nan, np.inf, -np.inf], [1e-42, 0.3, 1e38], [-0.0, -4.0, 2.0]],
                      [[0.7, 9.0, 0.2], [5.0, 5.0, 5.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0], [3e38, 1e-45, 0.1], [0.0, 4.0, -2.0]]], np.float32)
    n = np.array([3, 1, 0, 7, 2, 0], np.uint32)                  # n = 0 over a zero plane and over non-zero ones, n = 1
    w3 = relight.weights3(weights, 2)
    got = relight.relit(light, n, weights)
    assert got.dtype == np.float32 and got.shape == (6, 3)
    assert same(got, reference(light, n, w3))
    assert np.isnan(got[2]).all() and np.isnan(got[5, 0])        # 0 * inf: nothing special is done for n == 0
    assert np.isnan(got[3, 0]) and not np.isnan(got[[0, 1]]).any()
    one = relight.relit(light[:1], n, np.asarray(weights, np.float32)[:1])
    assert same(one, reference(light[:1], n, w3[:1]))


def test_relit_without_lights_is_positive_zero(relight):
    c, packed, used = relight.relit_pixels(np.zeros((0, 4, 3), np.float32), np.array([0, 1, 2, 3], np.uint32), np.zeros((0, 3), np.float32))
    assert c.shape == (4, 3) and not bits(c).any()
    assert (packed == 0xFF000000).all() and used == F(1.0)
    with pytest.raises(ValueError):
        relight.relit(np.zeros((2, 4, 3), np.float32), np.ones(4, np.uint32), [1.0])


def test_one_light_at_weight_one_packs_like_the_film_mean(relight, dp):
    """display == NULL: packed is display.py's default mapping (the reference's tone map) of the film mean when the plane is the film's sum"""
    rng = np.random.default_rng(3)
    s = rng.uniform(0.0, 30.0, (64, 3)).astype(np.float32)
    s[5] = np.nan; s[6] = 0.0
    n = rng.integers(1, 9, 64).astype(np.uint32); n[7] = 0
    with np.errstate(all="ignore"):
        mean = (s * (F(1.0) / n.astype(np.float32))[:, None]).astype(np.float32)
    c, packed, used = relight.relit_pixels(s[None], n, [1.0])
    assert same(c, mean) and used == F(1.0)
    assert np.array_equal(packed, dp.display(mean))
    assert packed[5] == 0xFFFFFFFF and packed[7] == 0xFFFFFFFF     # a NaN packs to white
    # a display config: the mapping of display.py on c, the exposure from the histogram of c with n deciding `empty`
    c2, packed2, used2 = relight.relit_pixels(s[None], n, [0.5], curve=dp.CURVE_ACES, transfer=dp.TRANSFER_SRGB, auto_exposure=1, key=0.2)
    E = dp.auto_exposure(dp.histogram(c2, n), 0.2, 0.0, 1.0)
    assert used2 == E and np.array_equal(packed2, dp.display(c2, exposure=E, curve=dp.CURVE_ACES, transfer=dp.TRANSFER_SRGB))
    with pytest.raises(ValueError):
        relight.relit_pixels(s[None], n, [1.0], source=1)
