"""The display read-out without a GPU (include/mi355rt.h): the new entry points are exported, the structs agree with the header,
the default config is the documented one, the two host rules (the sRGB threshold table and the auto-exposure of a histogram) agree with their
numpy statements (raytracer_rs_amd.display), invalid arguments name their field, and the numpy statement has, on the golden films, the
properties that keep the GPU tests (tests/test_gpu_display.py) from being vacuous."""
import ctypes as C
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["mi355rt_display_default_config", "mi355rt_display_histogram", "mi355rt_display_auto_exposure", "mi355rt_display_srgb_thresholds",
       "mi355rt_get_display_pixels"]
F = np.float32
FIXTURES = ["4boxes", "ico2", "ico3_tex", "thai2"]


@pytest.fixture(scope="module")
def dp(pkg):
    return importlib.import_module("raytracer_rs_amd.display")


def test_display_symbols_are_exported(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)


def test_display_struct_layouts_match_the_header(pkg, tmp_path):
    structs = [("mi355rt_luminance_histogram", pkg.LuminanceHistogram), ("mi355rt_display_config", pkg.DisplayConfig)]
    body = ""
    for cname, cls in structs:
        body += 'printf("%%zu\\n", sizeof(%s));' % cname
        body += "".join('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f) for f, _ in cls._fields_)
    consts = ["MI355RT_DISPLAY_SOURCE_FILM", "MI355RT_DISPLAY_SOURCE_DENOISED", "MI355RT_DISPLAY_SOURCE_DENOISED_SPLIT", "MI355RT_CURVE_REINHARD",
              "MI355RT_CURVE_REINHARD_WHITE", "MI355RT_CURVE_ACES", "MI355RT_CURVE_CLAMP", "MI355RT_TRANSFER_REFERENCE", "MI355RT_TRANSFER_SRGB",
              "MI355RT_HIST_BINS"]
    body += "".join('printf("%%u\\n", (unsigned)%s);' % c for c in consts)
    src = tmp_path / "psizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355rt.h"\nint main(void){' + body + 'return 0;}\n')
    exe = tmp_path / "psizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = []
    for _, cls in structs:
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    want += [pkg.DISPLAY_SOURCE_FILM, pkg.DISPLAY_SOURCE_DENOISED, pkg.DISPLAY_SOURCE_DENOISED_SPLIT, pkg.CURVE_REINHARD, pkg.CURVE_REINHARD_WHITE,
             pkg.CURVE_ACES, pkg.CURVE_CLAMP, pkg.TRANSFER_REFERENCE, pkg.TRANSFER_SRGB, pkg.HIST_BINS]
    assert got == want
    assert want[-10:] == [0, 1, 2, 0, 1, 2, 3, 0, 1, 256]
    assert C.sizeof(pkg.LuminanceHistogram) == 1040 and C.sizeof(pkg.DisplayConfig) == 36


def test_display_default_config_is_the_documented_one(pkg, dp):
    c = pkg.DisplayConfig()
    pkg.lib().mi355rt_display_default_config(C.byref(c))
    assert (c.source, c.curve, c.transfer, c.auto_exposure) == (0, 0, 0, 0)
    assert (F(c.exposure), F(c.white), F(c.key), F(c.low), F(c.high)) == (F(1.0), F(4.0), F(0.18), F(0.0), F(1.0))
    assert {f: (F(getattr(c, f)) if isinstance(getattr(c, f), float) else getattr(c, f)) for f, _ in c._fields_} == \
        {k: (F(v) if isinstance(v, float) else v) for k, v in dp.DEFAULTS.items()}
    c2 = pkg.display_config(curve=pkg.CURVE_ACES, exposure=2.0)
    assert (c2.curve, F(c2.exposure), F(c2.white)) == (2, F(2.0), F(4.0))
    with pytest.raises(TypeError):
        pkg.display_config(gamma=2.2)
    pkg.lib().mi355rt_display_default_config(None)          # a NULL config is ignored, not written
    assert (dp.SOURCE_FILM, dp.SOURCE_DENOISED, dp.SOURCE_DENOISED_SPLIT) == (0, 1, 2) and dp.CURVES == {"reinhard": 0, "reinhard-white": 1, "aces": 2, "clamp": 3}


def test_display_calls_without_a_handle_are_rejected(pkg):
    c = pkg.display_config()
    px = np.zeros(1, np.uint32); hist = pkg.LuminanceHistogram()
    L = pkg.lib()
    assert L.mi355rt_get_display_pixels(None, C.byref(c), None, px.ctypes.data_as(C.POINTER(C.c_uint32)), 1, None) == -1
    assert L.mi355rt_display_histogram(None, 0, None, C.byref(hist)) == -1


# ---- the sRGB table ------------------------------------------------------------------------------------------------------------------------------
def ulp_distance(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_srgb_thresholds_equal_the_numpy_statement_and_increase(pkg, dp):
    T, want = pkg.display_srgb_thresholds(), dp.srgb_thresholds()
    assert T.dtype == np.float32 and T.shape == (255,)
    d = ulp_distance(T, want)
    print("thresholds that differ from numpy's by one ulp: %d of 255" % int((d == 1).sum()))
    assert d.max() <= 1                                                            # the double pow of two math libraries
    for t in (T, want):
        gaps = np.diff(t)
        assert (gaps > 0).all() and 0 < t[0] and t[-1] < 1
        assert gaps.min() >= 3.0e-4, gaps.min()                                      # the linear segment: 1 / (255 * 12.92) = 3.035e-4
    assert abs(float(np.diff(T).min()) - 1.0 / (255 * 12.92)) < 1e-6
    assert pkg.lib().mi355rt_display_srgb_thresholds(None) == -1
    assert b"null" in pkg.lib().mi355rt_last_error(None)


def test_srgb_search_equals_the_rounded_encoding(pkg, dp):
    """the code the table gives is round(255 * OETF(z)), the sRGB encoding rounded to nearest, wherever z is not within 1e-6 of a threshold"""
    T = pkg.display_srgb_thresholds()
    rng = np.random.default_rng(5)
    z = np.concatenate([rng.random(8000), rng.random(2000) * 0.01]).astype(np.float32)          # the dark end, where the codes are dense, twice over
    assert z.size == 10000
    near = np.abs(z.astype(np.float64)[:, None] - T.astype(np.float64)[None, :]).min(axis=1) < 1e-6
    share = float(near.mean())
    print("z within 1e-6 of a threshold (excluded): %.3f %%" % (100 * share))
    assert share < 0.01
    code = np.searchsorted(T, z, side="right")
    want = np.round(255.0 * dp.srgb_oetf(z)).astype(np.int64)
    assert np.array_equal(code[~near], want[~near])
    # ... and display() is that search: CLAMP at exposure 1 maps a grey z to (code, code, code)
    px = dp.display(np.repeat(z[:, None], 3, axis=1), 1.0, dp.CURVE_CLAMP, dp.TRANSFER_SRGB, thresholds=T)
    assert np.array_equal(px, (0xFF000000 | code | code << 8 | code << 16).astype(np.uint32))
    assert dp.display(np.array([[0.0, 1.0, np.nan], [-1.0, np.inf, T[0]]], F), 1.0, dp.CURVE_CLAMP, dp.TRANSFER_SRGB, thresholds=T).tolist() == [0xFF00FFFF, 0xFF00FF01]


# ---- auto-exposure ---------------------------------------------------------------------------------------------------------------------------------
def hist_of(bins):
    b = np.zeros(256, np.uint32)
    for k, v in bins.items():
        b[k] = v
    return dict(bins=b, empty=3, nan=1, nonpositive=2, max_bits=0x3F800000)          # the four counters do not enter the rule


def centre(b):
    return (b + 856.5) / 8.0 - 127.0


AUTO_CASES = [
    ("one bin", {100: 7}, 0.18, 0.0, 1.0),
    ("one bin, percentiles inside it", {100: 1000}, 0.18, 0.25, 0.75),
    ("two bins, cut inside both", {90: 10, 140: 30}, 0.18, 0.1, 0.9),
    ("two bins, low cuts the first away", {90: 10, 140: 30}, 0.5, 0.25, 1.0),
    ("two bins, fractional ranks", {3: 7, 250: 6}, 0.18, 0.3, 0.55),
    ("all 256 bins", {b: 1 + (b * 37) % 11 for b in range(256)}, 0.18, 0.05, 0.95),
    ("all 256 bins, everything", {b: 5 for b in range(256)}, 1.0, 0.0, 1.0),
    ("counts near 2^32", {0: 0xFFFFFFFF, 128: 0xFFFFFFFE, 255: 0xFFFFFFFF}, 0.18, 0.01, 0.99),
    ("counts near 2^32 in every bin", {b: 0xFFFFFFFF - b for b in range(256)}, 0.18, 0.4, 0.6),
    ("a thin slice", {10: 1000, 200: 1000}, 0.18, 0.4999, 0.5001),
]


@pytest.mark.parametrize("case", AUTO_CASES, ids=[c[0] for c in AUTO_CASES])
def test_auto_exposure_equals_the_numpy_statement(pkg, dp, case):
    _, bins, key, low, high = case
    h = hist_of(bins)
    got, want = pkg.display_auto_exposure(h, key, low, high), dp.auto_exposure(h, key, low, high)
    assert got.dtype == np.float32 and want.dtype == np.float32 and np.isfinite(got) and got > 0
    rel = abs(float(got) - float(want)) / float(want)
    print("%s: library %.9g, numpy %.9g, relative difference %.3g" % (case[0], got, want, rel))
    assert rel <= 2.0 ** -22                                                       # one f32 ulp of slack for exp2


def test_auto_exposure_by_hand(pkg, dp):
    """values that need no second implementation"""
    for fn in (pkg.display_auto_exposure, dp.auto_exposure):
        # every kept pixel in bin b: key * 2^-centre_b
        for b in (0, 99, 255):
            want = 0.18 * 2.0 ** -centre(b)
            assert abs(float(fn(hist_of({b: 5}), 0.18, 0.0, 1.0)) - want) <= want * 2.0 ** -22, (fn, b)
        # bin 160 starts at (160 + 856) / 8 - 127 = 0, luminance 1, and ends an eighth of an octave above: its centre is 2^(1/16)
        assert centre(160) == 0.0625
        # 10 + 30 pixels, ranks [4, 36): 6 of the first bin and 26 of the second
        want = 0.18 * 2.0 ** -((6 * centre(90) + 26 * centre(140)) / 32)
        assert abs(float(fn(hist_of({90: 10, 140: 30}), 0.18, 0.1, 0.9)) - want) <= want * 2.0 ** -22
        # three pixels, ranks [floor(1.02), ceil(1.98)) = [1, 2): one pixel kept
        want = 0.25 * 2.0 ** -centre(7)
        assert abs(float(fn(hist_of({7: 3}), 0.25, 0.34, 0.66)) - want) <= want * 2.0 ** -22
        # K == 0: exactly 1
        assert fn(hist_of({}), 0.18, 0.0, 1.0) == F(1.0)


def test_auto_exposure_with_nothing_kept_is_exactly_one(pkg, dp):
    empty = hist_of({})
    for fn in (pkg.display_auto_exposure, dp.auto_exposure):
        assert fn(empty, 0.18, 0.0, 1.0) == F(1.0)
        assert fn(empty, 7.0, 0.2, 0.3) == F(1.0)
    # the counters alone are not pixels of the rule
    assert pkg.display_auto_exposure(dict(bins=np.zeros(256, np.uint32), empty=9, nan=9, nonpositive=9, max_bits=0), 0.18, 0.0, 1.0) == F(1.0)


BAD_AUTO = [("key", (0.0, 0.0, 1.0)), ("key", (-1.0, 0.0, 1.0)), ("key", (float("nan"), 0.0, 1.0)), ("key", (float("inf"), 0.0, 1.0)),
            ("low", (0.18, -0.1, 1.0)), ("low", (0.18, float("nan"), 1.0)), ("low", (0.18, 1.0, 1.0)),
            ("high", (0.18, 0.5, 0.5)), ("high", (0.18, 0.5, 0.25)), ("high", (0.18, 0.0, 1.5)), ("high", (0.18, 0.0, float("nan")))]


@pytest.mark.parametrize("field,args", BAD_AUTO)
def test_auto_exposure_invalid_arguments_name_their_field(pkg, dp, field, args):
    h = pkg.LuminanceHistogram.from_dict(hist_of({5: 5}))
    out = C.c_float(-7.0)
    assert pkg.lib().mi355rt_display_auto_exposure(C.byref(h), *args, C.byref(out)) == -1
    assert field in pkg.lib().mi355rt_last_error(None).decode()
    assert out.value == -7.0                                                       # nothing is written
    with pytest.raises(RuntimeError, match=field):
        pkg.display_auto_exposure(hist_of({5: 5}), *args)
    with pytest.raises(ValueError):
        dp.auto_exposure(hist_of({5: 5}), *args)


def test_auto_exposure_null_arguments(pkg):
    h = pkg.LuminanceHistogram()
    out = C.c_float(0.0)
    assert pkg.lib().mi355rt_display_auto_exposure(None, 0.18, 0.0, 1.0, C.byref(out)) == -1
    assert pkg.lib().mi355rt_display_auto_exposure(C.byref(h), 0.18, 0.0, 1.0, None) == -1


# ---- the numpy statement on hand-made pixels and on the golden films -------------------------------------------------------------------------------
def test_histogram_statement_on_hand_made_pixels(dp):
    L = [2.0 ** -20, np.nextafter(F(2.0 ** -20), F(0)), 1e-40, 1.0, np.nextafter(F(1.0), F(0)), 2.0 ** 0.125 * 1.0001, 4095.9, 4096.0, 1e30, np.inf,
         0.0, -0.0, -3.0, -np.inf, np.nan, 5.0]
    c = np.repeat(np.asarray(L, F)[:, None], 3, axis=1)                             # grey: L = (0.2126 g + 0.7152 g) + 0.0722 g, about g
    n = np.ones(len(L), np.uint32); n[-1] = 0
    h = dp.histogram(c, n)
    lum = dp.luminance(c)
    assert (h["empty"], h["nan"], h["nonpositive"]) == (1, 1, 4)
    assert int(h["bins"].sum()) == 10 and h["max_bits"] == 0x7F800000
    assert h["bins"][0] >= 2 and h["bins"][255] >= 3                                # below 2^-20 and denormal; 4096, 1e30 and +inf
    # a luminance of exactly 2^e opens bin 8 (e + 20); the float below it closes the bin before
    for e in (-20, -3, 0, 5, 11):
        edge = np.array([2.0 ** e], F)
        below = np.nextafter(edge, F(0))
        assert min(255, max(0, (int(edge.view(np.uint32)[0]) >> 20) - 856)) == 8 * (e + 20)
        assert min(255, max(0, (int(below.view(np.uint32)[0]) >> 20) - 856)) == max(0, 8 * (e + 20) - 1)
    assert np.isnan(lum[-2]) and lum[3] > 0


@pytest.mark.parametrize("name", FIXTURES)
def test_statement_on_the_golden_films_is_not_vacuous(pkg, dp, name):
    g = np.load(os.path.join(GOLDEN, "render_%s.npz" % name))
    s, n = g["octree_sum"].astype(np.float32).reshape(-1, 3), g["octree_n"].astype(np.uint32).reshape(-1)
    with np.errstate(all="ignore"):
        c = (s * (F(1) / n.astype(np.float32)[:, None])).astype(np.float32)
    h = dp.histogram(c, n)
    used = int((h["bins"] > 0).sum())
    print("%s: %d bins used (%d .. %d), %d non-positive, %d empty, %d NaN" % (name, used, np.flatnonzero(h["bins"])[0], np.flatnonzero(h["bins"])[-1],
                                                                               h["nonpositive"], h["empty"], h["nan"]))
    assert used >= 40
    assert h["nonpositive"] > 0
    assert int(h["bins"].sum()) + h["empty"] + h["nan"] + h["nonpositive"] == n.size
    E = dp.auto_exposure(h, 0.18, 0.0, 1.0)
    assert np.isfinite(E) and E > 0
    assert abs(float(pkg.display_auto_exposure(h, 0.18, 0.0, 1.0)) - float(E)) <= float(E) * 2.0 ** -22
    T = pkg.display_srgb_thresholds()
    outs = {(cu, tr): dp.display(c, E, cu, tr, 4.0, T) for cu in range(4) for tr in range(2)}
    for a, b in itertools.combinations(outs, 2):
        assert not np.array_equal(outs[a], outs[b]), (a, b)
    # the default mapping is the reference's tone map
    dn = importlib.import_module("raytracer_rs_amd.denoise")
    assert np.array_equal(dp.display(c), dn.pack(c))
