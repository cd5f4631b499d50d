"""The display read-out on the device (include/mi355rt.h) against its numpy statement (raytracer_rs_amd.display).

Every device output is an integer (histogram words, packed pixels), compared with array_equal; exposure_used is compared with the host rule:
equal to mi355rt_display_auto_exposure of the same histogram exactly (it is that code) and to the numpy statement within 2^-22 (one f32 ulp of
slack for exp2).  Hand-made films (film.set, in the manner of tests/test_film_edges.py, whose catalogue and poisoned films they start from)
cover what no render produces; rendered films cover the three sources; then identity with the existing read-outs, side effects, refusals
and the CLI."""
import ctypes as C
import functools
import importlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_film_edges import edge_film

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
F = np.float32
SHAPES = [(1, 1), (1, 9), (63, 3), (64, 4), (65, 5), (257, 3), (67, 13)]     # the tail of a 256-lane block and more than one block each way
# display_hist_kernel runs blocks of 1024 lanes, at most one per compute unit, each walking the image in steps of the grid: (129, 17) is three blocks
# with a tail, and 1000 x 307 pixels are 300 blocks' worth, more than the 256 compute units of an MI355X, so that some lanes take a second step
MORE = [(129, 17), (1000, 307)]
EXPOSURES = [1.0, 0.25, 3.5]
CURVES, TRANSFERS = range(4), range(2)
SCENE = "ico2"


@pytest.fixture(scope="module")
def dp(pkg):
    return importlib.import_module("raytracer_rs_amd.display")


@pytest.fixture(scope="module")
def table(pkg):
    return pkg.display_srgb_thresholds()


def make(pkg, scenes, name, w, h, **kw):
    return pkg.create_raytracer_from_arrays(scenes(name), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, **kw)


@pytest.fixture(scope="module")
def handles(pkg, scenes):
    made = {}

    def get(w, h, **kw):
        key = (w, h, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = make(pkg, scenes, SCENE, w, h, seed=1, **kw)
        return made[key]
    yield get
    for rt in made.values():
        rt.close()


def u32(x):
    return np.asarray(x, np.float32).view(np.uint32)


def from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def mean(s, n):
    """the film mean c = s * (1 / n) in f32 (film.rs:43-47)"""
    with np.errstate(all="ignore"):
        return (s * (F(1) / n.astype(np.float32)[:, None])).astype(np.float32)


# ---- the hand-made films ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_luminances(dp_name="raytracer_rs_amd.display"):
    """grey values g whose luminance (0.2126 g + 0.7152 g) + 0.0722 g lands exactly on a bin edge, one float below it and one above it, found by
    trying the floats around the edge; returns [(g, bits of L)], and which of the three each edge got"""
    dp = importlib.import_module(dp_name)
    out, complete = [], 0
    for b in (1, 2, 7, 8, 100, 159, 160, 161, 200, 254, 255):
        edge = np.uint32((b + 856) << 20)
        cand = from_bits(np.arange(int(edge) - 64, int(edge) + 65, dtype=np.int64).astype(np.uint32))
        L = u32(dp.luminance(np.repeat(cand[:, None], 3, axis=1)))
        got = 0
        for want in (edge - 1, edge, edge + 1):
            hit = np.flatnonzero(L == want)
            if hit.size:
                out.append((float(cand[hit[0]]), int(want)))
                got += 1
        complete += got == 3
    assert complete >= 6, complete                                     # most edges are hit from both sides and on the spot
    return out


def specials():
    """(n, (r, g, b)) pixels no render and no catalogue entry produces: bin edges, the ends of the histogram's range, single non-finite channels"""
    px = [(1, (g, g, g)) for g, _ in edge_luminances()]
    px += [(1, (1e-7, 1e-7, 1e-7)), (1, (2.0 ** -20,) * 3), (1, (1e-40, 1e-40, 1e-40)), (1, (1e-40, 0.0, 0.0)),          # below 2^-20, denormals
           (1, (5000.0, 5000.0, 5000.0)), (1, (4096.0, 4096.0, 4096.0)), (2, (1e30, 1e30, 1e30)),                        # above 2^12
           (1, (np.inf, 1.0, 1.0)), (1, (0.5, np.inf, 0.0)), (3, (np.inf, np.inf, np.inf)),                              # L = +inf
           (1, (np.nan, 1.0, 1.0)), (1, (1.0, 1.0, np.nan)), (1, (np.inf, -np.inf, 1.0)),                                # L = NaN
           (1, (-np.inf, 1.0, 1.0)), (1, (1.0, -np.inf, 1.0)), (1, (-1.0, 0.25, 0.0)), (1, (0.0, 0.0, 0.0)), (1, (-0.0, -0.0, -0.0)),   # L <= 0
           (0, (1.0, 2.0, 3.0)), (0, (np.nan, 0.0, 0.0)),                                                                # empty, whatever the sums
           (1, (0.18, 0.18, 0.18)), (4, (4.0, 2.0, 1.0)), (1, (0.999999, 1.0, 1.000001))]
    return px


@functools.lru_cache(maxsize=None)
def display_film(w, h, kind, turn=0):
    """(s float32[npix, 3], n uint32[npix]): the poisoned or finite catalogue film of tests/test_film_edges.py with the specials above put
    over it at seeded pixels (an image too small for all of them takes a window of the list that starts at `turn`); kind "flat": every pixel
    the same, all in one bin"""
    npix = w * h
    if kind == "flat":
        return np.tile(np.asarray([[2.0, 3.0, 1.0]], F), (npix, 1)), np.full(npix, 4, np.uint32)
    f = edge_film(w, h, kind, False)
    s, n = f["sum"].copy(), f["n"].copy()
    sp = specials()
    sp = sp[turn % len(sp):] + sp[:turn % len(sp)]
    rng = np.random.default_rng([7, w, h])
    where = rng.permutation(npix)[:len(sp)] if npix > 2 * len(sp) else np.arange(min(npix, len(sp)))
    for p, (cnt, rgb) in zip(where.tolist(), sp):
        n[p] = cnt
        s[p] = np.asarray(rgb, F) * F(max(cnt, 1))                      # n = 1: the mean is the value itself; n = 2, 3, 4: exact products
    for a in (s, n):
        a.setflags(write=False)
    return s, n


def put(rt, s, n):
    rt.film.set(s, np.zeros_like(s), n)


def assert_hist(got, want, what=""):
    assert np.array_equal(got["bins"], want["bins"]), (what, np.flatnonzero(got["bins"] != want["bins"])[:8].tolist())
    for k in ("empty", "nan", "nonpositive", "max_bits"):
        assert got[k] == want[k], (what, k, got[k], want[k])


def assert_pixels(got, want, what=""):
    assert got.dtype == np.uint32 and np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8].tolist(),
                                                                  [hex(x) for x in got[got != want][:4]], [hex(x) for x in want[got != want][:4]])


def check_source(pkg, dp, table, rt, c, n, source=0, exposures=EXPOSURES, curves=CURVES, transfers=TRANSFERS, what=""):
    """histogram, packed pixels of every curve x transfer x exposure, and the auto exposure, of one source image against display.py"""
    want_hist = dp.histogram(c, n)
    hist = rt.display_histogram(source)
    assert_hist(hist, want_hist, what)
    for E in exposures:
        for cu in curves:
            for tr in transfers:
                got, used = rt.get_display_pixels(source=source, curve=cu, transfer=tr, exposure=E, white=2.5)
                assert used == F(E)
                assert_pixels(got, dp.display(c, E, cu, tr, 2.5, table), "%s source %d curve %d transfer %d exposure %g" % (what, source, cu, tr, E))
    for key, low, high in ((0.18, 0.0, 1.0), (0.5, 0.1, 0.9)):
        want_E = dp.auto_exposure(want_hist, key, low, high)
        got, used = rt.get_display_pixels(source=source, curve=pkg.CURVE_ACES, transfer=pkg.TRANSFER_SRGB, auto_exposure=1, exposure=-1.0,
                                          key=key, low=low, high=high)
        assert used == pkg.display_auto_exposure(hist, key, low, high)
        assert abs(float(used) - float(want_E)) <= float(want_E) * 2.0 ** -22, (what, used, want_E)
        again, used2 = rt.get_display_pixels(source=source, curve=pkg.CURVE_ACES, transfer=pkg.TRANSFER_SRGB, exposure=float(used))
        assert used2 == used
        assert_pixels(got, again, what + " auto-exposure on against off")
        assert_pixels(got, dp.display(c, used, dp.CURVE_ACES, dp.TRANSFER_SRGB, 4.0, table), what + " auto-exposure")
    return want_hist


# ---- 1. hand-made films ------------------------------------------------------------------------------------------------------------------------------
def test_the_hand_made_films_hold_what_they_should(pkg, dp):
    """of the builder and the numpy statement, never of the library: what keeps the comparisons below from being vacuous"""
    s, n = display_film(67, 13, "nonfinite")
    h = dp.histogram(mean(s, n), n)
    assert h["empty"] >= 2 and h["nan"] >= 3 and h["nonpositive"] >= 5 and h["max_bits"] == 0x7F800000
    assert h["bins"][0] >= 3 and h["bins"][255] >= 5 and (h["bins"] > 0).sum() >= 12
    lum = u32(dp.luminance(mean(s, n)))
    for _, want in edge_luminances():
        assert (lum[n == 1] == want).any(), hex(want)                   # on the edge, one below, one above
    edges = {want for _, want in edge_luminances()}
    assert sum(1 for e in edges if e & 0xFFFFF == 0) >= 6 and sum(1 for e in edges if e & 0xFFFFF == 0xFFFFF) >= 6
    fs, fn = display_film(67, 13, "flat")
    fh = dp.histogram(mean(fs, fn), fn)
    assert (fh["bins"] > 0).sum() == 1 and fh["bins"].sum() == 67 * 13
    one = display_film(1, 1, "finite", 3)
    assert one[1].size == 1


@pytest.mark.parametrize("kind", ["finite", "nonfinite", "flat"])
@pytest.mark.parametrize("shape", SHAPES + MORE[:1])
def test_hand_made_films_equal_the_numpy_statement(pkg, dp, table, handles, shape, kind):
    w, h = shape
    rt = handles(w, h)
    for turn in ((0,) if w * h > 100 or kind == "flat" else range(0, len(specials()), max(1, w * h))):
        s, n = display_film(w, h, kind, turn)
        put(rt, s, n)
        c = mean(s, n)
        check_source(pkg, dp, table, rt, c, n, what="%dx%d %s turn %d" % (w, h, kind, turn),
                     exposures=EXPOSURES if turn == 0 or w * h > 1 else EXPOSURES[:1])
        assert np.array_equal(rt.get_display_pixels()[0], rt.get_tonemapped_pixels())       # the default config
        sb, _, nb = rt.film.pixel_datas()
        assert np.array_equal(u32(sb), u32(s)) and np.array_equal(nb, n)                   # only read


@pytest.mark.parametrize("kind", ["nonfinite", "flat"])
def test_an_image_of_more_than_one_step_per_lane(pkg, dp, table, handles, kind):
    w, h = MORE[1]
    rt = handles(w, h)
    s, n = display_film(w, h, kind)
    put(rt, s, n)
    c = mean(s, n)
    check_source(pkg, dp, table, rt, c, n, exposures=[3.5], curves=[pkg.CURVE_REINHARD_WHITE, pkg.CURVE_CLAMP], what="%dx%d %s" % (w, h, kind))


def test_threshold_film(pkg, dp, table, handles):
    """n = 1, CLAMP, exposure 1: channel values T[k], the float below and the float above, for every k (exact as film means: s * (1 / 1) = s);
    the sRGB codes must be k, k - 1, k"""
    w, h = 51, 5
    assert w * h == 255
    rt = handles(w, h)
    T = table
    s = np.stack([T, np.nextafter(T, F(-1)), np.nextafter(T, F(2))], axis=1).astype(np.float32)
    n = np.ones(255, np.uint32)
    put(rt, s, n)
    got, used = rt.get_display_pixels(curve=pkg.CURVE_CLAMP, transfer=pkg.TRANSFER_SRGB)
    k = np.arange(1, 256, dtype=np.uint32)
    want = (np.uint32(0xFF000000) | k << np.uint32(16) | (k - np.uint32(1)) << np.uint32(8) | k).astype(np.uint32)
    assert used == F(1)
    assert_pixels(got, want, "threshold film")
    assert_pixels(got, dp.display(s, 1.0, dp.CURVE_CLAMP, dp.TRANSFER_SRGB, 4.0, T), "threshold film against display.py")
    # the reference transfer on the same film truncates z * 255
    got, _ = rt.get_display_pixels(curve=pkg.CURVE_CLAMP)
    assert_pixels(got, dp.display(s, 1.0, dp.CURVE_CLAMP, dp.TRANSFER_REFERENCE), "threshold film, reference transfer")


# ---- 2. rendered films: the three sources, identity with the existing read-outs --------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("name", ["thai2", "ico3_tex"])
def test_rendered_films_equal_the_numpy_statement(pkg, scenes, dp, table, sem, name, direct):
    w, h = 64, 48
    rt = make(pkg, scenes, name, w, h, seed=21, flags=sem.gpu | (pkg.FLAG_DIRECT_FILM if direct else 0))
    rt.render(8)
    _, _, n = rt.film.pixel_datas()
    ldr = rt.get_tonemapped_pixels().copy()
    assert_pixels(rt.get_display_pixels()[0], ldr, "default config against get_tonemapped_pixels")
    images = {pkg.DISPLAY_SOURCE_FILM: (rt.film.get_pixels(), ldr)}
    images[pkg.DISPLAY_SOURCE_DENOISED] = rt.get_denoised_pixels()
    if direct:
        images[pkg.DISPLAY_SOURCE_DENOISED_SPLIT] = rt.get_denoised_pixels(split=True)
    hists = {}
    for source, (rgb, packed) in images.items():
        assert_pixels(rt.get_display_pixels(source=source)[0], packed, "source %d with default fields against the read-out's packed" % source)
        hists[source] = check_source(pkg, dp, table, rt, rgb, n, source=source, exposures=[0.7], what="%s source %d" % (name, source))
        assert (hists[source]["bins"] > 0).sum() >= 10 and hists[source]["empty"] == 0
    assert not np.array_equal(hists[0]["bins"], hists[1]["bins"])                            # the sources are different images
    # a denoise config of the caller's reaches the filter
    rgb2, _ = rt.get_denoised_pixels(iterations=2, sigma_luminance=0.5)
    got, _ = rt.get_display_pixels(source=1, curve=pkg.CURVE_ACES, transfer=pkg.TRANSFER_SRGB, exposure=2.0, denoise=dict(iterations=2, sigma_luminance=0.5))
    assert_pixels(got, dp.display(rgb2, 2.0, dp.CURVE_ACES, dp.TRANSFER_SRGB, 4.0, table), "source 1 with a denoise config")
    assert_hist(rt.display_histogram(1, iterations=2, sigma_luminance=0.5), dp.histogram(rgb2, n), "histogram with a denoise config")
    assert_hist(rt.display_histogram(1, iterations=0), hists[0], "no iteration: the film means")
    rt.close()


# ---- 3. it only reads ---------------------------------------------------------------------------------------------------------------------------------
def test_display_only_reads(pkg, scenes):
    w, h = 64, 160
    rt = make(pkg, scenes, "thai2", w, h, seed=9, flags=pkg.FLAG_DIRECT_FILM)
    rt.render(4)
    rt.trace_frame_additive()                                                               # the row cursor stands at 50
    film0 = [np.asarray(x).copy() for x in rt.film.pixel_datas()] + [rt.film.direct_sums()]
    counts0 = rt.last_counts().as_dict()
    row0 = rt.current_row
    ldr0 = rt.get_tonemapped_pixels().copy()
    for source in (0, 1, 2):                                                                # the first calls allocate
        rt.display_histogram(source)
        rt.get_display_pixels(source=source, transfer=pkg.TRANSFER_SRGB)
    hbm = rt.hbm_allocated_bytes()
    for source in (0, 1, 2):
        rt.display_histogram(source)
        for auto in (0, 1):
            for tr in TRANSFERS:
                rt.get_display_pixels(source=source, transfer=tr, curve=pkg.CURVE_ACES, auto_exposure=auto)
    assert rt.hbm_allocated_bytes() == hbm
    for x, y in zip(film0, list(rt.film.pixel_datas()) + [rt.film.direct_sums()]):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    assert rt.last_counts().as_dict() == counts0 and rt.current_row == row0
    assert np.array_equal(ldr0, rt.get_tonemapped_pixels())
    # the changed-row tracking of the tone-mapper: rows rendered after its last read-out are still mapped again after a display read-out
    rt.render(1)
    rt.get_display_pixels(auto_exposure=1)
    want = rt.get_display_pixels()[0]
    assert np.array_equal(rt.get_tonemapped_pixels(), want) and not np.array_equal(want, ldr0)
    rt.close()


def test_memory_is_allocated_on_first_use_and_counted(pkg, scenes):
    w, h = 100, 37
    rt = make(pkg, scenes, "ico2", w, h, seed=11)
    rt.render(2)
    rt.get_tonemapped_pixels()
    hbm0 = rt.hbm_allocated_bytes()
    rt.display_histogram()
    assert rt.hbm_allocated_bytes() - hbm0 == 1040                                          # the histogram's words
    rt.get_display_pixels()
    assert rt.hbm_allocated_bytes() - hbm0 == 1040 + 1024 + 4 * w * h                       # + the table and the packed image
    rt.get_display_pixels(transfer=pkg.TRANSFER_SRGB, auto_exposure=1)
    assert rt.hbm_allocated_bytes() - hbm0 == 1040 + 1024 + 4 * w * h
    rt.get_display_pixels(source=1)
    assert rt.hbm_allocated_bytes() - hbm0 == 1040 + 1024 + (4 + 32 + 52) * w * h           # + the denoiser's guides and buffers, shared with it
    rt.get_denoised_pixels()
    assert rt.hbm_allocated_bytes() - hbm0 == 1040 + 1024 + (4 + 32 + 52) * w * h
    rt.close()


@pytest.mark.parametrize("readout", ["histogram", "pixels", "auto"])
def test_drop_in_speculation_is_settled(pkg, scenes, oracle, readout):
    """as tests/test_gpu_denoise.py shows it for the denoiser: a speculative 50-row frame is out when the read-out comes; the read-out sees the film
    without it, and the drop-in loop goes on as if nothing had happened"""
    name, w, h = "thai2", 64, 160
    rt = make(pkg, scenes, name, w, h, seed=10)
    orc = oracle.Oracle(scenes(name), w, h, seed=10)
    rt.trace_frame_additive()
    launched0, _ = rt.debug_speculation()
    orc.trace_frame_additive()
    if readout == "histogram":
        dp = importlib.import_module("raytracer_rs_amd.display")
        s, _, n = orc.film()
        assert_hist(rt.display_histogram(), dp.histogram(mean(s, n), n), "the film without the speculative frame")
    else:
        got, used = rt.get_display_pixels(auto_exposure=1 if readout == "auto" else 0)
        if readout == "pixels":
            assert_pixels(got, orc.get_tonemapped_pixels(), "the film without the speculative frame")
        else:
            dp = importlib.import_module("raytracer_rs_amd.display")
            s, _, n = orc.film()
            assert_pixels(got, dp.display(mean(s, n), used), "the film without the speculative frame, auto-exposed")
    rt.trace_frame_additive()
    orc.trace_frame_additive()
    assert launched0 >= 1                                             # a speculative frame was out when the read-out came
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(u32(gs), u32(os_)) and np.array_equal(u32(gq), u32(oq))
    assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())
    orc.close()
    rt.close()


def test_a_queued_frame_is_settled(pkg, scenes):
    w, h = 64, 48
    a, b = make(pkg, scenes, "ico2", w, h, seed=5), make(pkg, scenes, "ico2", w, h, seed=5)
    a.render(3)
    b.render(3, wait=False)
    assert_hist(b.display_histogram(), a.display_histogram(), "behind render_async")
    b.render(2, wait=False); a.render(2)
    for kw in (dict(), dict(auto_exposure=1, transfer=pkg.TRANSFER_SRGB)):
        got, used = b.get_display_pixels(**kw)
        want, used_a = a.get_display_pixels(**kw)
        assert_pixels(got, want, "behind render_async")
        assert used == used_a
        b.render(1, wait=False); a.render(1)
    a.close(); b.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------------------
PATTERN = 0x12345678


def raw_pixels(pkg, rt, cfg, dn, packed, npix, used=None):
    return pkg.lib().mi355rt_get_display_pixels(rt._h, None if cfg is None else C.byref(cfg), None if dn is None else C.byref(dn),
                                                None if packed is None else packed.ctypes.data_as(C.POINTER(C.c_uint32)), npix,
                                                None if used is None else C.byref(used))


def last_error(pkg, rt):
    return pkg.lib().mi355rt_last_error(rt._h).decode()


BAD_FIELDS = [("source", dict(source=3)), ("curve", dict(curve=4)), ("transfer", dict(transfer=2)), ("auto_exposure", dict(auto_exposure=2)),
              ("exposure", dict(exposure=0.0)), ("exposure", dict(exposure=-1.0)), ("exposure", dict(exposure=float("nan"))), ("exposure", dict(exposure=float("inf"))),
              ("white", dict(white=0.0)), ("white", dict(white=float("nan"))), ("white", dict(white=float("inf")), ), ("white", dict(curve=3, white=-2.0)),
              ("key", dict(key=0.0)), ("key", dict(key=float("nan"))), ("key", dict(auto_exposure=1, key=float("inf"))),
              ("low", dict(low=-0.1)), ("low", dict(low=1.0)), ("low", dict(low=float("nan"))),
              ("high", dict(high=0.0)), ("high", dict(low=0.5, high=0.5)), ("high", dict(high=1.5)), ("high", dict(high=float("nan")))]
BAD_DENOISE = [("iterations", dict(iterations=11)), ("normal_power_log2", dict(normal_power_log2=11)), ("sigma_luminance", dict(sigma_luminance=0.0)),
               ("sigma_depth", dict(sigma_depth=float("nan"))), ("sigma_albedo", dict(sigma_albedo=-1.0))]


def test_invalid_calls_are_rejected_and_write_nothing(pkg, scenes):
    w, h = 32, 24
    rt = make(pkg, scenes, "ico2", w, h, seed=12)
    rt.render(2)
    npix = w * h
    packed = np.full(npix + 1, PATTERN, np.uint32)
    used = C.c_float(-7.0)
    for field, kw in BAD_FIELDS:
        assert raw_pixels(pkg, rt, pkg.display_config(**kw), None, packed, npix, used) == -1, kw
        assert field in last_error(pkg, rt), (kw, last_error(pkg, rt))
        with pytest.raises(RuntimeError, match=field):
            rt.get_display_pixels(**kw)
    for field, kw in BAD_DENOISE:
        assert raw_pixels(pkg, rt, pkg.display_config(source=1), pkg.denoise_config(**kw), packed, npix, used) == -1, kw
        assert field in last_error(pkg, rt)
        hist = pkg.LuminanceHistogram(); hist.empty = 77
        assert pkg.lib().mi355rt_display_histogram(rt._h, 1, C.byref(pkg.denoise_config(**kw)), C.byref(hist)) == -1
        assert field in last_error(pkg, rt) and hist.empty == 77
        assert raw_pixels(pkg, rt, pkg.display_config(), pkg.denoise_config(**kw), packed, npix) == 0          # ignored for the film
        packed[:] = PATTERN
    for bad_npix in (npix - 1, npix + 1, 0):
        assert raw_pixels(pkg, rt, pkg.display_config(), None, packed, bad_npix, used) == -1
        assert "npix" in last_error(pkg, rt)
    assert raw_pixels(pkg, rt, None, None, packed, npix, used) == -1 and "null config" in last_error(pkg, rt)
    assert raw_pixels(pkg, rt, pkg.display_config(), None, None, npix, used) == -1 and "packed" in last_error(pkg, rt)
    # the split source on a handle without the flag
    assert raw_pixels(pkg, rt, pkg.display_config(source=2), None, packed, npix, used) == -1
    assert "MI355RT_FLAG_DIRECT_FILM" in last_error(pkg, rt)
    hist = pkg.LuminanceHistogram(); hist.nan = 77
    assert pkg.lib().mi355rt_display_histogram(rt._h, 2, None, C.byref(hist)) == -1 and "MI355RT_FLAG_DIRECT_FILM" in last_error(pkg, rt)
    assert pkg.lib().mi355rt_display_histogram(rt._h, 3, None, C.byref(hist)) == -1 and "source" in last_error(pkg, rt)
    assert pkg.lib().mi355rt_display_histogram(rt._h, 0, None, None) == -1
    assert hist.nan == 77 and not any(hist.bins)
    assert (packed == PATTERN).all() and used.value == -7.0
    # exposure is not read with auto_exposure, and not validated
    assert raw_pixels(pkg, rt, pkg.display_config(auto_exposure=1, exposure=float("nan")), None, packed, npix, used) == 0
    assert used.value > 0 and packed[npix] == PATTERN and (packed[:npix] != PATTERN).all()
    rt.close()


@pytest.mark.parametrize("kind", ["device_group", "striped"])
def test_groups_and_stripes_are_rejected(pkg, scenes, kind):
    w, h = 32, 24
    kw = dict(device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE | pkg.FLAG_DIRECT_FILM) if kind == "device_group" else \
        dict(stripe_rows=4, stripe_rank=0, stripe_world=2, flags=pkg.FLAG_DIRECT_FILM)
    rt = make(pkg, scenes, "ico2", w, h, seed=13, **kw)
    rt.render(2)
    npix = w * h
    msg = "device group" if kind == "device_group" else "striped"
    packed = np.full(npix, PATTERN, np.uint32)
    for source in (0, 1, 2):
        assert raw_pixels(pkg, rt, pkg.display_config(source=source), None, packed, npix) == -1
        assert msg in last_error(pkg, rt)
        hist = pkg.LuminanceHistogram(); hist.max_bits = 77
        assert pkg.lib().mi355rt_display_histogram(rt._h, source, None, C.byref(hist)) == -1
        assert msg in last_error(pkg, rt) and hist.max_bits == 77
        with pytest.raises(RuntimeError, match=msg):
            rt.get_display_pixels(source=source)
        with pytest.raises(RuntimeError, match=msg):
            rt.display_histogram(source)
    assert (packed == PATTERN).all()
    rt.close()


# ---- 5. the CLI ---------------------------------------------------------------------------------------------------------------------------------------
def read_png(path):
    """(width, height, uint8[npix, 3]) of an 8-bit RGB PNG whose scanlines all use filter 0 (what the CLI writes)"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        ln, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + ln]
        if kind == b"IHDR":
            size = struct.unpack(">II", body[:8]); assert body[8:] == bytes([8, 2, 0, 0, 0])
        elif kind == b"IDAT":
            idat += body
        pos += 12 + ln
    w, h = size
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return w, h, raw[:, 1:].reshape(-1, 3)


def rgb_of(px):
    return np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8)


def test_cli_display_options(pkg, scenes, tmp_path):
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    w, h = 64, 48
    base = [exe, "-f", os.path.join(SCENES, "4boxes.scene"), "--width", str(w), "--height", str(h), "--seed", "17", "--spp", "4"]
    out = tmp_path / "x.png"
    r = subprocess.run(base + ["--srgb", "--curve", "aces", "--exposure", "2", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "display: exposure 2\n" in r.stdout
    rt = make(pkg, scenes, "4boxes", w, h, seed=17)
    rt.render(4)
    want, _ = rt.get_display_pixels(transfer=pkg.TRANSFER_SRGB, curve=pkg.CURVE_ACES, exposure=2.0)
    assert read_png(out)[:2] == (w, h) and np.array_equal(read_png(out)[2], rgb_of(want))
    plain = tmp_path / "y.png"
    r = subprocess.run(base + ["--out", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "display:" not in r.stdout
    today = rt.get_tonemapped_pixels()
    assert np.array_equal(read_png(plain)[2], rgb_of(today)) and not np.array_equal(today, want)
    # the source follows --denoise, the exposure is printed, and the two exposure options exclude each other
    auto = tmp_path / "z.png"
    r = subprocess.run(base + ["--denoise", "--auto-exposure", "--key", "0.25", "--out", str(auto)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want, used = rt.get_display_pixels(source=1, auto_exposure=1, key=0.25)
    assert ("display: exposure %.9g (auto)\n" % used) in r.stdout
    assert np.array_equal(read_png(auto)[2], rgb_of(want))
    r = subprocess.run(base + ["--exposure", "2", "--auto-exposure", "--out", str(auto)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "exclude" in r.stderr
    rt.close()
