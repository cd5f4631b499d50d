"""The feature film on the device (include/mi355rt.h "FEATURE FILM"): per-sample guides, coverage and denoising under any rays.

None of the yardsticks is the code under test.  The accumulation is held to raytracer_rs_amd.features (numpy, f32, operation for operation) fed with the
hits the CPU oracle's intersector gives for the rays mi355rt_lens_rays / raytracer_rs_amd.cameras state; the read-outs under MI355RT_GUIDES_FEATURES to
raytracer_rs_amd.denoise and raytracer_rs_amd.display fed with features.guides(planes).  Every comparison is on the bits (array_equal of uint32 views).

The shapes are the guides' (tests/test_gpu_denoise.py): 100 x 37 and 64 x 53 — widths that are no multiple of 64, 3700 and 3392 pixels: 15 and 14 blocks of 256
lanes with a partial last one — plus a 1 x 1 and a 3 x 2 image (one partial wave).  The poses of the two tiny images were searched on the CPU oracle so that
under every lens a pixel has samples that hit and samples that miss."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_gpu_display import assert_hist, assert_pixels, rgb_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
F = np.float32
MISS = 0xFFFFFFFF
E_INVALID = -1
SEED = 3
PLANES = ("n", "hits", "depth", "normal", "albedo")
# (lens, FIX_ROW_INDEX): pinhole, pinhole with the true row, thin (radius 0.3, focus 4), ortho
LENSES = [(dict(model="pinhole"), 0), (dict(model="pinhole"), 1), (dict(model="thin", radius=0.3, focus=4.0), 0), (dict(model="ortho", width_world=9.5), 0)]
# scene, width, height, (y angle, x angle) of the pose
SHAPES = [("ico2", 100, 37, None), ("thai2", 100, 37, None), ("ico3_tex", 64, 53, None), ("ico2", 1, 1, (-0.5, -0.1)), ("ico2", 3, 2, (-0.3, 0.15))]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ft(pkg):
    return importlib.import_module("raytracer_rs_amd.features")


@pytest.fixture(scope="module")
def dn(pkg):
    return importlib.import_module("raytracer_rs_amd.denoise")


@pytest.fixture(scope="module")
def dp(pkg):
    return importlib.import_module("raytracer_rs_amd.display")


@pytest.fixture(scope="module")
def cams(pkg):
    return importlib.import_module("raytracer_rs_amd.cameras")


def make(pkg, scenes, name, w, h, **kw):
    kw.setdefault("seed", SEED)
    return pkg.create_raytracer_from_arrays(scenes(name), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, **kw)


def last_error(pkg, rt):
    return (pkg.lib().mi355rt_last_error(rt._h) or b"").decode()


def planes_bits(p):
    return {k: (bits(p[k]) if p[k].dtype == np.float32 else np.asarray(p[k])).copy() for k in PLANES}


def assert_planes_equal(got, want, what=""):
    for k in PLANES:
        g, w = planes_bits(got)[k], planes_bits(want)[k]
        assert g.shape == w.shape and np.array_equal(g, w), (what, k, np.flatnonzero((g != w).reshape(g.shape[0], -1).any(1))[:8].tolist())


def assert_guides_equal(got, want):
    assert np.array_equal(got["prim"], want["prim"])
    for k in ("depth", "normal", "albedo"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k


def pose(rt, p):
    if p is not None:
        rt.camera.add_y_angle(p[0]); rt.camera.add_x_angle(p[1])


# ---- 1. the accumulation equals the statement, bit for bit, in all five planes ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,at", SHAPES)
def test_accumulation_equals_the_statement(pkg, scenes, oracle, ft, sem3, name, w, h, at):
    sc = scenes(name)
    brute = bool(sem3.orc & oracle.FLAG_BRUTE_FORCE)
    rt = make(pkg, scenes, name, w, h, flags=sem3.gpu)
    orc = oracle.Oracle(sc, w, h, seed=SEED, flags=sem3.orc)
    pose(rt, at)
    npix = w * h
    for lens, fix in LENSES:
        rt.set_flags(sem3.gpu | (pkg.FLAG_FIX_ROW_INDEX if fix else 0))
        rt.set_lens(**lens)
        rt.features.clear()
        assert_planes_equal(rt.features.get(), ft.empty(npix), "cleared")
        # the film is empty, so lens_rays(6) states the rays of the keys (p, 0 .. 5): the first call takes sample 0, the second numbers on from feat_n = 1
        rays = rt.lens_rays(6).reshape(6, npix, 6)
        tuv, prim = orc.intersect(rays.reshape(-1, 6), brute=brute, nthreads=16)
        tuv, prim = tuv.reshape(6, npix, 3), prim.reshape(6, npix)
        rt.features.render(1)
        want1 = ft.accumulate(ft.empty(npix), tuv[:1], prim[:1], sc, 1)
        assert_planes_equal(rt.features.get(), want1, "%s fix %d, 1 sample" % (lens["model"], fix))
        rt.features.render(5)
        want6 = ft.accumulate(want1, tuv[1:], prim[1:], sc, 5)
        got = rt.features.get()
        assert_planes_equal(got, want6, "%s fix %d, 1 + 5 samples" % (lens["model"], fix))
        assert (got["n"] == 6).all()
        partial = (got["hits"] > 0) & (got["hits"] < 6)
        if npix == 1:
            assert partial.all()                                              # the one pixel: samples that hit and samples that miss
        else:
            assert (got["hits"] == 6).any() and (got["hits"] == 0).any() and partial.any(), (lens, fix)
        assert np.array_equal(bits(rt.features.alpha()), bits(ft.alpha(want6)))
        if name == "ico3_tex":
            assert len(np.unique(got["albedo"][got["hits"] > 0], axis=0)) > 10    # the texture is looked up
    rt.close()


def test_a_film_with_counts_moves_nothing_and_another_base_is_reached_through_the_feature_n(pkg, scenes, oracle, ft):
    """the keys are (p, feat_n[p] + s), not the film's counts: a film set to n = 2 leaves the feature rays where they were, and lens_rays on that film
    states the rays a feature film takes after two samples"""
    name, w, h = "ico2", 37, 21
    sc = scenes(name)
    npix = w * h
    rt = make(pkg, scenes, name, w, h)
    orc = oracle.Oracle(sc, w, h, seed=SEED)
    rt.set_lens("thin", radius=0.3, focus=4.0)
    first = rt.lens_rays(2)
    z = np.zeros((npix, 3), np.float32)
    rt.film.set(z, z, np.full(npix, 2, np.uint32))
    later = rt.lens_rays(3)                                                   # keys (p, 2 .. 4)
    rt.features.render(2); rt.features.render(3)
    rays = np.concatenate([first, later])
    tuv, prim = orc.intersect(rays, nthreads=16)
    assert_planes_equal(rt.features.get(), ft.accumulate(ft.empty(npix), tuv, prim, sc, 5))
    rt.close()


# ---- 2. caller rays ---------------------------------------------------------------------------------------------------------------------------------------
EQ_W, EQ_H, EQ_SPP = 64, 32, 3


def test_caller_rays_equal_the_statement_and_device_equals_host(pkg, scenes, oracle, ft, cams, sem3):
    import torch
    sc = scenes("thai2")
    npix = EQ_W * EQ_H
    rt = make(pkg, scenes, "thai2", EQ_W, EQ_H, flags=sem3.gpu)
    orc = oracle.Oracle(sc, EQ_W, EQ_H, seed=SEED, flags=sem3.orc)
    rays = cams.equirect(rt.camera.matrices(), EQ_W, EQ_H, EQ_SPP, SEED).reshape(-1, 6)
    tuv, prim = orc.intersect(rays, brute=bool(sem3.orc & oracle.FLAG_BRUTE_FORCE), nthreads=16)
    want = ft.accumulate(ft.empty(npix), tuv, prim, sc, EQ_SPP)
    assert (want["hits"] == EQ_SPP).any() and (want["hits"] == 0).any() and ((want["hits"] > 0) & (want["hits"] < EQ_SPP)).any()
    rt.features.render_rays(rays, EQ_SPP)
    assert_planes_equal(rt.features.get(), want, "host")
    # a second call adds onto the first: the left operand is the handle's value
    rt.features.render_rays(rays, EQ_SPP)
    assert_planes_equal(rt.features.get(), ft.accumulate(want, tuv, prim, sc, EQ_SPP), "host, twice")
    rt.features.clear()
    rt.features.render_rays(torch.from_numpy(rays.copy()).to(torch.device("cuda", 0)), EQ_SPP)
    assert_planes_equal(rt.features.get(), want, "device")
    rt.close()


# ---- 3. coverage is the film's ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [dict(model="pinhole"), dict(model="thin", radius=0.3, focus=4.0)])
def test_coverage_is_the_films(pkg, scenes, sem, lens):
    w, h, spp = 100, 37, 4
    rt = make(pkg, scenes, "thai2", w, h, flags=sem.gpu)
    rt.set_lens(**lens)
    prim = rt.trace_rays(rt.lens_rays(spp), want=("prim",))["prim"].reshape(spp, w * h)      # the rays render(spp) is about to take
    c = rt.render(spp)
    rt.features.render(spp)
    got = rt.features.get()
    want = (prim != MISS).sum(0).astype(np.uint32)
    assert np.array_equal(got["hits"], want) and (got["n"] == spp).all()
    assert int(got["hits"].sum()) == c.primary_hits
    assert (want == 0).any() and (want == spp).any() and ((want > 0) & (want < spp)).any()
    rt.close()


# ---- 4. stripes -------------------------------------------------------------------------------------------------------------------------------------------
def test_striped_handles_work_on_their_rows(pkg, scenes, cams):
    w, h = 40, 19
    whole = make(pkg, scenes, "ico2", w, h)
    whole.set_lens("thin", radius=0.3, focus=4.0)
    whole.features.render(2); whole.features.render(1)
    full = whole.features.get()
    assert (full["hits"] > 0).any()
    rays = cams.equirect(whole.camera.matrices(), w, h, 2, SEED).reshape(-1, 6)
    whole.features.clear()
    whole.features.render_rays(rays, 2)
    full_rays = whole.features.get()
    seen = np.zeros(h, bool)
    for rank in (0, 1):
        st = make(pkg, scenes, "ico2", w, h, stripe_rows=4, stripe_rank=rank, stripe_world=2)
        rows = st.owned_rows()
        own = np.zeros(h, bool); own[rows] = True
        assert own.any() and not own.all() and not (seen & own).any()
        seen |= own
        mask = np.repeat(own, w)
        st.set_lens("thin", radius=0.3, focus=4.0)
        st.features.render(2); st.features.render(1)
        for want, what in ((full, "lens"), (full_rays, "rays")):
            if what == "rays":
                st.features.clear()
                assert not any(planes_bits(st.features.get())[k].any() for k in PLANES)
                st.features.render_rays(rays, 2)
            got = st.features.get()
            for k in PLANES:
                g, wv = planes_bits(got)[k], planes_bits(want)[k]
                assert np.array_equal(g[mask], wv[mask]), (rank, what, k)
                assert not g[~mask].any(), (rank, what, k)                    # rows the handle does not own stay zero
            assert np.array_equal(bits(st.features.alpha())[~mask], np.zeros((~mask).sum(), np.uint32))
        st.close()
    assert seen.all()
    whole.close()


# ---- 5. read-outs under FEATURES --------------------------------------------------------------------------------------------------------------------------
PARAMS = dict(normal_power_log2=7, sigma_luminance=1.0, sigma_depth=0.1, sigma_albedo=0.1)


def check_readouts(pkg, rt, dn, dp, guides, split):
    """the denoised read-outs (iterations 0, 1, 5) and display sources 1 and 2 of rt against denoise.py / display.py fed with `guides`"""
    w, h = rt.width, rt.height
    s, q, n = rt.film.pixel_datas()
    d = rt.film.direct_sums() if split else None
    table = pkg.display_srgb_thresholds()
    for it in (0, 1, 5):
        got_rgb, got_packed = rt.get_denoised_pixels(iterations=it, **PARAMS)
        want_rgb, want_packed = dn.denoise(s, q, n, guides, w, h, iterations=it, **PARAMS)
        assert np.array_equal(bits(got_rgb), bits(want_rgb)) and np.array_equal(got_packed, want_packed), it
        images = {pkg.DISPLAY_SOURCE_DENOISED: want_rgb}
        if split:
            got_rgb, got_packed = rt.get_denoised_pixels(split=True, iterations=it, **PARAMS)
            want_rgb, want_packed = dn.denoise_split(s, q, n, d, guides, w, h, iterations=it, **PARAMS)
            assert np.array_equal(bits(got_rgb), bits(want_rgb)) and np.array_equal(got_packed, want_packed), ("split", it)
            images[pkg.DISPLAY_SOURCE_DENOISED_SPLIT] = want_rgb
        for source, rgb in images.items():
            cfg = dict(iterations=it, **PARAMS)
            got, used = rt.get_display_pixels(source=source, curve=pkg.CURVE_ACES, transfer=pkg.TRANSFER_SRGB, exposure=1.5, denoise=cfg)
            assert used == F(1.5)
            assert_pixels(got, dp.display(rgb, 1.5, dp.CURVE_ACES, dp.TRANSFER_SRGB, 4.0, table), "source %d, %d iterations" % (source, it))
            assert_hist(rt.display_histogram(source, **cfg), dp.histogram(rgb, n), "source %d, %d iterations" % (source, it))


@pytest.mark.parametrize("lens", [dict(model="pinhole"), dict(model="thin", radius=0.3, focus=4.0)])
def test_readouts_under_features_equal_the_numpy_filter(pkg, scenes, ft, dn, dp, sem, lens):
    name, w, h = "thai2", 100, 37
    rt = make(pkg, scenes, name, w, h, flags=sem.gpu | pkg.FLAG_DIRECT_FILM)
    never = make(pkg, scenes, name, w, h, flags=sem.gpu | pkg.FLAG_DIRECT_FILM)      # a handle that never touches features
    for r in (rt, never):
        r.set_lens(**lens)
        r.render(4)
    assert rt.guide_source == "centre"
    rt.features.render(4)
    rt.set_guide_source("features")
    assert rt.guide_source == "features" and pkg.lib().mi355rt_get_guide_source(rt._h) == pkg.GUIDES_FEATURES
    planes = rt.features.get()
    want = ft.guides(planes)
    got = rt.guides()
    assert_guides_equal(got, want)
    hit = want["prim"] != MISS
    assert hit.any() and (~hit).any() and set(np.unique(got["prim"]).tolist()) == {0, MISS}
    centre = never.guides()
    assert not np.array_equal(bits(got["depth"]), bits(centre["depth"]))           # the two sources are different guides
    check_readouts(pkg, rt, dn, dp, want, split=True)
    # more samples: the converted guides follow the feature film
    rt.features.render(2)
    want2 = ft.guides(rt.features.get())
    assert not np.array_equal(bits(want2["depth"]), bits(want["depth"]))
    assert_guides_equal(rt.guides(), want2)
    rgb, packed = rt.get_denoised_pixels(**PARAMS)
    s, q, n = rt.film.pixel_datas()
    want_rgb, want_packed = dn.denoise(s, q, n, want2, w, h, iterations=5, **PARAMS)
    assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(packed, want_packed)
    # back to CENTRE: exactly what a handle that never touched features returns
    rt.set_guide_source("centre")
    assert_guides_equal(rt.guides(), centre)
    for kw in (dict(), dict(split=True), dict(iterations=1)):
        a, b = rt.get_denoised_pixels(**kw), never.get_denoised_pixels(**kw)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), kw
    for source in (1, 2):
        assert_pixels(rt.get_display_pixels(source=source)[0], never.get_display_pixels(source=source)[0], "centre, source %d" % source)
        assert_hist(rt.display_histogram(source), never.display_histogram(source))
    rt.close(); never.close()


# ---- 6. the denoiser now serves caller rays ---------------------------------------------------------------------------------------------------------------
def test_the_denoiser_serves_caller_rays(pkg, scenes, ft, dn, dp, cams):
    rt = make(pkg, scenes, "thai2", EQ_W, EQ_H, flags=pkg.FLAG_DIRECT_FILM)
    rays = cams.equirect(rt.camera.matrices(), EQ_W, EQ_H, EQ_SPP, SEED).reshape(-1, 6)
    rt.render_rays(rays, EQ_SPP)
    rt.features.render_rays(rays, EQ_SPP)
    # CENTRE: refused exactly as before
    for call in (lambda: rt.get_denoised_pixels(), lambda: rt.get_denoised_pixels(split=True), lambda: rt.get_display_pixels(source=1), lambda: rt.display_histogram(2)):
        with pytest.raises(RuntimeError, match="the film holds samples of mi355rt_render_rays, which the camera's guides and tiles do not describe"):
            call()
    rt.set_guide_source("features")
    guides = ft.guides(rt.features.get())
    assert (guides["prim"] == 0).any() and (guides["prim"] == MISS).any()
    assert_guides_equal(rt.guides(), guides)
    check_readouts(pkg, rt, dn, dp, guides, split=True)
    with pytest.raises(RuntimeError, match="mi355rt_render_adaptive"):           # stays refused as it was
        rt.render_adaptive()
    # a camera's feature film does not describe a film of caller rays
    rt.features.clear()
    rt.features.render(2)
    with pytest.raises(RuntimeError, match="mi355rt_features_render_rays"):
        rt.get_denoised_pixels()
    with pytest.raises(RuntimeError, match="mi355rt_features_render_rays"):
        rt.get_display_pixels(source=1)
    rt.guides()                                                               # the guides themselves are the camera's: served
    rt.close()


# ---- 7. nothing else moves --------------------------------------------------------------------------------------------------------------------------------
def handle_state(rt, direct):
    s, q, n = rt.film.pixel_datas()
    out = dict(s=bits(s).copy(), q=bits(q).copy(), n=n.copy(), ldr=rt.get_tonemapped_pixels().copy(), row=rt.current_row, counts=rt.last_counts().as_dict())
    if direct:
        out["d"] = bits(rt.film.direct_sums()).copy()
    return out


def same_state(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


def test_feature_calls_leave_everything_else_and_nothing_else_moves_the_feature_film(pkg, scenes, cams):
    w, h = 64, 53
    rt = make(pkg, scenes, "thai2", w, h, flags=pkg.FLAG_DIRECT_FILM)
    rt.render(3)
    rt.trace_frame_additive()
    rt.synchronize()
    before = handle_state(rt, True)
    assert before["row"] != 0 and before["counts"]["primary"] > 0
    rt.features.render(2)
    rt.features.get(); rt.features.alpha()
    rt.set_guide_source("features"); rt.guides(); rt.set_guide_source("centre")
    assert same_state(handle_state(rt, True), before)
    planes = planes_bits(rt.features.get())
    assert planes["hits"].any()
    # render, film.clear, film.set, a lens change and back, and a camera move leave the feature planes as they are
    rt.render(1)
    rt.film.clear()
    z = np.zeros((w * h, 3), np.float32)
    rt.film.set(z, z, np.ones(w * h, np.uint32), z)
    rt.set_lens("ortho", width_world=9.5); rt.set_lens("pinhole")
    rt.camera.move_rel(0.3, -0.2, 0.5)
    after = planes_bits(rt.features.get())
    assert all(np.array_equal(planes[k], after[k]) for k in PLANES)
    state = handle_state(rt, True)
    rt.features.clear()
    assert not any(planes_bits(rt.features.get())[k].any() for k in PLANES)
    assert not bits(rt.features.alpha()).any()
    rt.features.render(1)                                                     # a cleared feature film takes the new view
    assert same_state(handle_state(rt, True), state)
    rt.close()


def test_a_queued_frame_and_a_speculative_frame_are_settled(pkg, scenes, oracle):
    name, w, h = "thai2", 64, 160
    rt = make(pkg, scenes, name, w, h, seed=10)
    orc = oracle.Oracle(scenes(name), w, h, seed=10)
    rt.trace_frame_additive()
    launched0, _ = rt.debug_speculation()
    rt.features.render(1)
    rt.trace_frame_additive()
    orc.trace_frame_additive(); orc.trace_frame_additive()
    assert launched0 >= 1                                                     # a speculative frame was out when the feature pass came
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
    assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())
    # behind a queued frame: the film is the synchronous render's, the feature film that of a handle without a frame in flight
    a = make(pkg, scenes, name, 100, 37); b = make(pkg, scenes, name, 100, 37)
    a.render(2, wait=False)
    a.features.render(2)
    b.render(2); b.features.render(2)
    assert np.array_equal(a.last_counts().as_dict()["primary"], b.last_counts().as_dict()["primary"])
    for x, y in zip(a.film.pixel_datas(), b.film.pixel_datas()):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    fa, fb = planes_bits(a.features.get()), planes_bits(b.features.get())
    assert all(np.array_equal(fa[k], fb[k]) for k in PLANES)
    for r in (rt, a, b):
        r.close()


# ---- 8. guards and errors ---------------------------------------------------------------------------------------------------------------------------------
def test_guards_and_errors_write_nothing(pkg, scenes, cams):
    import torch
    w, h = 33, 29
    npix = w * h
    L = pkg.lib()
    rt = make(pkg, scenes, "ico2", w, h)
    rays = cams.equirect(rt.camera.matrices(), w, h, 2, SEED).reshape(-1, 6)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def refused(code, *words):
        assert code == E_INVALID
        for word in words:
            assert word in last_error(pkg, rt), (word, last_error(pkg, rt))

    # an empty feature film under FEATURES; an unknown source
    rt.render(2)
    refused(L.mi355rt_set_guide_source(rt._h, 2), "mi355rt_set_guide_source", "source")
    assert rt.guide_source == "centre"
    rt.set_guide_source("features")
    out_rgb = np.full((npix, 3), 7.0, np.float32); out_px = np.full(npix, 0x12345678, np.uint32); out_d = np.full(npix, 7.0, np.float32)
    cfg = pkg.denoise_config()
    refused(L.mi355rt_get_denoised_pixels(rt._h, C.byref(cfg), fp(out_rgb), up(out_px), npix), "empty", "mi355rt_features_render")
    refused(L.mi355rt_get_guides(rt._h, fp(out_d), None, None, None, npix), "empty")
    dcfg = pkg.display_config(source=1)
    refused(L.mi355rt_get_display_pixels(rt._h, C.byref(dcfg), None, up(out_px), npix, None), "empty")
    hist = pkg.LuminanceHistogram()
    refused(L.mi355rt_display_histogram(rt._h, 1, None, C.byref(hist)), "empty")
    assert (out_rgb == 7.0).all() and (out_px == 0x12345678).all() and (out_d == 7.0).all() and not np.array(hist.bins).any()
    rt.get_display_pixels(source=0); rt.display_histogram(0)                   # the film itself needs no guides

    # spp == 0, a wrong nrays, a NULL ray pointer, an unknown `where`; a wrong npix, all-NULL outputs — on a feature film that holds samples
    rt.features.render(2)
    held = planes_bits(rt.features.get())
    stamp = lambda: all(np.array_equal(held[k], planes_bits(rt.features.get())[k]) for k in PLANES)
    refused(L.mi355rt_features_render(rt._h, 0), "mi355rt_features_render", "spp")
    n = np.zeros(npix, np.uint32)
    refused(L.mi355rt_features_get(rt._h, up(n), None, None, None, None, npix - 1), "mi355rt_features_get", "npix")
    refused(L.mi355rt_features_get(rt._h, up(n), None, None, None, None, npix + 1), "npix")
    refused(L.mi355rt_features_get(rt._h, None, None, None, None, None, npix), "NULL")
    alpha = np.full(npix, 7.0, np.float32)
    refused(L.mi355rt_features_alpha(rt._h, fp(alpha), npix - 1), "mi355rt_features_alpha", "npix")
    refused(L.mi355rt_features_alpha(rt._h, None, npix), "alpha")
    assert not n.any() and (alpha == 7.0).all() and stamp()
    rt.features.clear()
    held = planes_bits(rt.features.get())
    refused(L.mi355rt_features_render_rays(rt._h, rays.ctypes.data, 2 * npix, 0, pkg.RAYS_HOST), "mi355rt_features_render_rays", "spp")
    refused(L.mi355rt_features_render_rays(rt._h, rays.ctypes.data, 2 * npix - 1, 2, pkg.RAYS_HOST), "nrays")
    refused(L.mi355rt_features_render_rays(rt._h, rays.ctypes.data, 2 * npix, 3, pkg.RAYS_HOST), "nrays")
    refused(L.mi355rt_features_render_rays(rt._h, None, 2 * npix, 2, pkg.RAYS_HOST), "rays6")
    refused(L.mi355rt_features_render_rays(rt._h, rays.ctypes.data, 2 * npix, 2, 2), "where")
    assert stamp()
    with pytest.raises(ValueError):
        rt.features.render_rays(torch.from_numpy(rays), 2)                    # a CPU tensor
    with pytest.raises(ValueError):
        rt.features.render_rays(rays[:, :5].copy(), 2)
    refused(L.mi355rt_get_guides(rt._h, fp(out_d), None, None, None, npix), "empty")       # cleared: empty again

    # camera and caller rays mixed
    rt.features.render_rays(rays, 2)
    held = planes_bits(rt.features.get())
    refused(L.mi355rt_features_render(rt._h, 1), "mi355rt_features_clear", "caller")
    assert stamp()
    rt.features.clear()
    rt.features.render(1)
    held = planes_bits(rt.features.get())
    refused(L.mi355rt_features_render_rays(rt._h, rays.ctypes.data, 2 * npix, 2, pkg.RAYS_HOST), "mi355rt_features_clear", "camera")
    assert stamp()

    # a view change (camera, lens, the FIX_ROW_INDEX bit), then features.render or a FEATURES read-out
    changes = [(lambda: rt.camera.add_y_angle(0.25), lambda: rt.camera.add_y_angle(-0.25)),
               (lambda: rt.set_lens("thin", radius=0.3, focus=4.0), lambda: rt.set_lens("pinhole")),
               (lambda: rt.set_flags(pkg.FLAG_FIX_ROW_INDEX), lambda: rt.set_flags(0))]
    for k, (change, undo) in enumerate(changes):
        rt.guides(); rt.get_denoised_pixels()                                  # served while the view is the stamp's
        change()
        refused(L.mi355rt_features_render(rt._h, 1), "mi355rt_features_render", "mi355rt_features_clear")
        refused(L.mi355rt_get_guides(rt._h, fp(out_d), None, None, None, npix), "mi355rt_get_guides", "mi355rt_features_clear")
        refused(L.mi355rt_get_denoised_pixels(rt._h, C.byref(cfg), fp(out_rgb), up(out_px), npix), "mi355rt_features_clear")
        refused(L.mi355rt_get_display_pixels(rt._h, C.byref(dcfg), None, up(out_px), npix, None), "mi355rt_features_clear")
        refused(L.mi355rt_display_histogram(rt._h, 1, None, C.byref(hist)), "mi355rt_features_clear")
        assert stamp() and (out_rgb == 7.0).all() and (out_px == 0x12345678).all() and (out_d == 7.0).all()
        if k == 0:
            undo()                                                            # back at the stamp's view: served again
            rt.features.render(1)
            held = planes_bits(rt.features.get())
        else:
            rt.features.clear(); rt.features.render(1)                        # or cleared and taken under the new view
            held = planes_bits(rt.features.get())
            rt.guides()
    rt.close()


def test_a_device_group_is_refused(pkg, scenes, cams):
    w, h = 32, 24
    npix = w * h
    rt = make(pkg, scenes, "ico2", w, h, device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    rays = cams.equirect(rt.camera.matrices(), w, h, 1, SEED).reshape(-1, 6)
    hbm = rt.hbm_allocated_bytes()
    n = np.full(npix, 7, np.uint32); a = np.full(npix, 7.0, np.float32)
    L = pkg.lib()
    calls = [lambda: L.mi355rt_features_render(rt._h, 1), lambda: L.mi355rt_features_render_rays(rt._h, rays.ctypes.data, npix, 1, pkg.RAYS_HOST),
             lambda: L.mi355rt_features_get(rt._h, n.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None, None, npix),
             lambda: L.mi355rt_features_alpha(rt._h, a.ctypes.data_as(C.POINTER(C.c_float)), npix), lambda: L.mi355rt_features_clear(rt._h),
             lambda: L.mi355rt_set_guide_source(rt._h, pkg.GUIDES_FEATURES)]
    for call in calls:
        assert call() == E_INVALID and "device group" in last_error(pkg, rt)
    assert (n == 7).all() and (a == 7.0).all() and rt.hbm_allocated_bytes() == hbm and rt.guide_source == "centre"
    rt.close()


# ---- 9. memory --------------------------------------------------------------------------------------------------------------------------------------------
def test_memory_is_allocated_on_first_use_and_counted(pkg, scenes, monkeypatch):
    """The planes and the converted guides are DeviceBuffers of the handle's one memory owner: they count into hbm_allocated_bytes from the call that needs
    them, and that owner frees what it counts when the handle goes (a closed handle has no counter left to read)."""
    monkeypatch.setenv("MI355RT_DEBUG_GUARD", "1")
    w, h = 100, 37
    npix = w * h
    rt = make(pkg, scenes, "thai2", w, h)
    rt.render(2); rt.get_tonemapped_pixels()
    hbm0 = rt.hbm_allocated_bytes()
    rt.render(2); rt.guide_source; rt.features.clear(); rt.features.get(); rt.features.alpha(); rt.set_guide_source("centre")
    assert rt.hbm_allocated_bytes() == hbm0                                   # nothing before the first accumulation
    rt.features.render(1)
    assert rt.hbm_allocated_bytes() - hbm0 == 36 * npix                       # the five planes
    rt.features.render(3); rt.features.get(); rt.features.alpha(); rt.features.clear(); rt.features.render(1)
    assert rt.hbm_allocated_bytes() - hbm0 == 36 * npix
    rt.set_guide_source("features")
    rt.guides()
    assert rt.hbm_allocated_bytes() - hbm0 == (36 + 32) * npix                # + the converted guides
    rt.get_denoised_pixels()
    assert rt.hbm_allocated_bytes() - hbm0 == (36 + 32 + 52) * npix           # + the filter's buffers, as under CENTRE
    rt.set_guide_source("centre")
    rt.get_denoised_pixels()
    assert rt.hbm_allocated_bytes() - hbm0 == (36 + 32 + 52 + 32) * npix      # + the centre-ray guides: each source keeps its cache
    assert rt.debug_check_guards() == 0
    rt.close()


# ---- 10. the CLI ------------------------------------------------------------------------------------------------------------------------------------------
def read_png_rgba(path):
    """(width, height, uint8[npix, 4]) of an 8-bit RGBA PNG (colour type 6) whose scanlines all use filter 0"""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        ln, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + ln]
        if kind == b"IHDR":
            size = struct.unpack(">II", body[:8]); assert body[8:] == bytes([8, 6, 0, 0, 0])
        elif kind == b"IDAT":
            idat += body
        pos += 12 + ln
    w, h = size
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    assert not raw[:, 0].any()
    return w, h, raw[:, 1:].reshape(-1, 4)


def test_cli_writes_the_feature_guided_read_out_with_alpha(pkg, scenes, tmp_path):
    from test_gpu_display import read_png
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    w, h = 48, 40
    base = [exe, "-f", os.path.join(SCENES, "thai2.scene"), "--width", str(w), "--height", str(h), "--seed", "17", "--spp", "4"]
    out = tmp_path / "x.png"
    r = subprocess.run(base + ["--features", "4", "--denoise", "--denoise-guides", "features", "--alpha", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "features: 4 samples per pixel\n" in r.stdout
    rt = make(pkg, scenes, "thai2", w, h, seed=17)
    rt.render(4)
    _, centre = rt.get_denoised_pixels(rgb=False)
    rt.features.render(4)
    rt.set_guide_source("features")
    _, px = rt.get_denoised_pixels(rgb=False)
    alpha = rt.features.alpha()
    a8 = (alpha * F(255.0) + F(0.5)).astype(np.uint32).astype(np.uint8)
    pw, ph, rgba = read_png_rgba(out)
    assert (pw, ph) == (w, h)
    assert np.array_equal(rgba[:, :3], rgb_of(px)) and np.array_equal(rgba[:, 3], a8)
    assert (a8 == 0).any() and (a8 == 255).any() and ((a8 > 0) & (a8 < 255)).any() and not np.array_equal(px, centre)
    assert not rgba[a8 == 0][:, :3].any()                                     # premultiplied by construction: no coverage, no colour
    # without the new options the CLI writes the bytes it always wrote; --denoise-guides centre is the default
    plain = tmp_path / "y.png"
    r = subprocess.run(base + ["--denoise", "--out", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "features:" not in r.stdout
    assert np.array_equal(read_png(plain)[2], rgb_of(centre))
    r = subprocess.run(base + ["--features", "4", "--denoise", "--denoise-guides", "centre", "--out", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and np.array_equal(read_png(plain)[2], rgb_of(centre))
    # the options name what they need
    for extra, word in ((["--denoise-guides", "features"], "--features"), (["--alpha", "--out", str(out)], "--features"),
                        (["--features", "2", "--alpha", "--out", str(tmp_path / "a.ppm")], ".png"), (["--denoise-guides", "sharp"], "centre or features")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
    rt.close()


def test_cli_denoises_an_orthographic_view_through_the_feature_film(pkg, scenes, cams, tmp_path):
    from test_gpu_display import read_png
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    w, h, spp = 48, 40, 3
    out = tmp_path / "o.png"
    base = [exe, "-f", os.path.join(SCENES, "thai2.scene"), "--width", str(w), "--height", str(h), "--seed", "17", "--spp", str(spp), "--ortho-width", "9.5"]
    r = subprocess.run(base + ["--features", str(spp), "--denoise", "--denoise-guides", "features", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rt = make(pkg, scenes, "thai2", w, h, seed=17)
    rays = cams.orthographic(rt.camera.matrices(), w, h, spp, 17, 9.5).reshape(-1, 6)
    rt.render_rays(rays, spp)
    rt.features.render_rays(rays, spp)
    rt.set_guide_source("features")
    _, px = rt.get_denoised_pixels(rgb=False)
    assert np.array_equal(read_png(out)[2], rgb_of(px))
    r = subprocess.run(base + ["--denoise", "--out", str(out)], capture_output=True, text=True, timeout=300)      # as before: no camera guides for these rays
    assert r.returncode != 0 and "--ortho-width" in r.stderr
    rt.close()
