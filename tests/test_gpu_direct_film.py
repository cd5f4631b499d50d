"""The direct film and the split denoised read-out on the device (include/mi355rt.h): a handle created with FLAG_DIRECT_FILM
keeps, per pixel, the f32 sum of its samples' root light terms -- bit-equal to the CPU oracle's node_L[0] summed in sample order, however
the samples arrive (whole frames, passes, adaptive rounds, 50-row calls with and without speculation); the flag changes nothing else;
the split read-out equals its numpy statement (raytracer_rs_amd.denoise.denoise_split) bit for bit, reads only, refuses what it cannot
serve, and is closer to the converged image than the raw film and the plain denoised read-out of the same film; the CLI."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
F = np.float32
MISS = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dn(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.denoise")


def make(pkg, scenes, name, w, h, flags=0, direct=True, **kw):
    return pkg.create_raytracer_from_arrays(scenes(name), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h,
                                            flags=flags | (pkg.FLAG_DIRECT_FILM if direct else 0), **kw)


_PREFIX = {}


def direct_prefix(oracle, scenes, name, w, h, seed, flags, kmax, camera=None):
    """P[k, p] = the f32 sum over s < k of the oracle's node_L[0] of sample s of pixel p, added in sample order (P[0] = 0): what the
    direct film of a pixel with k samples holds.  Computed once per (scene, size, seed, flags, camera) and shared; never modified."""
    key = (name, w, h, seed, flags, camera)
    have = _PREFIX.get(key)
    if have is not None and have.shape[0] > kmax:
        return have
    orc = oracle.Oracle(scenes(name), w, h, seed=seed, flags=flags)
    if camera:
        orc.camera_move_rel(*camera)
    P = np.zeros((kmax + 1, w * h, 3), np.float32)
    for p in range(w * h):
        for s in range(kmax):
            P[s + 1, p] = P[s, p] + orc.sample_debug(p, s)[1][0]
    P.setflags(write=False)
    _PREFIX[key] = P
    return P


def direct_for(P, n):
    """the direct film of pixels with n[p] samples each"""
    return P[np.asarray(n, np.int64), np.arange(len(n))]


def assert_film_equals_oracle(rt, orc):
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
    return on


# ---- 1. the direct film equals the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("ico2", 37, 21), ("thai2", 37, 21), ("ico3_tex", 40, 27)])
def test_direct_film_equals_the_oracle(pkg, scenes, oracle, sem3, name, w, h):
    spp = 5
    for fix_row in (False, True):
        gflags = sem3.gpu | (pkg.FLAG_FIX_ROW_INDEX if fix_row else 0)
        oflags = sem3.orc | (oracle.FLAG_FIX_ROW_INDEX if fix_row else 0)
        rt = make(pkg, scenes, name, w, h, flags=gflags, seed=5)
        assert not rt.film.direct_sums().any()                       # zero at creation
        rt.render(spp)
        orc = oracle.Oracle(scenes(name), w, h, seed=5, flags=oflags)
        orc.render(spp, nthreads=8)
        assert_film_equals_oracle(rt, orc)
        d = rt.film.direct_sums()
        want = direct_prefix(oracle, scenes, name, w, h, 5, oflags, spp)[spp]
        assert np.array_equal(bits(d), bits(want))
        s = rt.film.pixel_datas()[0]
        assert d.any() and not np.array_equal(bits(d), bits(s))      # there is direct light, and it is not the whole film


# ---- 2. it does not depend on how the samples arrive -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["two_calls", "small_passes", "no_raster", "no_cull_cache", "two_slices"])
def test_direct_film_does_not_depend_on_how_samples_arrive(pkg, scenes, oracle, monkeypatch, variant):
    name, w, h = "thai2", 37, 21
    if variant == "no_raster":
        monkeypatch.setenv("MI355RT_NO_RASTER", "1")
    if variant == "no_cull_cache":
        monkeypatch.setenv("MI355RT_NO_CULL_CACHE", "1")
    rt = make(pkg, scenes, name, w, h, seed=5, **(dict(samples_per_pass=2) if variant == "small_passes" else {}))
    if variant == "two_slices":
        rt.set_slices(2)
    if variant == "two_calls":
        rt.render(2); rt.render(3)
    else:
        rt.render(5)
    want = direct_prefix(oracle, scenes, name, w, h, 5, 0, 5)[5]
    assert np.array_equal(bits(rt.film.direct_sums()), bits(want))


def test_direct_film_follows_adaptive_rounds(pkg, scenes, oracle):
    """batches of 3 samples on 8 x 8 tiles of a 24-wide image: the 256-sample chunks of a pass straddle tiles; a pixel of a tile that has
    settled is not written any more and keeps its sum"""
    name, w, h = "thai2", 24, 16
    rt = make(pkg, scenes, name, w, h, seed=4)
    st = rt.render_adaptive(min_spp=3, max_spp=12, batch_spp=3, max_rounds=0, rel_error=0.3, abs_floor=0.05)
    n = rt.film.pixel_datas()[2]
    print("adaptive: rounds %d, n %s" % (st["rounds"], np.unique(n).tolist()))
    assert st["rounds"] >= 2 and len(np.unique(n)) > 1
    P = direct_prefix(oracle, scenes, name, w, h, 4, 0, 12)
    assert np.array_equal(bits(rt.film.direct_sums()), bits(direct_for(P, n)))


# ---- 3. the drop-in loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speculate", [True, False])
def test_direct_film_in_the_drop_in_loop(pkg, scenes, oracle, monkeypatch, speculate):
    name, w, h = "thai2", 32, 120                                     # the 50-row window wraps on the third call
    if not speculate:
        monkeypatch.setenv("MI355RT_NO_SPECULATE", "1")
    rt = make(pkg, scenes, name, w, h, seed=6)
    orc = oracle.Oracle(scenes(name), w, h, seed=6)
    for _ in range(7):
        rt.trace_frame_additive(); orc.trace_frame_additive()
        assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())
    launched, adopted = rt.debug_speculation()
    assert (launched >= 1 and adopted >= 1) if speculate else launched == 0
    P = direct_prefix(oracle, scenes, name, w, h, 6, 0, 4)
    d1 = rt.film.direct_sums()                                        # a speculative frame is out (if any): its rows are put back first
    on = orc.film()[2]
    assert on.min() < on.max()
    assert np.array_equal(bits(d1), bits(direct_for(P, on)))
    assert_film_equals_oracle(rt, orc)                                # settles the speculation (again: nothing is out)
    assert np.array_equal(bits(rt.film.direct_sums()), bits(d1))
    rt.trace_frame_additive(); orc.trace_frame_additive()             # ... and the loop goes on from the restored rows
    on = assert_film_equals_oracle(rt, orc)
    assert np.array_equal(bits(rt.film.direct_sums()), bits(direct_for(P, on)))
    # a camera move of the reference's loop (main.rs:116-169: move, film.clear()) zeroes it
    rt.camera.move_rel(0.1, 0.0, 0.05); orc.camera_move_rel(0.1, 0.0, 0.05)
    rt.film.clear(); orc.film_clear()
    assert not rt.film.direct_sums().any()
    rt.trace_frame_additive(); orc.trace_frame_additive()
    on = assert_film_equals_oracle(rt, orc)
    Pm = direct_prefix(oracle, scenes, name, w, h, 6, 0, 1, camera=(0.1, 0.0, 0.05))
    d = rt.film.direct_sums()
    assert d.any() and np.array_equal(bits(d), bits(direct_for(Pm, on)))


def test_direct_film_in_the_drop_in_loop_of_a_short_image(pkg, scenes, oracle):
    name, w, h = "thai2", 20, 30                                      # height < 50: every call wraps
    rt = make(pkg, scenes, name, w, h, seed=7)
    orc = oracle.Oracle(scenes(name), w, h, seed=7)
    for _ in range(2):                                                # 100 rows over 30: rows 0-9 hold 4 samples, the others 3
        rt.trace_frame_additive(); orc.trace_frame_additive()
        rt.get_tonemapped_pixels()
    on = assert_film_equals_oracle(rt, orc)
    P = direct_prefix(oracle, scenes, name, w, h, 7, 0, int(on.max()))
    assert on.min() < on.max()
    assert np.array_equal(bits(rt.film.direct_sums()), bits(direct_for(P, on)))


# ---- 4. the flag changes nothing else ---------------------------------------------------------------------------------------------------
COUNTERS = ("primary", "bounce", "shadow", "primary_hits", "primary_culled", "shadow_skipped")


def test_the_flag_changes_nothing_else(pkg, scenes):
    name, w, h = "thai2", 40, 110
    off = make(pkg, scenes, name, w, h, seed=8, direct=False)
    on = make(pkg, scenes, name, w, h, seed=8)
    assert on.hbm_allocated_bytes() - off.hbm_allocated_bytes() == 12 * w * h

    def same(counts=True):
        for a, b in zip(off.film.pixel_datas(), on.film.pixel_datas()):
            assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
        assert np.array_equal(bits(off.film.get_pixels()), bits(on.film.get_pixels()))
        assert np.array_equal(off.get_tonemapped_pixels(), on.get_tonemapped_pixels())
        (ra, pa), (rb, pb) = off.get_denoised_pixels(), on.get_denoised_pixels()
        assert np.array_equal(bits(ra), bits(rb)) and np.array_equal(pa, pb)
        if counts:
            ca, cb = off.last_counts(), on.last_counts()
            assert [getattr(ca, k) for k in COUNTERS] == [getattr(cb, k) for k in COUNTERS]
    off.render(3); on.render(3)
    same()
    for _ in range(4):                                                # a drop-in sequence: the window wraps on the third call
        assert off.trace_frame_additive() == on.trace_frame_additive()
        assert np.array_equal(off.get_tonemapped_pixels(), on.get_tonemapped_pixels())
    same()
    cfg = dict(min_spp=4, max_spp=13, batch_spp=3, max_rounds=0, rel_error=0.1, abs_floor=0.03)
    assert off.render_adaptive(**cfg) == on.render_adaptive(**cfg)
    same()
    assert len(np.unique(on.film.pixel_datas()[2])) > 1


# ---- 5. the split filter equals numpy ---------------------------------------------------------------------------------------------------
def tri_normals(scene):
    """calc_normal (mod.rs:198-205) in vecmath.rs order: cross(v1 - v0, v2 - v0), then normalized (sqrt((x*x + y*y) + z*z), three divisions)"""
    v = np.asarray(scene["tri_verts"], np.float32).reshape(-1, 9)
    a = v[:, 3:6] - v[:, 0:3]; b = v[:, 6:9] - v[:, 0:3]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.stack([cx / ln, cy / ln, cz / ln], axis=1).astype(np.float32)


def fetch_texel(tex, u, v):
    """texture.rs:21-27 as kernels.hip restates it: `as usize` truncation (NaN and negatives -> 0), the index clamped to the last texel"""
    th, tw = tex.shape[0], tex.shape[1]
    n = tw * th
    fx = u.astype(np.float32) * F(tw); fy = v.astype(np.float32) * F(th)
    x = np.where(fx > 0, np.minimum(fx, F(n + 1)), F(0)).astype(np.int64)
    y = np.where(fy > 0, np.minimum(fy, F(n + 1)), F(0)).astype(np.int64)
    i = np.minimum(np.minimum(y, n) * tw + np.minimum(x, n), n - 1)
    return np.asarray(tex, np.float32).reshape(-1, 3)[i]


def oracle_guides(orc, scene, w, h, fix_row, brute):
    """the guide buffers from the oracle: get_ray(u, v, 0.5, 0.5) with the film's pixel -> (u, v) mapping, intersect, normals, albedo"""
    p = np.arange(w * h)
    u = p % w; v = p // w if fix_row else p // h
    rays = np.stack([orc.get_ray(int(a), int(b), 0.5, 0.5) for a, b in zip(u, v)])
    tuv, prim = orc.intersect(rays, brute=brute, nthreads=16)
    hit = prim != MISS
    g = dict(depth=np.zeros(w * h, np.float32), normal=np.zeros((w * h, 3), np.float32), albedo=np.zeros((w * h, 3), np.float32),
             prim=prim.astype(np.uint32))
    pi = prim[hit].astype(np.int64)
    g["depth"][hit] = tuv[hit, 0]
    g["normal"][hit] = tri_normals(scene)[pi]
    geom = np.asarray(scene["tri_geom"], np.int64)[pi]
    kind = np.asarray(scene["mat_kind"])[geom]
    alb = np.asarray(scene["mat_rgb"], np.float32)[geom].copy()
    for m in np.unique(geom[kind == 1]):
        sel = geom == m
        alb[sel] = fetch_texel(scene["textures"][int(scene["mat_tex"][m])], tuv[hit][sel, 1], tuv[hit][sel, 2])
    g["albedo"][hit] = alb
    return g


PARAMS = [dict(normal_power_log2=7, sigma_luminance=1.0, sigma_depth=0.1, sigma_albedo=0.1),
          dict(normal_power_log2=0, sigma_luminance=0.5, sigma_depth=1.0, sigma_albedo=2.0),
          dict(normal_power_log2=10, sigma_luminance=40.0, sigma_depth=0.01, sigma_albedo=0.02)]


def check_split(rt, dn, guides, iterations=range(7), params=PARAMS):
    s, q, n = rt.film.pixel_datas()
    d = rt.film.direct_sums()
    differs = False
    for prm in params:
        for it in iterations:
            got_rgb, got_packed = rt.get_denoised_pixels(split=True, iterations=it, **prm)
            want_rgb, want_packed = dn.denoise_split(s, q, n, d, guides, rt.width, rt.height, iterations=it, **prm)
            assert np.array_equal(bits(got_rgb), bits(want_rgb)), (prm, it)
            assert np.array_equal(got_packed, want_packed), (prm, it)
            _, only_packed = rt.get_denoised_pixels(split=True, rgb=False, iterations=it, **prm)
            only_rgb, _ = rt.get_denoised_pixels(split=True, packed=False, iterations=it, **prm)
            assert np.array_equal(only_packed, want_packed) and np.array_equal(bits(only_rgb), bits(want_rgb))
            if it:
                differs |= not np.array_equal(bits(got_rgb), bits(rt.get_denoised_pixels(packed=False, iterations=it, **prm)[0]))
    # iterations = 0 is exactly get_pixels / get_tonemapped_pixels
    rgb, packed = rt.get_denoised_pixels(split=True, iterations=0)
    assert np.array_equal(bits(rgb), bits(rt.film.get_pixels())) and np.array_equal(packed, rt.get_tonemapped_pixels())
    assert differs                                                   # ... and with iterations it is not the plain read-out


def test_split_filter_equals_numpy_on_a_uniform_render(pkg, scenes, oracle, dn):
    name, w, h = "thai2", 60, 45
    rt = make(pkg, scenes, name, w, h, seed=5)
    rt.render(8)
    g = oracle_guides(oracle.Oracle(scenes(name), w, h, seed=5), scenes(name), w, h, False, False)
    check_split(rt, dn, g)


def test_split_filter_equals_numpy_on_an_adaptive_film(pkg, scenes, oracle, dn):
    name, w, h = "ico3_tex", 48, 40
    rt = make(pkg, scenes, name, w, h, seed=6, flags=pkg.FLAG_FIX_ROW_INDEX)
    rt.render_adaptive(min_spp=2, max_spp=12, batch_spp=2, rel_error=0.1, abs_floor=0.05)
    assert len(np.unique(rt.film.pixel_datas()[2])) > 1            # pixels with unequal n
    g = oracle_guides(oracle.Oracle(scenes(name), w, h, seed=6, flags=oracle.FLAG_FIX_ROW_INDEX), scenes(name), w, h, True, False)
    check_split(rt, dn, g, iterations=(0, 1, 3, 5), params=PARAMS[:2])


def test_split_filter_equals_numpy_on_a_drop_in_film(pkg, scenes, oracle, dn):
    """a few 50-row calls: empty rows (n == 0) beside rows of one sample (unknown variance), then rows of one beside rows of two"""
    name, w, h = "thai2", 40, 160
    rt = make(pkg, scenes, name, w, h, seed=7)
    g = oracle_guides(oracle.Oracle(scenes(name), w, h, seed=7), scenes(name), w, h, False, False)
    for want in ({0, 1}, {1, 2}):
        for _ in range(2):
            rt.trace_frame_additive()
        n = rt.film.pixel_datas()[2]
        assert set(np.unique(n).tolist()) == want
        check_split(rt, dn, g, iterations=(0, 1, 2, 4, 6), params=PARAMS[:2])
        rgb, packed = rt.get_denoised_pixels(split=True)
        assert np.isnan(rgb[n == 0]).all() and (packed[n == 0] == 0xFFFFFFFF).all()
        assert np.isfinite(rgb[n != 0]).all()


def test_split_filter_equals_numpy_on_a_textured_scene(pkg, scenes, oracle, dn):
    name, w, h = "ico3_tex", 64, 53
    rt = make(pkg, scenes, name, w, h, seed=3)
    rt.render(4)
    g = oracle_guides(oracle.Oracle(scenes(name), w, h, seed=3), scenes(name), w, h, False, False)
    check_split(rt, dn, g, iterations=(0, 5), params=PARAMS[:1])


# ---- 6. no side effects, and errors -----------------------------------------------------------------------------------------------------
def test_split_read_out_leaves_everything_and_allocates_on_first_use(pkg, scenes, monkeypatch):
    monkeypatch.setenv("MI355RT_DEBUG_GUARD", "1")
    w, h = 64, 48
    rt = make(pkg, scenes, "thai2", w, h, seed=9)
    rt.render(4)
    film0 = [np.asarray(x).copy() for x in rt.film.pixel_datas()]
    d0 = rt.film.direct_sums().copy()
    ldr0 = rt.get_tonemapped_pixels().copy()
    hbm0 = rt.hbm_allocated_bytes()
    rt.get_denoised_pixels(split=True)
    assert rt.hbm_allocated_bytes() - hbm0 == (32 + 52) * w * h      # the guides and the filter's buffers, as for the plain read-out
    rt.get_denoised_pixels(split=True, iterations=7); rt.get_denoised_pixels(); rt.get_denoised_pixels(split=True, rgb=False)
    assert rt.hbm_allocated_bytes() - hbm0 == (32 + 52) * w * h      # shared with it, nothing more
    for x, y in zip(film0, rt.film.pixel_datas()):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    assert np.array_equal(bits(d0), bits(rt.film.direct_sums()))
    assert np.array_equal(ldr0, rt.get_tonemapped_pixels())
    assert rt.debug_check_guards() == 0


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def uptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def last_error(pkg, rt):
    return pkg.lib().mi355rt_last_error(rt._h).decode()


def test_a_handle_without_the_flag_is_refused_and_nothing_is_written(pkg, scenes):
    w, h = 32, 24
    npix = w * h
    rt = make(pkg, scenes, "ico2", w, h, seed=12, direct=False)
    rt.render(2)
    L = pkg.lib()
    d = np.full((npix, 3), 7.0, np.float32); rgb = np.full((npix, 3), 7.0, np.float32); packed = np.full(npix, 0x12345678, np.uint32)
    assert L.mi355rt_film_get_direct(rt._h, fptr(d)) == -1
    assert "MI355RT_FLAG_DIRECT_FILM" in last_error(pkg, rt)
    assert L.mi355rt_get_denoised_pixels_split(rt._h, C.byref(pkg.denoise_config()), fptr(rgb), uptr(packed), npix) == -1
    assert "MI355RT_FLAG_DIRECT_FILM" in last_error(pkg, rt)
    assert (d == 7.0).all() and (rgb == 7.0).all() and (packed == 0x12345678).all()
    with pytest.raises(RuntimeError, match="MI355RT_FLAG_DIRECT_FILM"):
        rt.film.direct_sums()
    with pytest.raises(RuntimeError, match="MI355RT_FLAG_DIRECT_FILM"):
        rt.get_denoised_pixels(split=True)
    # the flag is a create-time flag, in both directions
    with pytest.raises(RuntimeError, match="create-time"):
        rt.set_flags(pkg.FLAG_DIRECT_FILM)
    assert L.mi355rt_set_flags(rt._h, pkg.FLAG_DIRECT_FILM | pkg.FLAG_FIX_ROW_INDEX) == -1
    on = make(pkg, scenes, "ico2", w, h, seed=12)
    with pytest.raises(RuntimeError, match="DIRECT_FILM"):
        on.set_flags(0)
    on.set_flags(pkg.FLAG_DIRECT_FILM | pkg.FLAG_FIX_ROW_INDEX)       # the run-time flags still change
    on.render(1)
    assert on.film.direct_sums().any()


def test_split_read_out_checks_its_arguments_like_the_plain_one(pkg, scenes):
    w, h = 32, 24
    npix = w * h
    rt = make(pkg, scenes, "ico2", w, h, seed=12)
    rt.render(2)
    L = pkg.lib()
    rgb = np.full((npix, 3), 7.0, np.float32); packed = np.full(npix, 0x12345678, np.uint32)
    for field, kw in [("iterations", dict(iterations=11)), ("normal_power_log2", dict(normal_power_log2=11)),
                      ("sigma_luminance", dict(sigma_luminance=0.0)), ("sigma_depth", dict(sigma_depth=float("inf"))),
                      ("sigma_albedo", dict(sigma_albedo=float("nan")))]:
        assert L.mi355rt_get_denoised_pixels_split(rt._h, C.byref(pkg.denoise_config(**kw)), fptr(rgb), uptr(packed), npix) == -1
        assert field in last_error(pkg, rt)
    assert L.mi355rt_get_denoised_pixels_split(rt._h, C.byref(pkg.denoise_config()), fptr(rgb), uptr(packed), npix - 1) == -1
    assert "npix" in last_error(pkg, rt)
    assert L.mi355rt_get_denoised_pixels_split(rt._h, C.byref(pkg.denoise_config()), None, None, npix) == -1
    assert "both NULL" in last_error(pkg, rt)
    assert L.mi355rt_get_denoised_pixels_split(rt._h, None, fptr(rgb), None, npix) == -1
    assert "null config" in last_error(pkg, rt)
    assert L.mi355rt_film_get_direct(rt._h, None) == -1
    assert (rgb == 7.0).all() and (packed == 0x12345678).all()


@pytest.mark.parametrize("kind", ["device_group", "striped"])
def test_groups_and_stripes_read_the_direct_film_but_not_the_split_read_out(pkg, scenes, kind):
    name, w, h = "thai2", 32, 24
    npix = w * h
    single = make(pkg, scenes, name, w, h, seed=13)
    single.render(3)
    want = single.film.direct_sums().reshape(h, w, 3)
    kw = dict(device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE) if kind == "device_group" else dict(stripe_rows=4, stripe_rank=1, stripe_world=2)
    rt = make(pkg, scenes, name, w, h, seed=13, **kw)
    rt.render(3)
    got = rt.film.direct_sums().reshape(h, w, 3)
    if kind == "device_group":
        assert np.array_equal(bits(got), bits(want))
    else:
        rows = rt.owned_rows()
        other = np.setdiff1d(np.arange(h), rows)
        assert len(rows) and len(other)
        assert np.array_equal(bits(got[rows]), bits(want[rows])) and not got[other].any()
        rt.film.clear()                                               # film_clear_rows_kernel clears the fourth plane too
        assert not rt.film.direct_sums().any()
        rt.render(3)
        assert np.array_equal(bits(rt.film.direct_sums().reshape(h, w, 3)[rows]), bits(want[rows]))
    rgb = np.full((npix, 3), 7.0, np.float32); packed = np.full(npix, 0x12345678, np.uint32)
    assert pkg.lib().mi355rt_get_denoised_pixels_split(rt._h, C.byref(pkg.denoise_config()), fptr(rgb), uptr(packed), npix) == -1
    msg = "device group" if kind == "device_group" else "striped"
    assert msg in last_error(pkg, rt)
    assert (rgb == 7.0).all() and (packed == 0x12345678).all()
    with pytest.raises(RuntimeError, match=msg):
        rt.get_denoised_pixels(split=True)


# ---- 7. it buys what the CPU evaluation says --------------------------------------------------------------------------------------------
def test_split_read_out_is_closer_to_the_converged_image(pkg, scenes):
    """thai2 160x120, film seed 5, against render(1024) of seed 99: RMSE of the tone-mapped means c / (1 + c), default config.  Orderings
    against the raw film and the plain denoised read-out of the SAME film, no thresholds; the CPU evaluation behind DESIGN.md §3e (a
    1024-spp oracle reference) gives 0.01752 / 0.01459 / 0.01193 (raw / plain / split) at 8 spp and 0.00661 / 0.00831 / 0.00539 at 64 spp:
    18 % or more between neighbours.  The test prints its values."""
    w, h = 160, 120
    ref = make(pkg, scenes, "thai2", w, h, seed=99, direct=False)
    ref.render(1024)
    truth = ref.film.get_pixels().astype(np.float64)
    ref.close()

    def rmse(x):
        x = np.asarray(x, np.float64)
        return float(np.sqrt(np.mean((x / (1 + x) - truth / (1 + truth)) ** 2)))
    rt = make(pkg, scenes, "thai2", w, h, seed=5)
    got = {}
    for spp, more in ((8, 8), (64, 56)):
        rt.render(more)
        assert int(rt.film.pixel_datas()[2].max()) == spp
        got[spp] = (rmse(rt.film.get_pixels()), rmse(rt.get_denoised_pixels(packed=False)[0]), rmse(rt.get_denoised_pixels(split=True, packed=False)[0]))
        print("tone-mapped rmse at %d spp: raw %.5f denoised %.5f split %.5f" % ((spp,) + got[spp]))
    raw, plain, split = got[8]
    assert split < plain < raw, got
    raw, plain, split = got[64]
    assert split < raw, got


# ---- 8. the CLI -------------------------------------------------------------------------------------------------------------------------
def read_png_rgb(data):
    """the pixels (uint8[npix, 3]) of an 8-bit RGB PNG whose scanlines all use filter type 0, as the CLI writes them"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            size = struct.unpack(">II", body[:8]); assert body[8:10] == b"\x08\x02"
        if kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h = size
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return (w, h), raw[:, 1:].reshape(-1, 3)


def test_cli_denoise_split_writes_the_library_read_out(pkg, scenes, tmp_path):
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    w, h = 64, 48
    out = tmp_path / "d.png"
    r = subprocess.run([exe, "-f", os.path.join(SCENES, "thai2.scene"), "--width", str(w), "--height", str(h), "--seed", "17",
                        "--spp", "4", "--denoise-split", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    size, rgb = read_png_rgb(out.read_bytes())
    assert size == (w, h)
    rt = make(pkg, scenes, "thai2", w, h, seed=17)
    rt.render(4)
    _, px = rt.get_denoised_pixels(split=True, rgb=False)
    want = np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8)
    assert np.array_equal(rgb, want)
    assert not np.array_equal(px, rt.get_denoised_pixels(rgb=False)[1])
