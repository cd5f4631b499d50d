"""The denoised read-out on the device (include/mi355rt.h): the guide buffers equal the CPU oracle's primary hits bit for bit
in every intersector semantics and follow the camera; the filtered image equals its numpy statement (raytracer_rs_amd.denoise) bit for bit
on films of every kind; the read-out changes nothing; errors, memory, the image quality it buys and the CLI."""
import ctypes as C
import os
import subprocess

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


def make(pkg, scenes, name, w, h, **kw):
    return pkg.create_raytracer_from_arrays(scenes(name), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, **kw)


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


def assert_guides_equal(got, want):
    assert np.array_equal(got["prim"], want["prim"])
    for k in ("depth", "normal", "albedo"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k


# ---- 1. guides equal the oracle, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("ico2", 100, 37), ("thai2", 100, 37), ("ico3_tex", 64, 53)])
def test_guides_equal_the_oracle(pkg, scenes, oracle, sem3, name, w, h):
    sc = scenes(name)
    brute = bool(sem3.orc & oracle.FLAG_BRUTE_FORCE)
    rt = make(pkg, scenes, name, w, h, seed=3, flags=sem3.gpu)
    orc = oracle.Oracle(sc, w, h, seed=3, flags=sem3.orc)
    g0 = rt.guides()
    assert_guides_equal(g0, oracle_guides(orc, sc, w, h, False, brute))
    assert (g0["prim"] != MISS).any() and (g0["prim"] == MISS).any()
    if name == "ico3_tex":
        assert len(np.unique(g0["albedo"][g0["prim"] != MISS], axis=0)) > 10          # the texture is looked up
    rt.set_flags(sem3.gpu | pkg.FLAG_FIX_ROW_INDEX)
    assert_guides_equal(rt.guides(), oracle_guides(orc, sc, w, h, True, brute))
    # the cache follows the camera
    rt.camera.move_rel(0.3, -0.2, 0.5); orc.camera_move_rel(0.3, -0.2, 0.5)
    rt.camera.add_x_angle(0.07); orc.camera_add_x_angle(0.07)
    rt.camera.add_y_angle(-0.11); orc.camera_add_y_angle(-0.11)
    moved = rt.guides()
    assert not np.array_equal(moved["prim"], g0["prim"])
    assert_guides_equal(moved, oracle_guides(orc, sc, w, h, True, brute))
    rt.set_flags(sem3.gpu)
    assert_guides_equal(rt.guides(), oracle_guides(orc, sc, w, h, False, brute))
    before = rt.guides()
    rt.set_seed(99)
    assert_guides_equal(rt.guides(), before)


# ---- 2. the filter equals its numpy statement --------------------------------------------------------------------------------------
PARAMS = [dict(normal_power_log2=7, sigma_luminance=1.0, sigma_depth=0.1, sigma_albedo=0.1),
          dict(normal_power_log2=0, sigma_luminance=0.5, sigma_depth=1.0, sigma_albedo=2.0),
          dict(normal_power_log2=10, sigma_luminance=40.0, sigma_depth=0.01, sigma_albedo=0.02)]


def check_filter(rt, dn, guides, iterations=range(7), params=PARAMS):
    s, q, n = rt.film.pixel_datas()
    for prm in params:
        for it in iterations:
            got_rgb, got_packed = rt.get_denoised_pixels(iterations=it, **prm)
            want_rgb, want_packed = dn.denoise(s, q, n, guides, rt.width, rt.height, iterations=it, **prm)
            assert np.array_equal(bits(got_rgb), bits(want_rgb)), (prm, it)
            assert np.array_equal(got_packed, want_packed), (prm, it)
            _, only_packed = rt.get_denoised_pixels(rgb=False, iterations=it, **prm)
            only_rgb, _ = rt.get_denoised_pixels(packed=False, iterations=it, **prm)
            assert np.array_equal(only_packed, want_packed) and np.array_equal(bits(only_rgb), bits(want_rgb))


def test_filter_equals_numpy_on_a_uniform_render(pkg, scenes, oracle, dn):
    name, w, h = "thai2", 60, 45
    rt = make(pkg, scenes, name, w, h, seed=5)
    rt.render(8)
    g = oracle_guides(oracle.Oracle(scenes(name), w, h, seed=5), scenes(name), w, h, False, False)
    check_filter(rt, dn, g)
    # iterations = 0 is exactly get_pixels / get_tonemapped_pixels
    rgb, packed = rt.get_denoised_pixels(iterations=0)
    assert np.array_equal(bits(rgb), bits(rt.film.get_pixels())) and np.array_equal(packed, rt.get_tonemapped_pixels())


def test_filter_equals_numpy_on_an_adaptive_film(pkg, scenes, oracle, dn):
    name, w, h = "ico3_tex", 48, 40
    rt = make(pkg, scenes, name, w, h, seed=6, flags=pkg.FLAG_FIX_ROW_INDEX)
    rt.render_adaptive(min_spp=2, max_spp=12, batch_spp=2, rel_error=0.1, abs_floor=0.05)
    n = rt.film.pixel_datas()[2]
    assert len(np.unique(n)) > 1                                   # pixels with unequal n
    g = oracle_guides(oracle.Oracle(scenes(name), w, h, seed=6, flags=oracle.FLAG_FIX_ROW_INDEX), scenes(name), w, h, True, False)
    check_filter(rt, dn, g, iterations=(0, 1, 3, 5), params=PARAMS[:2])


def test_filter_equals_numpy_on_a_drop_in_film(pkg, scenes, oracle, dn, sem):
    """a few 50-row calls: empty rows (n == 0) beside rows of one sample (unknown variance), then rows of one beside rows of two"""
    name, w, h = "thai2", 40, 160
    rt = make(pkg, scenes, name, w, h, seed=7, flags=sem.gpu)
    g = oracle_guides(oracle.Oracle(scenes(name), w, h, seed=7, flags=sem.orc), scenes(name), w, h, False,
                      bool(sem.orc & oracle.FLAG_BRUTE_FORCE))
    for want in ({0, 1}, {1, 2}):
        for _ in range(2):
            rt.trace_frame_additive()
        n = rt.film.pixel_datas()[2]
        assert set(np.unique(n).tolist()) == want
        check_filter(rt, dn, g, iterations=(0, 1, 2, 4, 6), params=PARAMS[:2])
        rgb, packed = rt.get_denoised_pixels()
        assert np.isnan(rgb[n == 0]).all() and (packed[n == 0] == 0xFFFFFFFF).all()
        assert np.isfinite(rgb[n != 0]).all()


def test_device_guides_feed_the_same_filter(pkg, scenes, dn):
    rt = make(pkg, scenes, "ico2", 33, 29, seed=8, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    rt.render(3)
    s, q, n = rt.film.pixel_datas()
    rgb, packed = rt.get_denoised_pixels(iterations=4)
    want_rgb, want_packed = dn.denoise(s, q, n, rt.guides(), 33, 29, iterations=4, **PARAMS[0])
    assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(packed, want_packed)


# ---- 3. no side effects --------------------------------------------------------------------------------------------------------------
def test_denoise_leaves_the_film_and_the_read_outs(pkg, scenes):
    rt = make(pkg, scenes, "thai2", 64, 48, seed=9)
    rt.render(4)
    film0 = [np.asarray(x).copy() for x in rt.film.pixel_datas()]
    ldr0 = rt.get_tonemapped_pixels().copy()
    rt.get_denoised_pixels()
    rt.guides()
    for x, y in zip(film0, rt.film.pixel_datas()):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    assert np.array_equal(ldr0, rt.get_tonemapped_pixels())


def test_drop_in_speculation_is_settled(pkg, scenes, oracle):
    name, w, h = "thai2", 64, 160
    rt = make(pkg, scenes, name, w, h, seed=10)
    orc = oracle.Oracle(scenes(name), w, h, seed=10)
    rt.trace_frame_additive()
    launched0, _ = rt.debug_speculation()
    rt.get_denoised_pixels()
    rt.trace_frame_additive()
    orc.trace_frame_additive(); orc.trace_frame_additive()
    assert launched0 >= 1                                             # a speculative frame was out when the read-out came
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
    assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())


def test_memory_is_allocated_on_first_use_only(pkg, scenes, monkeypatch):
    monkeypatch.setenv("MI355RT_DEBUG_GUARD", "1")
    w, h = 100, 37
    rt = make(pkg, scenes, "thai2", w, h, seed=11)
    rt.render(4)
    rt.film.get_pixels(); rt.get_tonemapped_pixels()
    hbm0 = rt.hbm_allocated_bytes()
    rt.render(4); rt.film.get_pixels(); rt.get_tonemapped_pixels()
    assert rt.hbm_allocated_bytes() == hbm0
    rt.guides()
    assert rt.hbm_allocated_bytes() - hbm0 == 32 * w * h                # the guides
    rt.get_denoised_pixels()
    assert rt.hbm_allocated_bytes() - hbm0 == (32 + 52) * w * h         # + the filter's buffers
    rt.camera.move_rel(0.1, 0.0, 0.0)
    rt.get_denoised_pixels(iterations=7); rt.get_denoised_pixels(rgb=False); rt.guides()
    assert rt.hbm_allocated_bytes() - hbm0 == (32 + 52) * w * h
    assert rt.debug_check_guards() == 0


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------------
def call_raw(pkg, rt, cfg, rgb, packed, npix):
    return pkg.lib().mi355rt_get_denoised_pixels(rt._h, C.byref(cfg), None if rgb is None else rgb.ctypes.data_as(C.POINTER(C.c_float)),
                                                 None if packed is None else packed.ctypes.data_as(C.POINTER(C.c_uint32)), npix)


def last_error(pkg, rt):
    return pkg.lib().mi355rt_last_error(rt._h).decode()


def test_invalid_calls_are_rejected_and_write_nothing(pkg, scenes):
    w, h = 32, 24
    rt = make(pkg, scenes, "ico2", w, h, seed=12)
    rt.render(2)
    npix = w * h
    bad = [("iterations", dict(iterations=11)), ("normal_power_log2", dict(normal_power_log2=11)),
           ("sigma_luminance", dict(sigma_luminance=0.0)), ("sigma_luminance", dict(sigma_luminance=float("nan"))),
           ("sigma_depth", dict(sigma_depth=-1.0)), ("sigma_depth", dict(sigma_depth=float("inf"))),
           ("sigma_albedo", dict(sigma_albedo=0.0)), ("sigma_albedo", dict(sigma_albedo=float("-inf")))]
    rgb = np.full((npix, 3), 7.0, np.float32); packed = np.full(npix, 0x12345678, np.uint32)
    for field, kw in bad:
        assert call_raw(pkg, rt, pkg.denoise_config(**kw), rgb, packed, npix) == -1
        assert field in last_error(pkg, rt)
        with pytest.raises(RuntimeError, match=field):
            rt.get_denoised_pixels(**kw)
    assert call_raw(pkg, rt, pkg.denoise_config(), rgb, packed, npix - 1) == -1                 # short npix
    assert "npix" in last_error(pkg, rt)
    assert call_raw(pkg, rt, pkg.denoise_config(), None, None, npix) == -1                      # both outputs NULL
    assert "both NULL" in last_error(pkg, rt)
    assert pkg.lib().mi355rt_get_denoised_pixels(rt._h, None, rgb.ctypes.data_as(C.POINTER(C.c_float)), None, npix) == -1
    assert "null config" in last_error(pkg, rt)
    d = np.full(npix, 7.0, np.float32)
    assert pkg.lib().mi355rt_get_guides(rt._h, d.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, npix - 1) == -1
    assert (rgb == 7.0).all() and (packed == 0x12345678).all() and (d == 7.0).all()


@pytest.mark.parametrize("kind", ["device_group", "striped"])
def test_groups_and_stripes_are_rejected(pkg, scenes, kind):
    w, h = 32, 24
    kw = dict(device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE) if kind == "device_group" else dict(stripe_rows=4, stripe_rank=0, stripe_world=2)
    rt = make(pkg, scenes, "ico2", w, h, seed=13, **kw)
    rt.render(2)
    npix = w * h
    rgb = np.full((npix, 3), 7.0, np.float32); packed = np.full(npix, 0x12345678, np.uint32)
    assert call_raw(pkg, rt, pkg.denoise_config(), rgb, packed, npix) == -1
    msg = "device group" if kind == "device_group" else "striped"
    assert msg in last_error(pkg, rt)
    d = np.full(npix, 7.0, np.float32)
    assert pkg.lib().mi355rt_get_guides(rt._h, d.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, npix) == -1
    assert (rgb == 7.0).all() and (packed == 0x12345678).all() and (d == 7.0).all()
    with pytest.raises(RuntimeError, match=msg):
        rt.get_denoised_pixels()


# ---- 5. it denoises -----------------------------------------------------------------------------------------------------------------
def test_denoised_image_is_closer_to_the_converged_one(pkg, scenes):
    """thai2 160x120, 8 spp, against a 512-spp render of another seed: RMSE of the tone-mapped means c / (1 + c), default config.
    Measured on an MI355X: raw 0.01766, denoised 0.01439 (ratio 0.815; the frames are deterministic); the test asks for a ratio below 0.9.
    The gain is far smaller than at 1080p: these pixels are 12 times wider, so neighbours differ in true value."""
    w, h = 160, 120
    ref = make(pkg, scenes, "thai2", w, h, seed=77)
    for _ in range(8):
        ref.render(64)
    truth = ref.film.get_pixels().astype(np.float64)
    ref.close()
    rt = make(pkg, scenes, "thai2", w, h, seed=1)
    rt.render(8)
    raw = rt.film.get_pixels().astype(np.float64)
    den, _ = rt.get_denoised_pixels(packed=False)

    def rmse(x):
        return float(np.sqrt(np.mean((x / (1 + x) - truth / (1 + truth)) ** 2)))
    e_raw, e_den = rmse(raw), rmse(den.astype(np.float64))
    print("denoise rmse raw %.5f denoised %.5f ratio %.3f" % (e_raw, e_den, e_den / e_raw))
    assert e_den < LIMIT * e_raw, (e_raw, e_den)


LIMIT = 0.9


# ---- 6. the CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_denoise_writes_the_library_read_out(pkg, scenes, tmp_path):
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    w, h = 48, 40
    out = tmp_path / "d.ppm"
    r = subprocess.run([exe, "-f", os.path.join(SCENES, "thai2.scene"), "--width", str(w), "--height", str(h), "--seed", "17",
                        "--spp", "8", "--denoise", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    data = out.read_bytes()
    hdr = ("P6\n%d %d\n255\n" % (w, h)).encode()
    assert data.startswith(hdr)
    rgb = np.frombuffer(data[len(hdr):], np.uint8).reshape(-1, 3)
    rt = make(pkg, scenes, "thai2", w, h, seed=17)
    rt.render(8)
    _, px = rt.get_denoised_pixels(rgb=False)
    want = np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8)
    assert np.array_equal(rgb, want)
    assert not np.array_equal(px, rt.get_tonemapped_pixels())
