"""The feature film without a GPU (include/mi355rt.h "FEATURE FILM"): the new entry points are exported, the constants agree with the
header, calls without a handle are rejected, the numpy statement (raytracer_rs_amd.features) does what the header says on hand-made planes, and the CLI
names its three options."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_features_render", "mi355rt_features_render_rays", "mi355rt_features_get", "mi355rt_features_clear", "mi355rt_features_alpha",
       "mi355rt_set_guide_source", "mi355rt_get_guide_source"]
F = np.float32
MISS = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ft(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.features")


def test_feature_symbols_are_exported(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)
        assert re.search(r"\b%s\(" % name, header), name


def test_feature_constants_match_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    for name, value in (("MI355RT_GUIDES_CENTRE", pkg.GUIDES_CENTRE), ("MI355RT_GUIDES_FEATURES", pkg.GUIDES_FEATURES)):
        m = re.search(r"#define\s+%s\s+(\d+)u" % name, header)
        assert m and int(m.group(1)) == value, name
    assert pkg.GUIDE_SOURCES == {"centre": 0, "features": 1}


def test_feature_calls_without_a_handle_are_rejected(pkg):
    L = pkg.lib()
    a = np.zeros(1, np.float32)
    assert L.mi355rt_features_render(None, 1) == -1
    assert L.mi355rt_features_render_rays(None, None, 0, 1, 0) == -1
    assert L.mi355rt_features_get(None, None, None, None, None, None, 0) == -1
    assert L.mi355rt_features_clear(None) == -1
    assert L.mi355rt_features_alpha(None, a.ctypes.data_as(C.POINTER(C.c_float)), 1) == -1
    assert L.mi355rt_set_guide_source(None, 0) == -1
    assert L.mi355rt_get_guide_source(None) == 0


# ---- the numpy statement on hand-made planes -------------------------------------------------------------------------------------------
def planes(n, hits, depth, normal, albedo):
    return dict(n=np.asarray(n, np.uint32), hits=np.asarray(hits, np.uint32), depth=np.asarray(depth, np.float32),
                normal=np.asarray(normal, np.float32).reshape(-1, 3), albedo=np.asarray(albedo, np.float32).reshape(-1, 3))


def test_guides_of_a_pixel_without_hits_are_a_miss(ft):
    # pixel 0: samples, none hit (its sums are zero, as the accumulation leaves them); pixel 1: no sample at all; even garbage sums do not leak out
    p = planes([4, 0, 3], [0, 0, 0], [0, 0, 7.5], [[0, 0, 0], [0, 0, 0], [1, 2, 3]], [[0, 0, 0], [0, 0, 0], [0.5, 0.5, 0.5]])
    g = ft.guides(p)
    assert g["prim"].dtype == np.uint32 and (g["prim"] == MISS).all()
    for k in ("depth", "normal", "albedo"):
        assert g[k].dtype == np.float32 and not bits(g[k]).any(), k             # +0.0, bit for bit


def test_guides_are_the_means_over_the_hits_not_over_the_samples(ft):
    # 3 of 8 samples hit: the divisor is 3
    p = planes([8], [3], [6.0], [[0.0, 0.0, 3.0]], [[0.3, 0.6, 0.9]])
    g = ft.guides(p)
    inv = F(1) / F(3)
    assert g["prim"][0] == 0
    assert bits(g["depth"])[0] == bits(F(6.0) * inv)
    assert np.array_equal(bits(g["albedo"][0]), bits(np.array([0.3, 0.6, 0.9], np.float32) * inv))
    m = F(3.0) * inv
    ln = np.sqrt((F(0) * F(0) + F(0) * F(0)) + m * m)
    assert np.array_equal(bits(g["normal"][0]), bits(np.array([F(0) / ln, F(0) / ln, m / ln], np.float32)))
    assert bits(ft.alpha(p))[0] == bits(F(3) / F(8))


def test_opposite_normals_give_a_zero_normal_not_a_nan(ft):
    p = planes([2], [2], [4.0], [[0.0, 0.0, 0.0]], [[1.0, 1.0, 1.0]])           # (0, 0, 1) + (0, 0, -1)
    g = ft.guides(p)
    assert g["prim"][0] == 0 and not bits(g["normal"]).any()
    assert bits(g["depth"])[0] == bits(F(4.0) * (F(1) / F(2)))


def test_a_denormal_depth_sum_stays_a_denormal(ft):
    tiny = np.float32(np.frombuffer(np.uint32(3).tobytes(), np.float32)[0])      # 3 * 2^-149
    p = planes([2], [2], [tiny], [[0, 0, 2]], [[0, 0, 0]])
    g = ft.guides(p)
    want = tiny * (F(1) / F(2))                                                   # 1.5 * 2^-149 rounds to even: 2 * 2^-149
    assert bits(g["depth"])[0] == bits(want) == 2
    assert np.array_equal(g["normal"][0], np.array([0, 0, 1], np.float32))


def test_alpha_is_hits_over_n_and_zero_without_samples(ft):
    p = planes([0, 5, 5, 7], [0, 0, 5, 3], [0] * 4, np.zeros((4, 3)), np.zeros((4, 3)))
    a = ft.alpha(p)
    assert a.dtype == np.float32
    assert np.array_equal(bits(a), bits(np.array([0.0, 0.0, 1.0, F(3) / F(7)], np.float32)))


def test_accumulate_adds_hits_in_sample_order_and_nothing_on_a_miss(ft):
    # one triangle per material: 0 is plain grey, 1 is textured (2 x 2 texels)
    tex = np.arange(12, dtype=np.float32).reshape(2, 2, 3) / F(16)
    scene = dict(tri_verts=np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1, 0, 2, 1, 2, 0, 1]], np.float32), tri_geom=np.array([0, 1], np.uint32),
                 mat_kind=np.array([0, 1]), mat_tex=np.array([0, 0]), mat_rgb=np.array([[0.25, 0.5, 0.75], [9, 9, 9]], np.float32), textures=[tex])
    npix, spp = 3, 3
    prim = np.full((spp, npix), MISS, np.uint32); tuv = np.full((spp, npix, 3), np.nan, np.float32)      # a miss's tuv is never read
    prim[0, 0] = 0; tuv[0, 0] = (1.5, 0.1, 0.2)
    prim[2, 0] = 1; tuv[2, 0] = (0.1, 0.75, 0.25)                                   # texel (x 1, y 0)
    prim[1, 1] = 0; tuv[1, 1] = (1e-3, 0.0, 0.0)
    start = ft.empty(npix)
    start["depth"][2] = F(-0.0)                                                    # a miss adds nothing, not even +0.0: the sign survives
    out = ft.accumulate(start, tuv.reshape(-1, 3), prim.reshape(-1), scene, spp)
    assert not bits(start["depth"])[:2].any() and start["n"].sum() == 0          # the input planes are left alone
    assert out["n"].tolist() == [3, 3, 3] and out["hits"].tolist() == [2, 1, 0]
    assert bits(out["depth"])[2] == 0x80000000
    assert bits(out["depth"])[0] == bits((F(0) + F(1.5)) + F(0.1)) and bits(out["depth"])[1] == bits(F(0) + F(1e-3))
    assert np.array_equal(out["normal"][0], np.array([0, 0, 1], np.float32) + np.array([0, 0, -1], np.float32))
    assert np.array_equal(bits(out["albedo"][0]), bits((np.zeros(3, np.float32) + np.array([0.25, 0.5, 0.75], np.float32)) + tex[0, 1]))
    assert np.array_equal(out["albedo"][1], np.array([0.25, 0.5, 0.75], np.float32))
    # a second call numbers on: n counts up, the sums keep their left operand
    again = ft.accumulate(out, tuv.reshape(-1, 3), prim.reshape(-1), scene, spp)
    assert again["n"].tolist() == [6, 6, 6] and again["hits"].tolist() == [4, 2, 0]
    assert bits(again["depth"])[0] == bits((out["depth"][0] + F(1.5)) + F(0.1))
    # rows a striped handle does not own stay as they are
    own = np.array([True, False, True])
    part = ft.accumulate(ft.empty(npix), tuv.reshape(-1, 3), prim.reshape(-1), scene, spp, owned=own)
    assert part["n"].tolist() == [3, 0, 3] and part["hits"].tolist() == [2, 0, 0] and not bits(part["albedo"][1]).any()


def test_cli_help_names_the_feature_options():
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True).stdout
    for opt in ("--features N", "--denoise-guides centre|features", "--alpha"):
        assert opt in out, opt
    assert "PREMULTIPLIED" in out
