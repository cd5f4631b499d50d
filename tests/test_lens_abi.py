"""Lens models without a device (include/mi355rt.h, "lens models"): the symbols and the layout of mi355rt_lens, and mi355rt_lens_ray — HOST
code, the same expressions the kernels compile — against the numpy statement raytracer_rs_amd.cameras, bit for bit.  The generators of cameras.py take their
jitter and lens sample from pcg4d themselves; to feed mi355rt_lens_ray the same four numbers they are recomputed here with the helpers cameras.py exports.
The comparison needs csrc/capi.cpp built with -ffp-contract=off: where the host compiler may contract dir_x * rot[k] + ... into fused multiply-adds (any
target with FMA instructions: tried with -ffp-contract=fast -mfma) the bits differ and 8 of these tests fail.  (A plain x86-64 build has no FMA instruction to
contract into, so there the flag only states the intent.)"""
import ctypes as C
import importlib

import numpy as np
import pytest

SEED = 5
E_INVALID = -1
SYMBOLS = ("mi355rt_lens_default", "mi355rt_set_lens", "mi355rt_get_lens", "mi355rt_lens_ray", "mi355rt_lens_rays")


@pytest.fixture(scope="module")
def cams(pkg):
    return importlib.import_module("raytracer_rs_amd.cameras")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_symbols_and_layout(pkg):
    lib = pkg.lib()
    names = [n for n, _, _ in pkg.ABI]
    for s in SYMBOLS:
        assert s in names and getattr(lib, s)
    assert (pkg.LENS_PINHOLE, pkg.LENS_THIN, pkg.LENS_ORTHO) == (0, 1, 2)         # MI355RT_LENS_*
    assert C.sizeof(pkg.Lens) == 16
    assert [getattr(pkg.Lens, f).offset for f in ("model", "radius", "focus", "width_world")] == [0, 4, 8, 12]
    raw = (C.c_uint32 * 4)(*([0xA5A5A5A5] * 4))
    lib.mi355rt_lens_default(C.cast(raw, C.POINTER(pkg.Lens)))
    assert list(raw) == [0, 0, int(np.float32(1.0).view(np.uint32)), 0]            # PINHOLE, radius 0, focus 1, width_world 0
    lib.mi355rt_lens_default(None)                                                  # a NULL pointer is ignored
    l = pkg.make_lens("thin", radius=0.25, focus=3.0)
    assert (l.model, l.radius, l.focus, l.width_world) == (1, 0.25, 3.0, 0.0)
    assert pkg.make_lens("ortho", width_world=9.5).as_dict() == dict(model="ortho", radius=0.0, focus=1.0, width_world=9.5)


def lens_ray_all(pkg, cam, w, h, flags, lens, words):
    """mi355rt_lens_ray for every (sample, pixel) of the hash words (arrays [spp, npix]) -> float32 [(spp * npix), 6]"""
    lib = pkg.lib()
    rot, orient, mx = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in cam)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u = [np.ascontiguousarray(x, np.float32) for x in words]
    spp, npix = u[0].shape
    out = np.zeros((spp * npix, 6), np.float32)
    one = np.zeros(6, np.float32)
    for s in range(spp):
        for p in range(npix):
            assert lib.mi355rt_lens_ray(fp(rot), fp(orient), fp(mx), w, h, flags, C.byref(lens), p, u[0][s, p], u[1][s, p], u[2][s, p], u[3][s, p], fp(one)) == 0
            out[s * npix + p] = one
    return out


@pytest.mark.parametrize("w,h", [(37, 21), (5, 3)])
@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("moved", [False, True])
def test_lens_ray_equals_cameras_py(pkg, cams, oracle, scenes, w, h, fix, moved):
    spp, npix = 3, w * h
    orc = oracle.Oracle(scenes("thai2"), w, h, seed=SEED, flags=oracle.FLAG_FIX_ROW_INDEX if fix else 0)
    if moved:
        orc.camera_move_rel(0.3, -0.2, 0.5); orc.camera_add_y_angle(0.2); orc.camera_add_x_angle(-0.1)
    cam = orc.camera_matrices()
    orc.close()
    film_n = np.random.default_rng(w * 100 + h).integers(0, 6, npix).astype(np.uint32)       # non-uniform: sample s of pixel p is number film_n[p] + s
    assert len(np.unique(film_n)) > 1
    pixel = np.arange(npix, dtype=np.uint32)[None, :]
    sampleno = film_n[None, :] + np.arange(spp, dtype=np.uint32)[:, None]
    words = [cams.u01(x) for x in cams.pcg4d(pixel, sampleno, np.uint32(0), np.uint32(SEED))]
    cases = [(pkg.make_lens("pinhole"), cams.pinhole(cam, w, h, spp, SEED, film_n=film_n, flags=fix)),
             (pkg.make_lens("thin", radius=0.1, focus=5.0), cams.thin_lens(cam, w, h, spp, SEED, 0.1, 5.0, film_n=film_n, flags=fix)),
             (pkg.make_lens("thin", radius=0.0, focus=1.0), cams.pinhole(cam, w, h, spp, SEED, film_n=film_n, flags=fix)),
             (pkg.make_lens("ortho", width_world=9.5), cams.orthographic(cam, w, h, spp, SEED, 9.5, film_n=film_n))]
    for lens, want in cases:
        got = lens_ray_all(pkg, cam, w, h, fix, lens, words)
        assert np.array_equal(bits(got), bits(want)), lens.as_dict()
    # the generators differ from each other: the comparison above could not pass by accident
    assert not np.array_equal(bits(cases[0][1]), bits(cases[1][1])) and not np.array_equal(bits(cases[0][1]), bits(cases[3][1]))
    # the module-level wrapper, and its default: the guide ray
    g = pkg.lens_ray(cam, w, h, cases[1][0], npix - 1, flags=fix)
    half = [np.full((1, npix), 0.5, np.float32)] * 4
    assert np.array_equal(bits(g), bits(lens_ray_all(pkg, cam, w, h, fix, cases[1][0], half)[npix - 1]))


def test_lens_ray_argument_errors(pkg, cams, oracle, scenes):
    lib = pkg.lib()
    w, h = 5, 3
    orc = oracle.Oracle(scenes("ico2"), w, h, seed=SEED)
    rot, orient, mx = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in orc.camera_matrices())
    orc.close()
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    err = lambda: (lib.mi355rt_last_error(None) or b"").decode()
    ray = np.full(6, 0xA5A5A5A5, np.uint32).view(np.float32)

    def call(lens, r=rot, o=orient, m=mx, out=ray, pixel=0, width=w, height=h):
        return lib.mi355rt_lens_ray(fp(r), fp(o), fp(m), width, height, 0, None if lens is None else C.byref(lens), pixel, 0.5, 0.5, 0.5, 0.5, fp(out))

    def refused(code, *names):
        assert code == E_INVALID
        assert all(nm in err() for nm in names), err()
        assert np.all(ray.view(np.uint32) == 0xA5A5A5A5)

    nan, inf = float("nan"), float("inf")
    refused(call(pkg.make_lens(3)), "model")
    refused(call(pkg.make_lens(0xFFFFFFFF)), "model")
    refused(call(pkg.make_lens("thin", radius=-0.5, focus=1.0)), "radius")
    refused(call(pkg.make_lens("thin", radius=nan, focus=1.0)), "radius")
    refused(call(pkg.make_lens("thin", radius=inf, focus=1.0)), "radius")
    refused(call(pkg.make_lens("thin", radius=0.1, focus=0.0)), "focus")
    refused(call(pkg.make_lens("thin", radius=0.1, focus=-2.0)), "focus")
    refused(call(pkg.make_lens("thin", radius=0.1, focus=inf)), "focus")
    refused(call(pkg.make_lens("thin", radius=0.1, focus=nan)), "focus")
    refused(call(pkg.make_lens("ortho", width_world=0.0)), "width_world")
    refused(call(pkg.make_lens("ortho", width_world=-9.5)), "width_world")
    refused(call(pkg.make_lens("ortho", width_world=nan)), "width_world")
    refused(call(pkg.make_lens("ortho", width_world=inf)), "width_world")
    ok = pkg.make_lens("thin", radius=0.1, focus=5.0)
    refused(call(None), "lens")
    refused(call(ok, r=None), "rot16")
    refused(call(ok, o=None), "orient16")
    refused(call(ok, m=None), "max_xy")
    assert call(ok, out=None) == E_INVALID and "ray6" in err()
    refused(call(ok, pixel=w * h), "pixel")
    refused(call(ok, width=0), "width")
    # only the fields the model reads are checked
    assert call(pkg.make_lens("pinhole", radius=nan, focus=-1.0, width_world=nan)) == 0
    assert call(pkg.make_lens("thin", radius=0.1, focus=5.0, width_world=nan)) == 0
    assert call(pkg.make_lens("ortho", radius=nan, focus=nan, width_world=9.5)) == 0
    assert np.all(np.isfinite(ray))
    with pytest.raises(RuntimeError, match="radius"):
        pkg.lens_ray((rot, orient, mx), w, h, pkg.make_lens("thin", radius=-1.0), 0)
