"""Bake on the device (include/mi355rt.h "BAKE"): UV charts to texels and surface points, per-point values back into an atlas.

The yardstick is the statement (raytracer_rs_amd.bake, numpy f32), which tests/test_bake_abi.py holds to exact rational coverage and to the header the kernels
compile.  Every comparison here is on the bits.  bake_texels must equal bake.texels, bake_atlas must equal bake.atlas, and RayTracer.bake must equal
bake.texels -> rt.gather -> bake.atlas (gather itself is held to its own statement by tests/test_gpu_gather.py).  The points and normals are tied to the scene
independently of the statement's own P: `direct` equals gather.direct over occluded_rays, and a short ray back along the normal finds the surface.  No test
feeds non-finite positions to the GPU: non-finite UVs cover nothing, so no point is made from them."""
import ctypes as C
import importlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bake_charts as bc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5
MISS = 0xFFFFFFFF
E_INVALID = -1
F = np.float32
LISTS = ("ids", "points", "normals", "albedo")
ALL = ("owner", "bary") + LISTS
GATHERED = ("n", "sum", "sumsq", "direct")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype != np.uint8 else np.ascontiguousarray(a)


@pytest.fixture(scope="module")
def bake(pkg):
    return importlib.import_module("raytracer_rs_amd.bake")


@pytest.fixture(scope="module")
def ga(pkg):
    return importlib.import_module("raytracer_rs_amd.gather")


def make(pkg, scene, w=16, h=16, **kw):
    kw.setdefault("seed", SEED)
    return pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, **kw)


def cut(scene, tris):
    """the scene with the listed triangles only"""
    sc = dict(scene)
    sc["tri_verts"] = np.ascontiguousarray(scene["tri_verts"][tris]); sc["tri_geom"] = np.ascontiguousarray(scene["tri_geom"][tris])
    return sc


@pytest.fixture(scope="module")
def handles(pkg, scenes):
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            base = scenes("4boxes")
            scene = {"two": lambda: cut(base, [0, 1]), "crowd": lambda: cut(base, [0] * 200)}.get(name, lambda: scenes(name))()
            made[key] = (make(pkg, scene, **kw), scene)
        return made[key]
    yield get
    for rt, _ in made.values():
        rt.close()


def same_texels(got, want, keys=ALL):
    assert got["ncovered"] == want["ncovered"]
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape)
        assert np.array_equal(bits(got[k]), bits(want[k])), k


# ---- 1. bake_texels against the statement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("4boxes", 64, 64), ("4boxes", 24, 40), ("ico2", 128, 128), ("ico3_tex", 96, 96)])
def test_texels_equal_the_statement_on_the_auto_atlas(bake, handles, name, w, h):
    rt, scene = handles(name)
    uv = bake.auto_atlas(scene["tri_geom"].size, w, h)
    want = bake.texels(uv, w, h, scene)
    got = rt.bake_texels(uv, w, h)
    same_texels(got, want)
    assert want["ncovered"] > scene["tri_geom"].size and set(want["owner"][want["ids"]]) == set(range(scene["tri_geom"].size))
    if name == "ico3_tex":
        assert len(np.unique(got["albedo"], axis=0)) > 4                       # the albedo comes through the texture
    # a selection of the outputs, and the count alone
    some = rt.bake_texels(uv, w, h, want=("ids", "normals"))
    same_texels(some, want, ("ids", "normals"))
    assert rt.bake_texels(uv, w, h, want=())["ncovered"] == want["ncovered"]
    flipped = rt.bake_texels(uv, w, h, flip=True)
    same_texels(flipped, bake.texels(uv, w, h, scene, flip=True))
    assert np.array_equal(bits(flipped["normals"]), bits(-got["normals"]))


@pytest.mark.parametrize("scene_name,name", [("two", n) for n in sorted(bc.charts(2))] + [("4boxes", n) for n in sorted(bc.charts(48))])
def test_texels_equal_the_statement_on_hand_made_charts(bake, handles, scene_name, name):
    rt, scene = handles(scene_name)
    uv, w, h = bc.charts(scene["tri_geom"].size)[name]
    same_texels(rt.bake_texels(uv, w, h), bake.texels(uv, w, h, scene))


def test_a_tile_with_200_triangles(pkg, bake, handles):
    """200 coincident triangles, 200 copies of one chart: one tile's list holds them all.  The handle is created with FLAG_TRUE_CLOSEST_HIT, which builds no
    octree: the reference's octree cannot separate coincident triangles and splits such a scene down to its last level on the host, for minutes (more than
    triangles_per_leaf of them in one place is all it takes).  bake_texels does not look at the intersector."""
    rt, scene = handles("crowd", flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    uv, w, h = bc.crowd(200)
    want = bake.texels(uv, w, h, scene)
    assert want["ncovered"] >= 6 and (want["owner"][want["ids"]] == 0).all()
    same_texels(rt.bake_texels(uv, w, h), want)
    # the same crowd with the first 150 charts moved off the atlas: triangle 150 wins
    uv2 = uv.copy(); uv2[:150] = np.asarray(bc.OFF, F)
    want2 = bake.texels(uv2, w, h, scene)
    assert (want2["owner"][want2["ids"]] == 150).all()
    same_texels(rt.bake_texels(uv2, w, h), want2)


def test_texels_on_device_tensors(bake, handles):
    import torch
    rt, scene = handles("4boxes")
    uv = bake.auto_atlas(48, 65, 9)
    want = bake.texels(uv, 65, 9, scene)
    dev = torch.device("cuda", 0)
    tuv = torch.from_numpy(uv.copy()).to(dev)
    got = rt.bake_texels(tuv, 65, 9)
    hbm = rt.hbm_allocated_bytes()
    got = rt.bake_texels(tuv, 65, 9)
    assert rt.hbm_allocated_bytes() == hbm
    for k in ALL:
        assert isinstance(got[k], torch.Tensor) and got[k].device == dev
        assert np.array_equal(bits(got[k].cpu().numpy()), bits(want[k])), k
    assert got["ncovered"] == want["ncovered"]
    assert np.array_equal(tuv.cpu().numpy().view(np.uint32), uv.view(np.uint32))        # read in place, not written
    with pytest.raises(ValueError, match="GPU"):
        rt.bake_texels(tuv.cpu(), 65, 9)
    with pytest.raises(ValueError, match="shape"):
        rt.bake_texels(uv[:47], 65, 9)
    with pytest.raises(TypeError, match="dtype"):
        rt.bake_texels(uv.astype(np.float64), 65, 9)


def raw_texels(pkg, rt, uv, w, h, want=ALL, where=0, count=True):
    """mi355rt_bake_texels through ctypes into sentinel-filled outputs; returns (code, arrays, ncovered)"""
    o, arrs = pkg.BakeTexelOutputs(), {}
    cols = {"owner": 1, "bary": 2, "ids": 1, "points": 3, "normals": 3, "albedo": 3}
    for k in want:
        arrs[k] = np.full(w * h * cols[k], 0xA5A5A5A5, np.uint32)
        setattr(o, k, arrs[k].ctypes.data)
    n = C.c_uint32(0xA5A5A5A5)
    code = pkg.lib().mi355rt_bake_texels(rt._h, None if uv is None else uv.ctypes.data, w, h, 0, where, C.byref(o), C.byref(n) if count else None)
    return code, arrs, n.value


def test_texels_write_what_they_say_and_refuse_the_rest(pkg, bake, handles, scenes):
    rt, scene = handles("4boxes")
    uv = bake.auto_atlas(48, 24, 40)
    want = bake.texels(uv, 24, 40, scene)
    code, arrs, n = raw_texels(pkg, rt, uv, 24, 40)
    assert code == 0 and n == want["ncovered"]
    cov = want["owner"] != MISS
    assert np.array_equal(arrs["owner"], want["owner"])
    assert np.array_equal(arrs["bary"].reshape(-1, 2)[cov], bits(want["bary"])[cov]) and (arrs["bary"].reshape(-1, 2)[~cov] == 0xA5A5A5A5).all()       # untouched where uncovered
    for k in LISTS:
        a = arrs[k].reshape(24 * 40, -1)
        assert np.array_equal(a[:n].reshape(want[k].shape), bits(want[k])) and (a[n:] == 0xA5A5A5A5).all(), k
    lib = pkg.lib()
    err = lambda h=rt: (lib.mi355rt_last_error(h._h) or b"").decode()

    def refused(result, *names):
        code, arrs, n = result
        assert code == E_INVALID and "mi355rt_bake_texels" in err() and all(nm in err() for nm in names), err()
        assert all(np.all(v == 0xA5A5A5A5) for v in arrs.values()) and n == 0xA5A5A5A5

    refused(raw_texels(pkg, rt, None, 24, 40), "uv")
    refused(raw_texels(pkg, rt, uv, 0, 40), "width")
    refused(raw_texels(pkg, rt, uv, 24, 16385), "height")
    refused(raw_texels(pkg, rt, uv, 24, 40, where=2), "where")
    refused(raw_texels(pkg, rt, uv, 24, 40, want=(), count=False), "out")
    assert lib.mi355rt_bake_texels(rt._h, uv.ctypes.data, 24, 40, 0, 0, None, None) == E_INVALID and "out" in err()
    n = C.c_uint32()
    assert lib.mi355rt_bake_texels(rt._h, uv.ctypes.data, 24, 40, 0, 0, None, C.byref(n)) == 0 and n.value == want["ncovered"]
    with pytest.raises(ValueError, match="want"):
        rt.bake_texels(uv, 24, 40, want=("rgb",))
    with pytest.raises(ValueError, match="width"):
        rt.bake_texels(uv, 0, 40)
    g = make(pkg, scenes("4boxes"), device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    code, arrs, n = raw_texels(pkg, g, uv, 24, 40)
    assert code == E_INVALID and "device group" in err(g) and "mi355rt_bake_texels" in err(g) and all(np.all(v == 0xA5A5A5A5) for v in arrs.values())
    atlas = np.full(24 * 40 * 3, 0xA5A5A5A5, np.uint32)
    assert lib.mi355rt_bake_atlas(g._h, want["ids"].ctypes.data, want["points"].ctypes.data, want["ncovered"], 24, 40, 2, 0, atlas.ctypes.data, None) == E_INVALID
    assert "device group" in err(g) and "mi355rt_bake_atlas" in err(g) and (atlas == 0xA5A5A5A5).all()
    g.close()


# ---- 2. bake_atlas against the statement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.masks()))
def test_atlas_equals_the_statement(bake, handles, name):
    import torch
    rt, _ = handles("4boxes")
    ids, values, w, h, dilate = bc.masks()[name]
    want = bake.atlas(ids, values, w, h, dilate)
    got = rt.bake_atlas(ids, values, w, h, dilate)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    # the order of the ids does not matter: descending, shuffled
    for order in (np.argsort(ids)[::-1], np.random.default_rng(3).permutation(ids.size)):
        got = rt.bake_atlas(np.ascontiguousarray(ids[order]), np.ascontiguousarray(values[order]), w, h, dilate)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    dev = torch.device("cuda", 0)
    hbm = rt.hbm_allocated_bytes()
    ta, tv = rt.bake_atlas(torch.from_numpy(ids.view(np.int32).copy()).to(dev), torch.from_numpy(values.copy()).to(dev), w, h, dilate)
    assert rt.hbm_allocated_bytes() == hbm
    assert ta.device == dev and np.array_equal(bits(ta.cpu().numpy()), bits(want[0])) and np.array_equal(tv.cpu().numpy(), want[1])


def test_atlas_refusals_write_nothing(pkg, handles):
    rt, _ = handles("4boxes")
    lib = pkg.lib()
    err = lambda: (lib.mi355rt_last_error(rt._h) or b"").decode()
    values = np.ones((4, 3), F)

    def call(ids, n, w=4, h=4, where=0, atlas=True, valid=True, vals=values):
        a = np.full(w * h * 3, 0xA5A5A5A5, np.uint32); v = np.full(w * h, 0xA5, np.uint8)
        code = lib.mi355rt_bake_atlas(rt._h, None if ids is None else ids.ctypes.data, None if vals is None else vals.ctypes.data, n, w, h, 2, where,
                                      a.ctypes.data if atlas else None, v.ctypes.data if valid else None)
        return code, a, v

    def refused(result, *names):
        code, a, v = result
        assert code == E_INVALID and "mi355rt_bake_atlas" in err() and all(nm in err() for nm in names), err()
        assert (a == 0xA5A5A5A5).all() and (v == 0xA5).all()

    refused(call(np.array([1, 5, 1, 7], np.uint32), 4), "twice")
    refused(call(np.array([1, 5, 16, 7], np.uint32), 4), ">= width * height")
    refused(call(np.array([1, 5, 0xFFFFFFFF, 7], np.uint32), 4), ">= width * height")
    refused(call(None, 4), "ids")
    refused(call(np.arange(4, dtype=np.uint32), 4, vals=None), "values3")
    refused(call(np.arange(4, dtype=np.uint32), 4, w=0), "width")
    refused(call(np.arange(4, dtype=np.uint32), 4, where=2), "where")
    refused(call(np.arange(4, dtype=np.uint32), 4, atlas=False, valid=False), "NULL")
    refused(call(np.zeros(17, np.uint32), 17, vals=np.ones((17, 3), F)), "twice")
    code, a, v = call(np.array([1, 5, 15, 7], np.uint32), 4, valid=False)         # one output is enough
    assert code == 0 and not (a == 0xA5A5A5A5).any() and (v == 0xA5).all()
    with pytest.raises(RuntimeError, match="twice"):
        rt.bake_atlas(np.array([3, 3], np.uint32), np.ones((2, 3), F), 4, 4)
    with pytest.raises(ValueError, match="shape"):
        rt.bake_atlas(np.array([3, 2, 1], np.uint32), np.ones((2, 3), F), 4, 4)


# ---- 3. RayTracer.bake against bake.texels -> rt.gather -> bake.atlas ---------------------------------------------------------------------------------------
_STATEMENT_TEXELS = {}


def texels_4boxes(bake, scenes):
    if "t" not in _STATEMENT_TEXELS:
        uv = bake.auto_atlas(48, 32, 32)
        _STATEMENT_TEXELS["t"] = (uv, bake.texels(uv, 32, 32, scenes("4boxes")))
    return _STATEMENT_TEXELS["t"]


def same_bake(bake, got, tex, g, dilate=2):
    same_texels(got["texels"], tex)
    for k in GATHERED:
        assert np.array_equal(bits(got["gather"][k]), bits(g[k])), k
    for name, val in (("direct", g["direct"]), ("indirect", bake.indirect(g)), ("radiance", bake.radiance(tex["albedo"], g["direct"], g))):
        want = bake.atlas(tex["ids"], val, 32, 32, dilate)
        assert np.array_equal(bits(got[name][0]), bits(want[0])) and np.array_equal(got[name][1], want[1]), name


@pytest.mark.parametrize("weight", ["mean", "cosine"])
def test_bake_equals_the_statement(bake, scenes, handles, sem3, weight):
    uv, tex = texels_4boxes(bake, scenes)
    rt, _ = handles("4boxes", flags=sem3.gpu)
    got = rt.bake(uv, 32, 32, spp=4, weight=weight)
    g = rt.gather(tex["points"], tex["normals"], tex["ids"], spp=4, weight=weight, want=GATHERED)
    same_bake(bake, got, tex, g)
    assert (got["gather"]["n"] == 4).all() and np.isfinite(got["radiance"][0]).all() and got["radiance"][0].any()
    assert (got["radiance"][1] == 1).sum() == tex["ncovered"] and (got["radiance"][1] > 1).any()


def test_bake_continues_bit_for_bit(bake, scenes, handles, sem3):
    uv, tex = texels_4boxes(bake, scenes)
    rt, _ = handles("4boxes", flags=sem3.gpu)
    a = rt.bake(uv, 32, 32, spp=3)
    b = rt.bake(uv, 32, 32, spp=5, first_sample=3, into=a)
    one = rt.bake(uv, 32, 32, spp=8)
    assert (b["gather"]["n"] == 8).all()
    for k in GATHERED:
        assert np.array_equal(bits(b["gather"][k]), bits(one["gather"][k])), k
    for name in ("direct", "indirect", "radiance"):
        assert np.array_equal(bits(b[name][0]), bits(one[name][0])) and np.array_equal(b[name][1], one[name][1]), name


def test_chunks_cut_the_texel_list(bake, scenes, handles, sem3, monkeypatch):
    uv, tex = texels_4boxes(bake, scenes)
    assert tex["ncovered"] * 4 > 1024 and tex["ncovered"] % 1024 != 0
    rt, _ = handles("4boxes", flags=sem3.gpu)
    one = rt.bake(uv, 32, 32, spp=4)
    monkeypatch.setenv("MI355RT_PASS_SAMPLES", "1024")
    cutup = rt.bake(uv, 32, 32, spp=4)
    for k in GATHERED:
        assert np.array_equal(bits(cutup["gather"][k]), bits(one["gather"][k])), k
    assert np.array_equal(bits(cutup["radiance"][0]), bits(one["radiance"][0]))


def test_a_striped_handle_bakes_what_an_unstriped_one_does(pkg, bake, scenes, handles):
    uv, tex = texels_4boxes(bake, scenes)
    rt, _ = handles("4boxes")
    striped = make(pkg, scenes("4boxes"), stripe_rows=2, stripe_rank=1, stripe_world=3)
    a, b = rt.bake(uv, 32, 32, spp=2), striped.bake(uv, 32, 32, spp=2)
    same_texels(b["texels"], a["texels"])
    for name in ("direct", "indirect", "radiance"):
        assert np.array_equal(bits(b[name][0]), bits(a[name][0])) and np.array_equal(b[name][1], a[name][1]), name
    striped.close()


def test_bake_on_device_tensors(bake, scenes, handles):
    import torch
    uv, tex = texels_4boxes(bake, scenes)
    rt, _ = handles("4boxes")
    host = rt.bake(uv, 32, 32, spp=2)
    got = rt.bake(torch.from_numpy(uv.copy()).to(torch.device("cuda", 0)), 32, 32, spp=2)
    for name in ("direct", "indirect", "radiance"):
        assert isinstance(got[name][0], torch.Tensor)
        assert np.array_equal(bits(got[name][0].cpu().numpy()), bits(host[name][0])) and np.array_equal(got[name][1].cpu().numpy(), host[name][1]), name


# ---- 4. the points and normals belong to the scene -----------------------------------------------------------------------------------------------------------
def test_direct_at_texel_centres_and_the_surface_under_them(pkg, bake, ga, scenes, sem3):
    scene = scenes("4boxes")
    rt = make(pkg, scene, flags=sem3.gpu)
    uv = bake.auto_atlas(48, 32, 32)
    t = rt.bake_texels(uv, 32, 32)
    lights = np.ascontiguousarray(scene["lights"], F)
    blocked = rt.occluded_rays(ga.shadow_rays(t["points"], lights))
    want = ga.direct(t["points"], t["normals"], lights, blocked)
    got = rt.bake(uv, 32, 32, spp=1, dilate=0)
    assert np.array_equal(bits(got["direct"][0][t["ids"]]), bits(want)) and want.any()
    assert not got["direct"][0][got["direct"][1] == 0].any()
    rt.close()
    # A short ray back along the normal finds the surface: (P + 0.001 N, -N) hits at t < 0.01.  The hit triangle's identity is NOT asserted: a texel centre on
    # the chart's hypotenuse side can give a point on the edge that the two coplanar triangles of a box face share, and which of the two the intersector
    # reports there is its own tie rule, not the bake's.
    tc = make(pkg, scene, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    rays = np.ascontiguousarray(np.concatenate([t["points"] + F(0.001) * t["normals"], -t["normals"]], axis=1), F)
    tuv, prim = tc.intersect_rays(rays)
    print("back rays: %d, hits %d, t in [%g, %g]" % (len(rays), (prim != MISS).sum(), tuv[:, 0].min(), tuv[:, 0].max()))
    assert (prim != MISS).all() and (tuv[:, 0] < 0.01).all() and (tuv[:, 0] > 0).all()
    tc.close()


# ---- 5. what a bake leaves alone -----------------------------------------------------------------------------------------------------------------------------
def test_an_untouched_handle(pkg, bake, scenes, sem3):
    uv = bake.auto_atlas(48, 32, 32)
    flags = sem3.gpu | pkg.FLAG_DIRECT_FILM | pkg.FLAG_LIGHT_FILMS
    rt = make(pkg, scenes("4boxes"), flags=flags)
    rt.set_lens("thin", radius=0.05, focus=4.0)
    rt.render(2)
    rt.features.render(1)
    film = lambda: [bits(a).copy() for a in rt.film.pixel_datas()] + [bits(rt.film.direct_sums()).copy(), bits(rt.light_films.get()).copy()] + [bits(a).copy() for a in rt.features.get().values()]
    before = film()
    row, cam, lens = rt.current_row, [a.copy() for a in rt.camera.matrices()], rt.lens.as_dict()
    counts = rt.last_counts().as_dict()
    hbm0 = rt.hbm_allocated_bytes()
    rt.bake_texels(uv, 32, 32, want=("owner", "ids", "normals", "albedo"))
    assert rt.hbm_allocated_bytes() == hbm0                                      # no points asked for: nothing is kept
    rt.bake_texels(uv, 32, 32)
    hbm1 = rt.hbm_allocated_bytes()
    assert hbm1 - hbm0 == 48 * 36                                                # the one-time scene-order copy of (A, B - A, C - A): 36 bytes per triangle
    rt.bake_texels(uv, 32, 32)
    ids = np.arange(50, dtype=np.uint32)
    rt.bake_atlas(ids, np.ones((50, 3), F), 32, 32, 3)
    assert rt.hbm_allocated_bytes() == hbm1
    assert rt.last_counts().as_dict() == counts                                  # neither call traces a ray or touches the counters
    rt.bake(uv, 32, 32, spp=2)
    hbm2 = rt.hbm_allocated_bytes()                                              # the gather inside may have grown the pass buffers once, as trace_rays does (§3m)
    rt.bake(uv, 32, 32, spp=2)
    assert rt.hbm_allocated_bytes() == hbm2 >= hbm1
    after = film()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert rt.current_row == row and rt.lens.as_dict() == lens
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(cam, rt.camera.matrices()))
    rt.get_denoised_pixels()                                                     # the caller-ray mark is not set
    twin = make(pkg, scenes("4boxes"), flags=flags)
    twin.set_lens("thin", radius=0.05, focus=4.0)
    twin.render(2); twin.render(1); rt.render(1)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(rt.film.pixel_datas()[:2], twin.film.pixel_datas()[:2]))
    rt.close(); twin.close()


def test_a_bake_behind_a_speculative_frame(pkg, bake, scenes):
    """trace_frame_additive leaves the next 50-row frame in flight; a bake settles it as every other read-out does, and the film goes on as if nothing happened"""
    uv = bake.auto_atlas(48, 32, 32)
    rt, twin = make(pkg, scenes("4boxes"), 64, 64), make(pkg, scenes("4boxes"), 64, 64)
    rt.trace_frame_additive(); twin.trace_frame_additive()
    got = rt.bake(uv, 32, 32, spp=1)
    same_texels(got["texels"], twin.bake_texels(uv, 32, 32))
    rt.trace_frame_additive(); twin.trace_frame_additive()
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(rt.film.pixel_datas(), twin.film.pixel_datas()))
    rt.close(); twin.close()


# ---- 6. the display mapping of an image that is no film, and the CLI -----------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
SCENE_4BOXES = os.path.join(ROOT, "tests", "golden", "scenes", "4boxes.scene")
PARENT_FRAME = os.path.join(ROOT, "tests", "golden", "cli_4boxes_64x48_seed17_spp2.ppm")


def read_png(path):
    """(width, height, uint8 (npix, 3)) of an 8-bit RGB PNG with one IDAT chunk and filter 0 on every scanline, as the CLI writes it"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        chunks[data[pos + 4:pos + 8]] = data[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, h, depth, colour = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (depth, colour) == (8, 2)
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return w, h, raw[:, 1:].reshape(-1, 3)


def rgb_of(px):
    return np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8)


def test_display_image_is_the_display_read_out_of_the_same_image(pkg, scenes):
    """mi355rt_display_image on the film's mean image packs what mi355rt_get_display_pixels packs from the film at the same exposure, and without a config what
    get_tonemapped_pixels packs; it keeps nothing on the handle and refuses auto-exposure."""
    rt = make(pkg, scenes("4boxes"), 40, 24)
    rt.render(3)
    s, _, n = rt.film.pixel_datas()
    mean = (s.reshape(-1, 3) * (np.float32(1) / n.astype(np.float32))[:, None]).astype(np.float32)       # display_source: sum * (1 / n)
    hbm = rt.hbm_allocated_bytes()
    assert np.array_equal(rt.display_image(mean), rt.get_tonemapped_pixels())
    assert rt.hbm_allocated_bytes() == hbm
    for cfg in (dict(exposure=2.0, curve=pkg.CURVE_ACES, transfer=pkg.TRANSFER_SRGB), dict(exposure=0.5, curve=pkg.CURVE_REINHARD_WHITE, white=2.0), dict(curve=pkg.CURVE_CLAMP)):
        assert np.array_equal(rt.display_image(mean, **cfg), rt.get_display_pixels(**cfg)[0]), cfg
    odd = np.linspace(0, 3, 7 * 3, dtype=np.float32).reshape(7, 3)                                        # any number of pixels, not the frame's
    assert rt.display_image(odd).shape == (7,) and (rt.display_image(odd) >> 24 == 255).all()
    with pytest.raises(RuntimeError, match="auto_exposure"):
        rt.display_image(mean, auto_exposure=1)
    with pytest.raises(RuntimeError, match="exposure"):
        rt.display_image(mean, exposure=-1.0)
    with pytest.raises(ValueError, match="shape"):
        rt.display_image(mean.reshape(-1))
    rt.close()


def test_cli_bake_writes_the_png_the_python_path_packs(pkg, bake, scenes, tmp_path):
    out, uvf = tmp_path / "lightmap.png", tmp_path / "uv.f32"
    base = [EXE, "-f", SCENE_4BOXES, "--seed", "17", "--spp", "4"]
    r = subprocess.run(base + ["--bake", "64,64", "--bake-uv-out", str(uvf), "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rt = make(pkg, scenes("4boxes"), 64, 48, seed=17)
    uv = bake.auto_atlas(48, 64, 64)
    assert np.array_equal(np.fromfile(uvf, "<f4").view(np.uint32), uv.reshape(-1).view(np.uint32))
    b = rt.bake(uv, 64, 64, spp=4)
    assert ("bake: 64 x 64 texels in cells of 12, %d covered, 4 samples each, 2 dilation steps" % b["texels"]["ncovered"]) in r.stdout and "display:" not in r.stdout
    w, h, px = read_png(out)
    assert (w, h) == (64, 64) and np.array_equal(px, rgb_of(rt.display_image(b["radiance"][0]))) and px.any()
    # the display options and the dilation count reach the atlas; a .ppm holds the same bytes
    ppm = tmp_path / "lightmap.ppm"
    r = subprocess.run(base + ["--bake", "24,40", "--bake-dilate", "5", "--srgb", "--curve", "aces", "--exposure", "2", "--out", str(ppm)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "display: exposure 2\n" in r.stdout, r.stderr
    b = rt.bake(bake.auto_atlas(48, 24, 40), 24, 40, spp=4, dilate=5)
    want = rgb_of(rt.display_image(b["radiance"][0], transfer=pkg.TRANSFER_SRGB, curve=pkg.CURVE_ACES, exposure=2.0))
    data = open(ppm, "rb").read()
    assert data.startswith(b"P6\n24 40\n255\n") and np.array_equal(np.frombuffer(data[len(b"P6\n24 40\n255\n"):], np.uint8).reshape(-1, 3), want)
    assert (b["radiance"][1] == 6).any()
    rt.close()
    # refusals, each with its message and no file
    none = tmp_path / "none.png"
    for extra, word in ((["--bake", "64,64", "--auto-exposure"], "--auto-exposure"), (["--bake", "64,64", "--denoise"], "excludes"), (["--bake", "64"], "W,H"),
                        (["--bake", "0,8"], "16384"), (["--bake", "8,8", "--gpus", "2"], "excludes"), (["--bake-uv-out", str(uvf)], "needs --bake"), (["--bake", "4,4"], "too small")):
        r = subprocess.run(base + extra + ["--out", str(none)], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and word in r.stderr and not none.exists(), (extra, r.stderr)
    r = subprocess.run([EXE, "-f", SCENE_4BOXES, "--bake", "8,8", "--out", str(none)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs --spp" in r.stderr and not none.exists()


def test_cli_without_bake_writes_the_parents_bytes(tmp_path):
    """tests/golden/cli_4boxes_64x48_seed17_spp2.ppm is the file the parent commit's bin/raytracer wrote for this command line on an MI355X"""
    out = tmp_path / "frame.ppm"
    r = subprocess.run([EXE, "-f", SCENE_4BOXES, "--width", "64", "--height", "48", "--seed", "17", "--spp", "2", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(PARENT_FRAME, "rb").read()
