"""Bake without a GPU (include/mi355rt.h "BAKE"): the entry points and the struct are what the header says; the host side of the shared
per-texel arithmetic (mi355rt_bake_texel, mi355rt_bake_point, mi355rt_bake_dilate_texel: csrc/bake_raster.hpp, the header the kernels of csrc/bake.hip
compile) equals the numpy statement (raytracer_rs_amd.bake) bit for bit; the auto atlas equals its statement and keeps its three properties; the
dilation does what its text says on hand-made masks; and the statement's coverage agrees with exact rational coverage on jittered meshes, in both
directions, with no exception.  tests/test_gpu_bake.py runs the kernels against the same statement on the same charts."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import bake_charts as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_bake_texels", "mi355rt_bake_atlas", "mi355rt_bake_texel", "mi355rt_bake_point", "mi355rt_bake_dilate_texel", "mi355rt_bake_auto_atlas", "mi355rt_display_image"]
F = np.float32
MISS = 0xFFFFFFFF
E_INVALID = -1
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def bake(pkg):
    return importlib.import_module("raytracer_rs_amd.bake")


def c_owners(pkg, uv, w, h):
    """owner and bary from one mi355rt_bake_texel call per (triangle, texel), the lowest index kept"""
    L = pkg.lib()
    owner = np.full(w * h, MISS, np.uint32); bary = np.zeros((w * h, 2), F)
    for i in range(uv.shape[0]):
        tri = np.ascontiguousarray(uv[i].reshape(6))
        for y in range(h):
            for x in range(w):
                if owner[y * w + x] != MISS:
                    continue
                cov = C.c_uint32(9); b = np.full(2, 7.0, F)
                assert L.mi355rt_bake_texel(fp(tri), w, h, x, y, C.byref(cov), fp(b)) == 0
                assert cov.value in (0, 1)
                if cov.value:
                    owner[y * w + x] = i; bary[y * w + x] = b
                else:
                    assert np.array_equal(b, np.full(2, 7.0, F))          # untouched where uncovered
    return owner, bary


def test_bake_symbols_and_struct(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)
        assert re.search(r"\b%s\(" % name, header), name
    # typedef struct mi355rt_bake_texel_outputs { uint32_t *owner; float *bary; uint32_t *ids; float *points, *normals, *albedo; }: six pointers
    assert C.sizeof(pkg.BakeTexelOutputs) == 48
    assert [n for n, _ in pkg.BakeTexelOutputs._fields_] == list(pkg.BAKE_TEXEL_OUTPUTS) == ["owner", "bary", "ids", "points", "normals", "albedo"]
    assert re.search(r"mi355rt_bake_texel_outputs \{ uint32_t \*owner; float \*bary; uint32_t \*ids; float \*points, \*normals, \*albedo; \}", header)
    import inspect
    sig = inspect.signature(pkg.RayTracer.bake)
    assert [(k, v.default) for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty][:5] == [("spp", 16), ("weight", "mean"), ("dilate", 2), ("first_sample", 0), ("into", None)]
    assert inspect.signature(pkg.RayTracer.bake_atlas).parameters["dilate"].default == 2
    assert inspect.signature(pkg.RayTracer.bake_texels).parameters["flip"].default is False


def test_bake_texel_refusals(pkg):
    L = pkg.lib()
    uv = np.zeros(6, F); cov = C.c_uint32(); b = np.zeros(2, F)
    assert L.mi355rt_bake_texel(None, 4, 4, 0, 0, C.byref(cov), fp(b)) == E_INVALID and b"uv6" in L.mi355rt_last_error(None)
    assert L.mi355rt_bake_texel(fp(uv), 4, 4, 0, 0, None, fp(b)) == E_INVALID and b"covered" in L.mi355rt_last_error(None)
    assert L.mi355rt_bake_texel(fp(uv), 0, 4, 0, 0, C.byref(cov), fp(b)) == E_INVALID and b"width" in L.mi355rt_last_error(None)
    assert L.mi355rt_bake_texel(fp(uv), 4, 16385, 0, 0, C.byref(cov), fp(b)) == E_INVALID
    assert L.mi355rt_bake_texel(fp(uv), 4, 4, 4, 0, C.byref(cov), fp(b)) == E_INVALID and b"outside" in L.mi355rt_last_error(None)
    assert L.mi355rt_bake_texel(fp(uv), 4, 4, 3, 3, C.byref(cov), None) == 0 and cov.value == 0          # bary2 may be NULL


@pytest.mark.parametrize("name", sorted(bc.charts(2)))
def test_host_twin_equals_the_statement_on_hand_made_charts(pkg, bake, name):
    uv, w, h = bc.charts(2)[name]
    want = bake.texels(uv, w, h)
    owner, bary = c_owners(pkg, uv, w, h)
    assert np.array_equal(owner, want["owner"])
    assert np.array_equal(bits(bary), bits(want["bary"]))
    assert np.array_equal(want["ids"], np.nonzero(want["owner"] != MISS)[0])


def test_host_twin_on_many_small_charts_over_a_whole_atlas_chart(pkg, bake):
    uv, w, h = bc.charts(48)["whole_atlas_under_small_ones"]
    want = bake.texels(uv, w, h)
    # the bins of the kernels are not in play here: every triangle against the texels of four rows
    rows = (0, 1, 17, 63)
    L = pkg.lib()
    for y in rows:
        for x in range(w):
            got = MISS
            for i in range(48):
                cov = C.c_uint32()
                assert L.mi355rt_bake_texel(fp(np.ascontiguousarray(uv[i].reshape(6))), w, h, x, y, C.byref(cov), None) == 0
                if cov.value:
                    got = i
                    break
            assert got == want["owner"][y * w + x], (x, y)
    assert (want["owner"] != MISS).all() and (want["owner"] == 47).sum() > 3000 and len(set(want["owner"])) == 48


def test_what_the_hand_made_charts_are_for(bake):
    c = bc.charts(2)
    o = lambda name: bake.texels(*c[name])["owner"].reshape(c[name][2], c[name][1])
    d = o("diagonal")
    assert (d != MISS).all() and (np.diag(d) == 0).all() and (d[np.triu_indices(8, 1)] == 0).all() and (d[np.tril_indices(8, -1)] == 1).all()
    s = o("diagonal_swapped")
    assert (np.diag(s) == 0).all() and (s[np.tril_indices(8, -1)] == 0).all() and (s[np.triu_indices(8, 1)] == 1).all()
    m = o("mirrored")
    assert np.array_equal(m, d)                                                   # both windings are accepted
    assert (o("zero_area") == MISS).all() and (o("outside") == MISS).all() and (o("sub_texel") == MISS).all() and (o("nan_inf") == MISS).all()
    hf = o("half_outside")
    assert (hf[:4, :4][np.add.outer(np.arange(4), np.arange(4)) <= 3] == 0).all() and (hf == 0).sum() == 10 and (hf[4:, 4:] == 1).all() and (hf == 1).sum() == 16
    ni = o("neg_inf")
    assert (ni != 0).all() and (ni == 1).sum() == 10                             # the chart with an infinite vertex covers nothing, the other is untouched
    ov, os_ = o("overlap"), o("overlap_swapped")
    assert (ov == 0).sum() > 50 and (ov == 1).sum() > 20 and ((os_ == 0) == (ov != MISS)).all() and (os_ != 1).all()
    assert bake.texels(*c["tiny_atlas"])["owner"].tolist() == [0]


def test_point_and_scene_lists_of_the_statement(pkg, bake, scenes):
    scene = scenes("ico3_tex")
    n = scene["tri_geom"].size
    uv = bake.auto_atlas(n, 96, 96)
    t = bake.texels(uv, 96, 96, scene)
    assert t["ncovered"] == t["ids"].size == t["points"].shape[0] and t["ncovered"] > n
    tri = t["owner"][t["ids"]]
    assert set(tri) == set(range(n))
    v = scene["tri_verts"][tri]
    L = pkg.lib()
    for k in range(0, t["ncovered"], 97):
        for a in range(3):
            got = F(L.mi355rt_bake_point(float(v[k, a]), float(F(v[k, 3 + a] - v[k, a])), float(F(v[k, 6 + a] - v[k, a])), float(t["bary"][t["ids"][k], 0]), float(t["bary"][t["ids"][k], 1])))
            assert bits(got) == bits(t["points"][k, a])
    # inside the triangle: u, v >= 0 and u + v <= 1 up to rounding, and the point lies in the triangle's plane
    u, w_ = t["bary"][t["ids"], 0], t["bary"][t["ids"], 1]
    assert (u >= 0).all() and (w_ >= 0).all() and (u + w_ <= 1 + 1e-6).all()
    flipped = bake.texels(uv, 96, 96, scene, flip=True)
    assert np.array_equal(bits(flipped["normals"]), bits(-t["normals"])) and np.array_equal(bits(flipped["points"]), bits(t["points"]))
    assert len(np.unique(t["albedo"], axis=0)) > 4                               # the texture shows in the albedo


# ---- the auto atlas ------------------------------------------------------------------------------------------------------------------------------------
def c_auto_atlas(pkg, ntri, w, h, gutter):
    uv = np.full((ntri, 3, 2), np.nan, F); cell = C.c_uint32(0)
    rc = pkg.lib().mi355rt_bake_auto_atlas(ntri, w, h, gutter, fp(uv), C.byref(cell))
    return rc, uv, cell.value


def smallest_accepted(bake, ntri, gutter):
    s = 1
    while True:
        try:
            bake.auto_atlas(ntri, s, s, gutter)
            return s
        except ValueError:
            s += 1


@pytest.mark.parametrize("gutter", [0, 1, 2])
@pytest.mark.parametrize("ntri", [1, 2, 3, 48, 608])
def test_auto_atlas_equals_its_statement_and_keeps_its_properties(pkg, bake, ntri, gutter):
    s0 = smallest_accepted(bake, ntri, gutter)
    rc, _, _ = c_auto_atlas(pkg, ntri, s0 - 1, s0 - 1, gutter) if s0 > 1 else (E_INVALID, None, None)
    assert rc == E_INVALID                                                      # the library refuses what the statement refuses
    top = max(64, s0)
    sizes = sorted({(s0, s0), (s0 + 1, s0), (s0, s0 + 3), ((s0 + top) // 2, top), (top, top), (top, (s0 + top) // 2 + 1)})
    for w, h in sizes:
        want = bake.auto_atlas(ntri, w, h, gutter)
        rc, uv, cell = c_auto_atlas(pkg, ntri, w, h, gutter)
        assert rc == 0 and np.array_equal(bits(uv), bits(want)), (w, h)
        assert cell >= 1 and (w // cell) * (h // cell) >= (ntri + 1) // 2 and ((w // (cell + 1)) * (h // (cell + 1)) < (ntri + 1) // 2 or cell == min(w, h))
        # through the statement's rasteriser: nobody claims a texel twice, everybody owns one, different owners keep their distance
        claims = np.zeros((h, w), np.int32)
        for i in range(ntri):
            claims += (bake.owners(want[i:i + 1], w, h)[0] != MISS).reshape(h, w) if ntri <= 48 else 0
        assert claims.max() <= 1
        owner = bake.owners(want, w, h)[0].reshape(h, w)
        if ntri <= 48:
            assert ((owner != MISS) == (claims == 1)).all()
        assert set(owner[owner != MISS]) == set(range(ntri))
        need = max(gutter, 1)
        for dy in range(-(need - 1), need):
            for dx in range(-(need - 1), need):
                a = owner[max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx)]
                b = owner[max(0, -dy):h + min(0, -dy), max(0, -dx):w + min(0, -dx)]
                assert ((a == b) | (a == MISS) | (b == MISS)).all(), (w, h, dx, dy)


def test_auto_atlas_claims_for_many_triangles(bake):
    # 608 triangles, one by one, on the atlas the GPU test uses: no texel is claimed twice
    uv = bake.auto_atlas(608, 128, 128, 1)
    claims = np.zeros(128 * 128, np.int32)
    for i in range(608):
        claims += bake.owners(uv[i:i + 1], 128, 128)[0] != MISS
    assert claims.max() == 1 and claims.sum() == (bake.owners(uv, 128, 128)[0] != MISS).sum()


def test_auto_atlas_refusals(pkg, bake):
    L = pkg.lib()
    uv = np.zeros((4, 3, 2), F)
    for args, word in (((0, 8, 8, 1), b"ntri"), ((4, 0, 8, 1), b"width"), ((4, 8, 16385, 1), b"width"), ((4, 8, 8, 20000), b"gutter"), ((4, 4, 4, 1), b"too small"), ((608, 64, 64, 1), b"too small")):
        big = np.zeros((max(args[0], 1), 3, 2), F)
        assert L.mi355rt_bake_auto_atlas(*args, fp(big), None) == E_INVALID
        assert word in L.mi355rt_last_error(None), (args, L.mi355rt_last_error(None))
        with pytest.raises(ValueError):
            bake.auto_atlas(*args)
    assert L.mi355rt_bake_auto_atlas(4, 8, 8, 1, None, None) == E_INVALID and b"uv is NULL" in L.mi355rt_last_error(None)
    assert L.mi355rt_bake_auto_atlas(4, 8, 8, 1, fp(uv), None) == 0              # cell may be NULL


# ---- the atlas -----------------------------------------------------------------------------------------------------------------------------------------
def c_atlas(pkg, ids, values, w, h, dilate):
    """the statement's loop around mi355rt_bake_dilate_texel"""
    L = pkg.lib()
    img = np.zeros((w * h, 3), F); val = np.zeros(w * h, np.uint8)
    img[ids] = values; val[ids] = 1
    for k in range(1, dilate + 1):
        nimg, nval = img.copy(), val.copy()
        for t in np.nonzero(val == 0)[0]:
            rgb = np.full(3, 9.0, F)
            if L.mi355rt_bake_dilate_texel(fp(img), val.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, int(t % w), int(t // w), fp(rgb)):
                nimg[t] = rgb; nval[t] = min(1 + k, 255)
        if np.array_equal(nval, val):
            break
        img, val = nimg, nval
    return img, val


@pytest.mark.parametrize("name", sorted(bc.masks()))
def test_atlas_statement_equals_the_host_twin(pkg, bake, name):
    ids, values, w, h, dilate = bc.masks()[name]
    img, val = bake.atlas(ids, values, w, h, dilate)
    cimg, cval = c_atlas(pkg, ids, values, w, h, dilate)
    assert np.array_equal(val, cval) and np.array_equal(bits(img), bits(cimg))
    assert np.array_equal(bits(img[ids]), bits(values)) and (val[ids] == 1).all()


def test_atlas_dilation_by_hand(bake):
    m = bc.masks()
    # one texel in the middle of 7 x 5: iteration k fills the ring at Chebyshev distance k with the one value
    ids, values, w, h, _ = m["one_texel"]
    img, val = bake.atlas(ids, values, w, h, 2)
    yy, xx = np.mgrid[0:h, 0:w]
    dist = np.maximum(abs(xx - 3), abs(yy - 2)).reshape(-1)
    assert np.array_equal(val, np.where(dist <= 2, 1 + dist, 0).astype(np.uint8))
    assert np.array_equal(bits(img[dist <= 2]), bits(np.broadcast_to(values[0], ((dist <= 2).sum(), 3)))) and (img[dist > 2] == 0).all()
    # the hole of a ring: eight neighbours in the order N, W, E, S, NW, NE, SW, SE, one division
    ids, values, w, h, _ = m["island"]
    img, val = bake.atlas(ids, values, w, h, 1)
    at = {int(i): v for i, v in zip(ids, values)}
    order = [(4, 2), (3, 3), (5, 3), (4, 4), (3, 2), (5, 2), (3, 4), (5, 4)]
    acc = at[order[0][1] * w + order[0][0]].copy()
    for x, y in order[1:]:
        acc = acc + at[y * w + x]
    assert np.array_equal(bits(img[3 * w + 4]), bits(acc / F(8))) and val[3 * w + 4] == 2
    # the borders do not wrap: a texel in the corner fills towards the inside only
    ids, values, w, h, _ = m["corner_texel"]
    img, val = bake.atlas(ids, values, w, h, 1)
    assert np.array_equal(np.nonzero(val)[0], [0, 1, 4, 5])
    # full and empty atlases stay what they are; dilate 0 is the scatter
    for name in ("full", "empty", "dilate_0"):
        ids, values, w, h, d = m[name]
        img, val = bake.atlas(ids, values, w, h, d)
        assert (val == 1).sum() == ids.size and (val <= 1).all() and (img[val == 0] == 0).all()
    # more iterations than the atlas is wide: everything is filled, the marks count the distance to the nearest given texel and nothing saturates here
    ids, values, w, h, d = m["dilate_beyond_the_atlas"]
    img, val = bake.atlas(ids, values, w, h, d)
    yy, xx = np.mgrid[0:h, 0:w]
    dist = np.minimum(np.maximum(abs(xx - 1), abs(yy - 5)), np.maximum(abs(xx - 9), abs(yy - 2))).reshape(-1)
    assert np.array_equal(val, (1 + dist).astype(np.uint8))
    # the sum starts from the first neighbour, not from +0: a lone -0 stays -0
    ids, values, w, h, d = m["negative_zero"]
    img, _ = bake.atlas(ids, values, w, h, d)
    assert np.array_equal(bits(img[1]), bits(np.array([-0.0, 1.0, 0.5], F)))
    with pytest.raises(ValueError):
        bake.atlas(np.array([1, 1], np.uint32), np.zeros((2, 3), F), 2, 2)
    with pytest.raises(ValueError):
        bake.atlas(np.array([4], np.uint32), np.zeros((1, 3), F), 2, 2)


def test_atlas_marks_saturate(bake):
    img, val = bake.atlas(np.array([0], np.uint32), np.ones((1, 3), F), 300, 1, 400)
    assert val[0] == 1 and val[253] == 254 and (val[254:] == 255).all() and (img == 1).all()


# ---- against exact rational coverage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_statement_agrees_with_exact_coverage(bake, seed):
    uv, size = bc.jittered_mesh(seed)
    owner = bake.owners(uv, size, size)[0].reshape(size, size)
    px = uv[:, :, 0].astype(np.float64) * size; py = uv[:, :, 1].astype(np.float64) * size
    inside_unowned = owned_outside = 0
    for y in range(size):
        for x in range(size):
            near = np.nonzero((px.min(1) <= x + 1) & (px.max(1) >= x) & (py.min(1) <= y + 1) & (py.max(1) >= y))[0]
            inside = any(bc.exactly_inside(uv[i], size, x, y) for i in near)
            o = owner[y, x]
            if o == MISS:
                inside_unowned += inside
            elif not bc.exactly_inside(uv[o], size, x, y):
                owned_outside += 1
    print("seed %d: %d texels, %d exactly inside but unowned, %d owned but exactly outside" % (seed, size * size, inside_unowned, owned_outside))
    assert (owner != MISS).all()                                                # the mesh covers the atlas
    assert inside_unowned == 0 and owned_outside == 0
