"""Probe visibility without a GPU (include/mi355rt.h "PROBE VISIBILITY"): the entry points and structs are what the header says, and the host
side of the shared arithmetic (mi355rt_oct_encode, mi355rt_oct_texel, mi355rt_probe_visibility_one, mi355rt_probes_lookup_vis_one: csrc/oct_vis.hpp, the header
the kernels compile) equals the numpy statement (raytracer_rs_amd.probes) bit for bit on hand-made films, directions and queries.  The statement itself is held
to the closed-form octahedral map in float64, to the geometry of the map's seams, to hand-written sums, to the unweighted lookup it must collapse to, and to a
wall it must not let light through.  tests/test_gpu_probes_vis.py runs the kernels against the same statement."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import probe_cases as pc
import probe_vis_cases as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_probes_vis_default_config", "mi355rt_probes_gather_depth", "mi355rt_probes_lookup_vis", "mi355rt_oct_encode", "mi355rt_oct_texel",
       "mi355rt_probe_visibility_one", "mi355rt_probes_lookup_vis_one"]
F = np.float32
FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)
fp = lambda a: a.ctypes.data_as(FP)
up = lambda a: a.ctypes.data_as(UP)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pr(pkg):
    return importlib.import_module("raytracer_rs_amd.probes")


def c_depth(pkg, depth, probe=None):
    """mi355rt_probe_depth over the arrays of a film (of one of its probes)"""
    cnt, mom = (depth["count"], depth["moments"]) if probe is None else (depth["count"][probe], depth["moments"][probe])
    assert cnt.flags["C_CONTIGUOUS"] and mom.flags["C_CONTIGUOUS"] and cnt.dtype == np.uint32 and mom.dtype == F
    return pkg.ProbeDepth(int(depth["res"]), float(depth["max_distance"]), cnt.ctypes.data, mom.ctypes.data)


def c_encode(pkg, d):
    out = np.full((len(d), 2), 7.0, F)
    for i in range(len(d)):
        assert pkg.lib().mi355rt_oct_encode(fp(d[i]), fp(out[i])) == 0
    return out[:, 0].copy(), out[:, 1].copy()


def c_texel(pkg, d, R):
    out = np.full((len(d), 2), 99, np.uint32)
    for i in range(len(d)):
        assert pkg.lib().mi355rt_oct_texel(fp(d[i]), R, up(out[i])) == 0
    return out[:, 0].copy(), out[:, 1].copy()


def c_visibility(pkg, depth, probe, vs):
    d = c_depth(pkg, depth, probe)
    out = np.full(len(vs), 7.0, F)
    w = C.c_float(7.0)
    for i in range(len(vs)):
        assert pkg.lib().mi355rt_probe_visibility_one(C.byref(d), fp(vs[i]), C.byref(w)) == 0
        out[i] = w.value
    return out


def c_lookup_vis(pkg, g, res, depth, usable, points, dirs, nrm, mode, cheb, facing, bias):
    """one mi355rt_probes_lookup_vis_one call per query -> (rgb, ok)"""
    grid = pkg.ProbeGrid.from_dict(g)
    n = np.ascontiguousarray(res["n"], np.uint32); sh = np.ascontiguousarray(res["sh"], F)
    d = c_depth(pkg, depth)
    vc = pkg.ProbeVisConfig((1 if cheb else 0) | (2 if facing and nrm is not None else 0), bias)
    usp = None if usable is None else usable.ctypes.data_as(C.POINTER(C.c_uint8))
    rgb = np.full((len(points), 3), np.nan, F); ok = np.zeros(len(points), np.uint8)
    one = C.c_uint32(99)
    for q in range(len(points)):
        assert pkg.lib().mi355rt_probes_lookup_vis_one(C.byref(grid), up(n), fp(sh), usp, C.byref(d), C.byref(vc), fp(points[q]), fp(dirs[q]),
                                                       None if nrm is None else fp(nrm[q]), pkg.SH_MODES[mode], fp(rgb[q]), C.byref(one)) == 0
        ok[q] = one.value
    return rgb, ok


# ---- symbols, structs, refusals ------------------------------------------------------------------------------------------------------------------------
def test_vis_symbols_structs_defaults_and_refusals(pkg, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)
        assert re.search(r"\b%s\(" % name, header), name
    for name, value in (("MI355RT_VIS_CHEBYSHEV", pkg.VIS_CHEBYSHEV), ("MI355RT_VIS_FACING", pkg.VIS_FACING)):
        m = re.search(r"#define\s+%s\s+(\d+)u" % name, header)
        assert m and int(m.group(1)) == value, name
    assert (pkg.VIS_CHEBYSHEV, pkg.VIS_FACING) == (1, 2)
    assert C.sizeof(pkg.ProbeDepth) == 24
    assert [(n, getattr(pkg.ProbeDepth, n).offset) for n, _ in pkg.ProbeDepth._fields_] == [("res", 0), ("max_distance", 4), ("count", 8), ("moments", 16)]
    assert C.sizeof(pkg.ProbeVisConfig) == 8
    assert [(n, getattr(pkg.ProbeVisConfig, n).offset) for n, _ in pkg.ProbeVisConfig._fields_] == [("flags", 0), ("normal_bias", 4)]
    # the structs of PROBES are what they were
    assert (C.sizeof(pkg.ProbeConfig), C.sizeof(pkg.ProbeOutputs), C.sizeof(pkg.ProbeGrid)) == (16, 32, 36)
    assert pkg.PROBE_OUTPUTS == ("n", "hits", "near", "sh")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355rt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %u %u\\n",'
                   'sizeof(mi355rt_probe_depth),sizeof(mi355rt_probe_vis_config),offsetof(mi355rt_probe_depth,max_distance),offsetof(mi355rt_probe_depth,count),'
                   'offsetof(mi355rt_probe_depth,moments),offsetof(mi355rt_probe_vis_config,normal_bias),MI355RT_VIS_CHEBYSHEV,MI355RT_VIS_FACING);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [24, 8, 4, 8, 16, 4, 1, 2]
    lib = pkg.lib()
    vc = pkg.ProbeVisConfig(9, 4.0)
    lib.mi355rt_probes_vis_default_config(C.byref(vc))
    assert vc.flags == 3 and vc.normal_bias == 0.0
    lib.mi355rt_probes_vis_default_config(None)          # tolerated
    # NULL handles and arguments
    cfg = pkg.ProbeConfig(); lib.mi355rt_probes_default_config(C.byref(cfg))
    assert lib.mi355rt_probes_gather_depth(None, None, None, 0, C.byref(cfg), 0, None, None) == -1
    assert lib.mi355rt_probes_lookup_vis(None, None, None, None, None, None, None, None, None, None, 0, 0, 0, None, None) == -1
    err = lambda: lib.mi355rt_last_error(None).decode()
    v3 = np.array([0.0, 0.0, 1.0], F); o2 = np.zeros(2, F); i2 = np.zeros(2, np.uint32)
    assert lib.mi355rt_oct_encode(None, fp(o2)) == -1 and "dir" in err()
    assert lib.mi355rt_oct_encode(fp(v3), None) == -1 and "uv" in err()
    assert lib.mi355rt_oct_texel(None, 8, up(i2)) == -1 and lib.mi355rt_oct_texel(fp(v3), 8, None) == -1
    for R in (0, 1, 17, 2**31):
        assert lib.mi355rt_oct_texel(fp(v3), R, up(i2)) == -1 and "res" in err()
    f = pv.film(3, 1, 1)
    w = C.c_float(7.0)
    good = c_depth(pkg, f)
    assert lib.mi355rt_probe_visibility_one(C.byref(good), fp(v3), C.byref(w)) == 0 and w.value != 7.0
    w = C.c_float(7.0)

    def depth_with(**kw):
        d = c_depth(pkg, f)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bad_depths = [(dict(res=1), "res"), (dict(res=17), "res"), (dict(res=0), "res"), (dict(max_distance=0.0), "max_distance"), (dict(max_distance=-1.0), "max_distance"),
                  (dict(max_distance=float("nan")), "max_distance"), (dict(max_distance=float("inf")), "max_distance"), (dict(max_distance=2e12), "max_distance"),
                  (dict(count=None), "count"), (dict(moments=None), "moments")]
    for kw, word in bad_depths:
        assert lib.mi355rt_probe_visibility_one(C.byref(depth_with(**kw)), fp(v3), C.byref(w)) == -1 and word in err(), kw
    assert lib.mi355rt_probe_visibility_one(None, fp(v3), C.byref(w)) == -1 and "depth" in err()
    assert lib.mi355rt_probe_visibility_one(C.byref(good), None, C.byref(w)) == -1 and lib.mi355rt_probe_visibility_one(C.byref(good), fp(v3), None) == -1
    assert w.value == 7.0
    assert lib.mi355rt_probe_visibility_one(C.byref(depth_with(max_distance=1e12)), fp(v3), C.byref(w)) == 0       # the top itself is allowed
    # the lookup of one query
    g = pkg.ProbeGrid.from_dict(pc.grid((1, 1, 1)))
    n = np.ones(1, np.uint32); sh = np.zeros(27, F)
    rgb = np.full(3, 7.0, F)
    lib.mi355rt_probes_vis_default_config(C.byref(vc))

    def one(grid=g, n_=n, sh_=sh, depth=good, vc_=vc, point=v3, dir_=v3, normal=v3, mode=0, rgb_=rgb):
        a = lambda x, conv: None if x is None else conv(x)
        return lib.mi355rt_probes_lookup_vis_one(a(grid, C.byref), a(n_, up), a(sh_, fp), None, a(depth, C.byref), a(vc_, C.byref), a(point, fp), a(dir_, fp), a(normal, fp),
                                                 mode, a(rgb_, fp), None)

    assert one() == 0 and not np.array_equal(rgb, np.full(3, 7.0, F))
    rgb[:] = 7.0
    for kw, word in ((dict(grid=None), "grid"), (dict(n_=None), "n is NULL"), (dict(sh_=None), "sh"), (dict(depth=None), "depth"), (dict(vc_=None), "vc"),
                     (dict(point=None), "point"), (dict(dir_=None), "dir"), (dict(rgb_=None), "rgb"), (dict(mode=2), "mode"),
                     (dict(normal=None), "normals3"),                                                            # the default flags hold FACING
                     (dict(normal=None, vc_=pkg.ProbeVisConfig(1, 0.5)), "normal_bias"), (dict(vc_=pkg.ProbeVisConfig(4, 0.0)), "flags"),
                     (dict(vc_=pkg.ProbeVisConfig(3, float("nan"))), "normal_bias"), (dict(vc_=pkg.ProbeVisConfig(0, float("inf"))), "normal_bias")):
        assert one(**kw) == -1 and word in err(), (kw, err())
        assert "mi355rt_probes_lookup_vis_one" in err()
    for kw, word in bad_depths:
        assert one(depth=depth_with(**kw)) == -1 and word in err(), kw
    assert np.array_equal(rgb, np.full(3, 7.0, F))                                                               # a refusal writes nothing
    assert one(normal=None, vc_=pkg.ProbeVisConfig(1, 0.0)) == 0 and one(normal=None, vc_=pkg.ProbeVisConfig(0, -0.0)) == 0
    bad = pkg.ProbeGrid.from_dict(pc.grid((1, 1, 1))); bad.spacing[1] = 0.0
    assert one(grid=bad) == -1 and "spacing" in err()


# ---- the map ----------------------------------------------------------------------------------------------------------------------------------------------
def closed_form(d):
    """the octahedral map in float64 from its textbook form: project on the octahedron |x| + |y| + |z| = 1, fold the lower half outwards, map [-1, 1] to [0, 1]"""
    d = np.asarray(d, np.float64)
    p = d / np.abs(d).sum(axis=1)[:, None]
    px, py = p[:, 0].copy(), p[:, 1].copy()
    low = d[:, 2] < 0
    sx, sy = np.where(d[:, 0] >= 0, 1.0, -1.0), np.where(d[:, 1] >= 0, 1.0, -1.0)
    px[low], py[low] = ((1 - np.abs(p[:, 1])) * sx)[low], ((1 - np.abs(p[:, 0])) * sy)[low]
    return px * 0.5 + 0.5, py * 0.5 + 0.5


def decode(u, w):
    """the point of the octahedron |x| + |y| + |z| = 1 at (u, w) of the unit square, float64: the inverse of closed_form"""
    px, py = 2 * np.asarray(u, np.float64) - 1, 2 * np.asarray(w, np.float64) - 1
    z = 1 - np.abs(px) - np.abs(py)
    x = np.where(z >= 0, px, (1 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0))
    y = np.where(z >= 0, py, (1 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0))
    return np.stack([x, y, z], axis=-1)


def test_oct_encode_and_texel_equal_the_statement_and_the_closed_form(pkg, pr):
    d = pv.directions()
    assert len(d) > 3400 and np.isfinite(d).all()
    u, w = pr.oct_encode(d)
    assert u.dtype == F and not np.isnan(u).any() and not np.isnan(w).any()
    cu, cw = c_encode(pkg, d)
    assert np.array_equal(bits(cu), bits(u)) and np.array_equal(bits(cw), bits(w))
    assert u.min() >= 0 and u.max() <= 1 and w.min() >= 0 and w.max() <= 1
    assert (u == 0).any() and (u == 1).any() and (w == 0).any() and (w == 1).any()                              # the square's edges are reached exactly
    # by hand on one direction of each half, every rounding written out
    for x, y, z in ((F(0.3), F(-0.5), F(0.7)), (F(-0.3), F(0.5), F(-0.7))):
        s = F(F(abs(x) + abs(y)) + abs(z))
        px, py = F(x / s), F(y / s)
        if z < 0:
            px, py = F(F(F(1.0) - abs(py)) * (F(1.0) if x >= 0 else F(-1.0))), F(F(F(1.0) - abs(px)) * (F(1.0) if y >= 0 else F(-1.0)))
        hand = np.array([F(F(px * F(0.5)) + F(0.5)), F(F(py * F(0.5)) + F(0.5))], F)
        got = pr.oct_encode(np.array([x, y, z], F))
        assert np.array_equal(bits(np.array(got, F)), bits(hand))
    # against the closed form in float64: one division, at most a subtraction and a multiply-add of values <= 1 — 4 ulp of 1
    ru, rw = closed_form(d)
    assert np.abs(u.astype(np.float64) - ru).max() <= 4 * 2.0 ** -24 and np.abs(w.astype(np.float64) - rw).max() <= 4 * 2.0 ** -24
    # ... and the map inverts: the decoded point is the direction scaled to the octahedron
    back = decode(u, w)
    want = d.astype(np.float64) / np.abs(d.astype(np.float64)).sum(axis=1)[:, None]
    assert np.abs(back - want).max() <= 2e-6                                                                    # z = 1 - |px| - |py| adds the two errors, each doubled by 2 u - 1
    # the texel
    odd = pv.odd_vectors()
    for R in pv.RES + (5, 7):
        ix, iy = pr.oct_texel(d, R)
        cx, cy = c_texel(pkg, d, R)
        assert ix.dtype == np.uint32 and np.array_equal(ix, cx) and np.array_equal(iy, cy)
        assert ix.max() == R - 1 and iy.max() == R - 1 and ix.min() == 0 and iy.min() == 0
        assert np.array_equal(ix, np.minimum(np.floor(u * F(R)), R - 1)) and np.array_equal(iy, np.minimum(np.floor(w * F(R)), R - 1))          # the conversion is a floor
        # vectors without a direction land in a texel all the same: no index is made from a NaN
        ox, oy = pr.oct_texel(odd, R)
        gx, gy = c_texel(pkg, odd, R)
        assert np.array_equal(ox, gx) and np.array_equal(oy, gy) and ox.max() <= R - 1 and oy.max() <= R - 1
        assert (ox[0], oy[0]) == (0, 0)                                                                           # the zero vector: 0 / 0 is a NaN, which becomes 0
    with pytest.raises(ValueError, match="res"):
        pr.oct_texel(d[:3], 1)
    with pytest.raises(ValueError, match="res"):
        pr.oct_texel(d[:3], 17)


@pytest.mark.parametrize("R", pv.RES)
def test_wrap_puts_a_neighbour_beyond_the_edge_on_an_adjacent_texel(pr, R):
    """Decoded in float64, the centre of the texel an out-of-range neighbour wraps to lies on the octahedron no farther from the centre of the texel it is a
    neighbour of than in-range neighbours (the eight around a texel) ever lie from each other, and it is the texel the map itself assigns to the point just
    beyond the edge: walking over the edge of the square is walking over a seam of the octahedron."""
    centre = lambda i, j: decode((np.asarray(i) + 0.5) / R, (np.asarray(j) + 0.5) / R)
    ii, jj = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    far = 0.0
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ni, nj = ii + di, jj + dj
            ok = (ni >= 0) & (ni < R) & (nj >= 0) & (nj < R)
            far = max(far, np.linalg.norm(centre(ii[ok], jj[ok]) - centre(ni[ok], nj[ok]), axis=1).max())
    seen = 0
    for i in range(R):
        for j in range(R):
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    ni, nj = i + di, j + dj
                    wi, wj = pr.oct_wrap(ni, nj, R)
                    wi, wj = int(wi), int(wj)
                    assert 0 <= wi < R and 0 <= wj < R
                    if 0 <= ni < R and 0 <= nj < R:
                        assert (wi, wj) == (ni, nj)                                                              # in range: untouched
                        continue
                    seen += 1
                    assert np.linalg.norm(centre(wi, wj) - centre(i, j)) <= far * (1 + 1e-12), (i, j, ni, nj, wi, wj)
                    if (0 <= ni < R) != (0 <= nj < R):
                        # over one edge: the point a little beyond the edge, mirrored back over the seam (the edge is glued to itself about its midpoint), is in
                        # the texel the rule names
                        u, w = (ni + 0.5) / R, (nj + 0.5) / R
                        if not 0 <= ni < R:
                            u, w = (-u if ni < 0 else 2 - u), 1 - w
                        else:
                            u, w = 1 - u, (-w if nj < 0 else 2 - w)
                        assert (int(u * R), int(w * R)) == (wi, wj)
    assert seen == 4 * R + 4 + 2 * 4 * (R - 1)                                                                   # edge texels look out once or (corners) five times


# ---- the depth film -------------------------------------------------------------------------------------------------------------------------------------------
def test_project_depth_with_prev_and_by_hand(pr):
    rng = np.random.default_rng(8)
    npts, spp, R, D = 5, 12, 3, 2.5
    d = rng.normal(size=(spp * npts, 3))
    d = np.ascontiguousarray((d / np.linalg.norm(d, axis=1)[:, None]).astype(F))
    t = rng.uniform(0.1, 5, spp * npts).astype(F)
    t[7] = np.nan; t[9] = F(D); t[13] = np.inf
    hit = rng.random(spp * npts) < 0.7
    hit[[7, 9, 13]] = True
    one = pr.project_depth(t, hit, d, npts, R, D)
    assert one["count"].dtype == np.uint32 and one["count"].shape == (npts, 9) and one["moments"].dtype == F and one["moments"].shape == (npts, 9, 2)
    assert (one["count"].sum(axis=1) == spp).all()                                                               # every sample in exactly one texel
    a = pr.project_depth(t[:5 * npts], hit[:5 * npts], d[:5 * npts], npts, R, D)
    keep = {k: v.copy() for k, v in a.items()}
    b = pr.project_depth(t[5 * npts:], hit[5 * npts:], d[5 * npts:], npts, R, D, prev=a)
    assert all(np.array_equal(keep[k], a[k]) for k in keep)                                                      # prev is not written
    assert np.array_equal(b["count"], one["count"]) and np.array_equal(bits(b["moments"]), bits(one["moments"]))
    # by hand, point by point, in sample order
    plain = clamped = missed = 0
    for i in range(npts):
        cnt = np.zeros(9, np.uint32); m = np.zeros((9, 2), F)
        for s in range(spp):
            e = s * npts + i
            ix, iy = pr.oct_texel(d[e], R)
            k = int(iy) * R + int(ix)
            if hit[e] and t[e] < F(D):
                dist = t[e]; plain += 1
            else:
                dist = F(D); clamped += int(hit[e]); missed += int(not hit[e])
            cnt[k] += 1
            m[k, 0] = F(m[k, 0] + dist)
            m[k, 1] = F(m[k, 1] + F(dist * dist))
        assert np.array_equal(cnt, one["count"][i]) and np.array_equal(bits(m), bits(one["moments"][i]))
    assert plain > 10 and clamped > 5 and missed > 5 and np.isfinite(one["moments"]).all()                      # the NaN and the infinite t became D
    for R_, D_ in ((1, 1.0), (17, 1.0), (2.5, 1.0), (8, 0.0), (8, -1.0), (8, np.inf), (8, np.nan), (8, 2e12)):
        with pytest.raises(ValueError):
            pr.project_depth(t, hit, d, npts, R_, D_)
    # at the top of max_distance 2^32 samples' worth of D^2 is still finite
    assert np.isfinite(F(F(1e12) * F(1e12)) * F(2.0 ** 32))


# ---- visibility ---------------------------------------------------------------------------------------------------------------------------------------------
def test_visibility_one_equals_the_statement(pkg, pr):
    vs = np.ascontiguousarray(np.concatenate([pv.directions()[::3], pv.odd_vectors()]))
    ones = below = 0
    for R in pv.RES:
        for seed, empty in ((1, 0.25), (2, 0.7), (3, 0.0)):
            f = pv.film(R, 2, seed, empty)
            want = np.array([pr.visibility(f["count"][1], f["moments"][1], R, v) for v in vs], F)
            got = c_visibility(pkg, f, 1, vs)
            assert np.array_equal(bits(got), bits(want)), (R, seed)
            assert not np.isnan(want).any() and want.min() >= 0 and want.max() <= 1                              # the infinities of the empty texels were never read
            ones += int((want == 1).sum()); below += int((want < 1).sum())
        # r that is not a positive finite number: 1, whatever the film
        odd = pv.odd_vectors()
        w = c_visibility(pkg, pv.flat_film(R, 1), 0, odd)
        with np.errstate(all="ignore"):
            rr = np.sqrt((odd[:, 0] * odd[:, 0] + odd[:, 1] * odd[:, 1]) + odd[:, 2] * odd[:, 2])
        fine = (rr > 0) & np.isfinite(rr)
        assert (~fine).sum() >= 9 and fine.sum() >= 3 and (w[~fine] == 1).all()
        assert np.array_equal(w[fine], (rr[fine] <= F(2.0 ** -6)).astype(F)) and (w[fine] == 0).any() and (w[fine] == 1).any()        # the flat film: 0 beyond its mean
        # all four texels empty: no information, 1
        none = dict(res=R, max_distance=F(3.0), count=np.zeros((1, R * R), np.uint32), moments=np.full((1, R * R, 2), np.inf, F))
        assert (c_visibility(pkg, none, 0, vs) == 1).all()
        assert all(pr.visibility(none["count"][0], none["moments"][0], R, v) == 1 for v in vs[::50])
    assert ones > 1000 and below > 1000


def test_visibility_by_hand(pkg, pr):
    # R = 3 and the direction +z: u = w = 0.5, g = 0.5 * 3 + 0.5 = 2 exactly, so i1 = 2 and f = 0 on both axes — the one texel (1, 1) with weight 1
    R = 3
    cnt = np.zeros(9, np.uint32); m = np.full((9, 2), np.inf, F)
    cnt[4] = 8; m[4] = [12.0, 18.0]                                      # mean 1.5, mean2 2.25: var 0
    f = dict(res=R, max_distance=F(3.0), count=cnt[None], moments=m[None])
    for v, want in (([0, 0, 1.5], 1.0), ([0, 0, 1.0], 1.0), ([0, 0, 1.5000001], 0.0), ([0, 0, 2.0], 0.0)):       # r == mean and r < mean: 1; var == 0 beyond: 0
        v = np.array(v, F)
        assert pr.visibility(cnt, m, R, v) == F(want) and c_visibility(pkg, f, 0, v[None])[0] == F(want), v
    m[4] = [12.0, 20.0]                                                  # mean2 2.5: var 0.25; at r = 2: dd = 0.5, c = 0.25 / (0.25 + 0.25) = 0.5, weight 0.125
    assert pr.visibility(cnt, m, R, np.array([0, 0, 2.0], F)) == F(0.125) and c_visibility(pkg, f, 0, np.array([[0, 0, 2.0]], F))[0] == F(0.125)
    # two texels with count 0 among the four: R = 2, direction (1, 1, 2): u = w = 0.625, g = 1.75: i1 = 1, f = 0.75 on both axes; texels (0..1, 0..1)
    R = 2
    cnt = np.array([4, 0, 0, 2], np.uint32); m = np.array([[4.0, 5.0], [np.inf, np.inf], [np.inf, np.inf], [2.0, 3.0]], F)
    v = np.array([1, 1, 2], F)
    wts = [F(0.25) * F(0.25), F(0.75) * F(0.75)]
    ws = F(F(0.0) + wts[0]) + wts[1]
    a = F(F(F(0.0) + F(wts[0] * F(F(4.0) / F(4.0)))) + F(wts[1] * F(F(2.0) / F(2.0))))
    b = F(F(F(0.0) + F(wts[0] * F(F(5.0) / F(4.0)))) + F(wts[1] * F(F(3.0) / F(2.0))))
    mean, mean2 = F(a / ws), F(b / ws)
    r = np.sqrt(F(F(F(1.0) + F(1.0)) + F(4.0)))
    var = abs(F(mean2 - F(mean * mean))); dd = F(r - mean)
    c = F(var / F(var + F(dd * dd)))
    hand = F(F(c * c) * c)
    assert r > mean and 0 < hand < 1
    got = pr.visibility(cnt, m, R, v)
    assert bits(got) == bits(hand)
    assert bits(c_visibility(pkg, dict(res=R, max_distance=F(3.0), count=cnt[None], moments=m[None]), 0, v[None])[0]) == bits(hand)
    with pytest.raises(ValueError, match="res"):
        pr.visibility(cnt, m, 1, v)


# ---- the weighted lookup -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["radiance", "irradiance"])
def test_lookup_vis_one_equals_the_statement_and_collapses_to_lookup(pkg, pr, mode):
    lookup_one = importlib.import_module("test_probes_abi").c_lookup
    used = unused = differs = 0
    for k, (name, g, res, depth, usable, pts, dirs, nrm) in enumerate(pv.lookup_cases()):
        step = 1 if len(pts) < 200 else 2                              # the queries' kinds repeat with period 8: every second one still holds each kind
        p, d, nr = (np.ascontiguousarray(a[k % step::step]) for a in (pts, dirs, nrm))
        plain, pok = pr.lookup(g, res, p, d, mode, usable)
        for cheb, facing in pv.FLAGS:
            for normals, bias in ((nr, 0.0), (nr, 0.13), (None, 0.0)):
                want, wok = pr.lookup_vis(g, res, depth, p, d, normals, mode, usable, cheb, facing, bias)
                got, gok = c_lookup_vis(pkg, g, res, depth, usable, p, d, normals, mode, cheb, facing, bias)
                assert want.dtype == F and wok.dtype == np.uint8
                assert np.array_equal(gok, wok), (name, cheb, facing, bias)
                assert np.array_equal(bits(got), bits(want)), (name, cheb, facing, bias)
                assert not want[wok == 0].view(np.uint32).any()                                                 # rgb exactly +0 where no corner was used
                assert not (wok & ~pok).any()                                                                    # weighting never adds a corner
                if not cheb and (not facing or normals is None):
                    # the reduction: (t * 1) * 1 is t, on every bit, for the statement and for the library's own unweighted entry
                    assert np.array_equal(bits(want), bits(plain)) and np.array_equal(wok, pok), (name, bias)
                else:
                    differs += int((bits(want) != bits(plain)).any())
                used += int(wok.sum()); unused += int((wok == 0).sum())
        c_plain, c_pok = lookup_one(pkg, g, res, usable, p, d, mode)
        c_zero, c_zok = c_lookup_vis(pkg, g, res, depth, usable, p, d, nr, mode, False, False, 0.0)
        assert np.array_equal(bits(c_zero), bits(c_plain)) and np.array_equal(c_zok, c_pok) and np.array_equal(bits(c_plain), bits(plain))
        if name.endswith("flat"):
            # visibility 0 beyond 2^-6 of a probe: only a query on a usable probe keeps a corner, and the mask has hidden some of those
            want, wok = pr.lookup_vis(g, res, depth, p, d, None, mode, usable, True, False, 0.0)
            assert 0 < wok.sum() < pok.sum() and (wok == 0).sum() > len(p) // 2
            hidden = np.zeros_like(usable)
            assert not pr.lookup_vis(g, res, depth, p, d, None, mode, hidden, True, False, 0.0)[1].any()
        if name.startswith("nothing usable"):
            assert not pr.lookup_vis(g, res, depth, p, d, nr, mode, usable)[1].any()
    assert used > 5000 and unused > 1000 and differs > 20
    with pytest.raises(ValueError, match="mode"):
        pr.lookup_vis(g, res, depth, p, d, None, "sine")
    with pytest.raises(ValueError, match="normal_bias"):
        pr.lookup_vis(g, res, depth, p, d, nr, mode, normal_bias=float("nan"))


def test_lookup_vis_by_hand(pkg, pr):
    """One query between two probes on the x axis, (2, 1, 1) grid: every number of the two corners written out."""
    g = dict(origin=np.array([-1.0, 0.0, 0.0], F), spacing=np.array([2.0, 1.0, 1.0], F), counts=np.array([2, 1, 1], np.uint32))
    rng = np.random.default_rng(12)
    res = dict(n=np.array([16, 9], np.uint32), sh=rng.normal(size=(2, 9, 3)).astype(F))
    depth = pv.film(3, 2, 77, empty=0.0)
    p = np.array([[0.5, 0.25, -0.125]], F); nrm = np.array([[-0.6, 0.0, 0.8]], F); d = np.array([[0.0, 0.6, 0.8]], F); bias = F(0.25)
    pb = (p[0] + bias * nrm[0]).astype(F)
    C_ = np.zeros(27, F); wsum = F(0.0)
    for j, t in ((0, F(0.25)), (1, F(0.75))):                           # f_x = (0.5 + 1) / 2 = 0.75; y and z have one probe: weight 1 on the lower, 0 on the upper corner
        pos = np.array([g["origin"][0] + F(j) * g["spacing"][0], 0.0, 0.0], F)
        v = (pb - pos).astype(F)
        r = np.sqrt(F(F(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
        vis = pr.visibility(depth["count"][j], depth["moments"][j], 3, v)
        q = F(F(F(F(F(-v[0]) * nrm[0, 0] + F(-v[1]) * nrm[0, 1]) + F(-v[2]) * nrm[0, 2]) / r + F(1.0)) * F(0.5))
        q = q if q >= F(0.0001) else F(0.0001)
        face = F(F(q * q) + F(0.2))
        wj = F(F(t * vis) * face)
        assert wj != 0
        wsum = F(wsum + wj)
        s = F(wj * F(F(12.566370614) / F(res["n"][j])))
        C_ = (C_ + s * res["sh"][j].reshape(27)).astype(F)
    b = pr.basis(d[0])
    want = np.zeros(3, F)
    for k in range(9):
        A = (F(3.14159265), F(2.09439510), F(0.785398163))[0 if k == 0 else 1 if k < 4 else 2]
        want = (want + (A * C_[3 * k:3 * k + 3]) * b[k]).astype(F)
    want = (want / wsum).astype(F)
    rgb, ok = pr.lookup_vis(g, res, depth, p, d, nrm, "irradiance", None, True, True, float(bias))
    assert ok[0] == 1 and np.array_equal(bits(rgb[0]), bits(want))
    crgb, cok = c_lookup_vis(pkg, g, res, depth, None, p, d, nrm, "irradiance", True, True, float(bias))
    assert cok[0] == 1 and np.array_equal(bits(crgb[0]), bits(want))
    assert pr.grid_max_distance(g) == float(F(1.5 * np.sqrt(6.0)))


# ---- the wall -------------------------------------------------------------------------------------------------------------------------------------------------
def wall_film(pr, probe_x, R, n, seed):
    """The depth film of a probe at (probe_x, 0, 0) in a world whose only surface is the plane x = 0, from n uniform sphere samples; D = 3"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d = np.ascontiguousarray((d / np.linalg.norm(d, axis=1)[:, None]).astype(F))
    with np.errstate(all="ignore"):
        t = (-probe_x / d[:, 0].astype(np.float64))
    hit = np.isfinite(t) & (t > 0)
    return pr.project_depth(np.where(hit, t, 0).astype(F), hit, d, 1, R, 3.0)


def test_a_probe_behind_a_wall_gets_no_weight(pkg, pr):
    """Probe A at x = -1 behind the wall x = 0, probe B at x = +1 in front of it, a query 0.5 beyond the wall at x = 0.5: trilinear alone gives A 0.25.  With the
    Chebyshev weight (R = 8, 1 024 fixed-seed samples, D = 3) A must get below 1e-3 of the weight — a condition; the numpy prototype gave 6e-11.  B sees the
    query nearer than its mean depth that way and keeps visibility exactly 1."""
    R, n = 8, 1024
    fa, fb = wall_film(pr, -1.0, R, n, 101), wall_film(pr, 1.0, R, n, 102)
    depth = dict(res=R, max_distance=F(3.0), count=np.concatenate([fa["count"], fb["count"]]), moments=np.concatenate([fa["moments"], fb["moments"]]))
    q = np.array([0.5, 0.0, 0.0], F)
    va = pr.visibility(depth["count"][0], depth["moments"][0], R, q - np.array([-1, 0, 0], F))
    vb = pr.visibility(depth["count"][1], depth["moments"][1], R, q - np.array([1, 0, 0], F))
    share = float(F(0.25) * va) / (float(F(0.25) * va) + float(F(0.75) * vb))
    print("visibility of the probe behind the wall %.3g, in front %.3g; A's share of the weight %.3g" % (va, vb, share))
    assert vb == 1 and share < 1e-3
    # the same through the lookup: A's light (red) against B's (green), as the library's host entry computes it
    g = dict(origin=np.array([-1.0, 0.0, 0.0], F), spacing=np.array([2.0, 1.0, 1.0], F), counts=np.array([2, 1, 1], np.uint32))
    sh = np.zeros((2, 9, 3), F)
    sh[0, 0, 0] = 1.0; sh[1, 0, 1] = 1.0
    res = dict(n=np.array([1, 1], np.uint32), sh=sh)
    plain = pr.lookup(g, res, q[None], np.array([[1, 0, 0]], F), "radiance")[0][0]
    assert abs(plain[0] / (plain[0] + plain[1]) - 0.25) < 1e-6                                                  # the leak
    rgb, ok = c_lookup_vis(pkg, g, res, depth, None, q[None], np.array([[1, 0, 0]], F), None, "radiance", True, False, 0.0)
    assert ok[0] == 1 and rgb[0, 1] > 0 and rgb[0, 0] / (rgb[0, 0] + rgb[0, 1]) < 1e-3
    assert np.array_equal(bits(rgb), bits(pr.lookup_vis(g, res, depth, q[None], np.array([[1, 0, 0]], F), None, "radiance")[0]))
    # a query on the probe's own side, nearer than the probe usually sees that way: exactly 1
    for probe, x in ((0, -0.5), (0, -1.75), (1, 0.25), (1, 2.5)):
        v = np.array([x, 0.1, -0.05], F) - np.array([(-1.0, 1.0)[probe], 0, 0], F)
        assert pr.visibility(depth["count"][probe], depth["moments"][probe], R, v) == 1
        assert c_visibility(pkg, depth, probe, v[None])[0] == 1
