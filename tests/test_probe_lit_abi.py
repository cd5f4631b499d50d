"""Probe-lit shading without a GPU (include/mi355rt.h "PROBE-LIT"): the entry points and structs are what the header says, the host side of the
shared arithmetic (mi355rt_probe_lit_one: csrc/probe_lit_math.hpp, the header the kernels compile) equals the numpy statement (raytracer_rs_amd.probe_lit) bit
for bit, and the statement itself is held to the lookup it restates, to the analytic hemisphere mean of a band-limited field, and — its shade() — to the CPU
oracle's root light sum.  tests/test_gpu_probe_lit.py runs the kernels against the same statement."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import probe_lit_cases as plc
import probe_vis_cases as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_probe_lit_points", "mi355rt_probe_lit_rays", "mi355rt_probe_lit_one"]
F = np.float32
FP = plc.FP
bits = plc.bits
fp = lambda a: a.ctypes.data_as(FP)


@pytest.fixture(scope="module")
def plit(pkg):
    return importlib.import_module("raytracer_rs_amd.probe_lit")


@pytest.fixture(scope="module")
def pr(pkg):
    return importlib.import_module("raytracer_rs_amd.probes")


@pytest.fixture(scope="module")
def ga(pkg):
    return importlib.import_module("raytracer_rs_amd.gather")


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


# ---- symbols, structs, the constant ---------------------------------------------------------------------------------------------------------------------------
def test_probe_lit_symbols_structs_and_constant(pkg, plit, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert "PROBE-LIT" in header
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)
        assert re.search(r"\b%s\(" % name, header), name
    m = re.search(r"#define\s+MI355RT_PROBE_LIT_CLAMP\s+(\d+)u", header)
    assert m and int(m.group(1)) == 1 == pkg.PROBE_LIT_CLAMP == plit.CLAMP
    assert C.sizeof(pkg.ProbeVolume) == 56 and C.sizeof(pkg.ProbeLitOutputs) == 48
    assert [(n, getattr(pkg.ProbeVolume, n).offset) for n, _ in pkg.ProbeVolume._fields_] == [("grid", 0), ("n", 8), ("sh", 16), ("usable", 24), ("depth", 32), ("vc", 40),
                                                                                              ("offsets", 48)]
    assert [(n, getattr(pkg.ProbeLitOutputs, n).offset) for n, _ in pkg.ProbeLitOutputs._fields_] == [("rgb", 0), ("light", 8), ("indirect", 16), ("tuv", 24), ("prim", 32),
                                                                                                      ("ok", 40)]
    assert tuple(n for n, _ in pkg.ProbeLitOutputs._fields_) == pkg.PROBE_LIT_OUTPUTS == plit.OUTPUTS
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355rt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %u\\n",'
                   'sizeof(mi355rt_probe_volume),sizeof(mi355rt_probe_lit_outputs),offsetof(mi355rt_probe_volume,usable),offsetof(mi355rt_probe_volume,depth),'
                   'offsetof(mi355rt_probe_volume,offsets),offsetof(mi355rt_probe_lit_outputs,tuv),offsetof(mi355rt_probe_lit_outputs,ok),MI355RT_PROBE_LIT_CLAMP);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [56, 48, 24, 32, 48, 24, 40, 1]
    lib = pkg.lib()
    # NULL handles
    assert lib.mi355rt_probe_lit_points(None, None, None, None, 0, 0, 0, None, None) == -1
    assert lib.mi355rt_probe_lit_rays(None, None, None, 0, 0, 0, None) == -1
    for name in ("probe_lit_points", "probe_lit_rays", "render_probe_lit"):
        assert callable(getattr(pkg.RayTracer, name))


# ---- every refusal of mi355rt_probe_lit_one -------------------------------------------------------------------------------------------------------------------
def test_probe_lit_one_refusals(pkg, plit):
    lib = pkg.lib()
    err = lambda: lib.mi355rt_last_error(None).decode()
    name, g, res, depth, usable, pts, dirs, nrm = pv.lookup_cases()[2]
    good = plit.volume(g, res, depth=depth, usable=usable, offsets=plc.offsets_for(g, "seeded"))
    p, n = np.ascontiguousarray(pts[0]), np.ascontiguousarray(nrm[0])
    out = np.full(3, 7.0, F); ok = C.c_uint32(99)

    def refused(v, msg, point=p, normal=n, flags=1, indirect=out):
        code = lib.mi355rt_probe_lit_one(None if v is None else C.byref(v), None if point is None else fp(point), None if normal is None else fp(normal), flags,
                                         None if indirect is None else fp(indirect), C.byref(ok))
        assert code == -1 and err() == "mi355rt_probe_lit_one: " + msg, (code, err(), msg)
        assert (out == 7.0).all() and ok.value == 99                                   # nothing written

    v, keep = plc.c_volume(pkg, good)
    assert lib.mi355rt_probe_lit_one(C.byref(v), fp(p), fp(n), 1, fp(out), None) == 0 and not (out == 7.0).any()      # the good call, ok NULL
    out[:] = 7.0
    refused(None, "volume is NULL")

    def broken(**kw):
        b, k = plc.c_volume(pkg, good)
        for key, val in kw.items():
            setattr(b, key, val)
        return b, k

    b, k = broken(); b.grid = None
    refused(b, "grid is NULL")
    for field, value, msg in (("counts", (0, 1, 1), "grid.counts: a count is 0"), ("counts", (2048, 2048, 512), "grid.counts: the product must be < 2^31"),
                              ("spacing", (1.0, 0.0, 1.0), "grid.spacing must be finite and positive"), ("spacing", (1.0, np.inf, 1.0), "grid.spacing must be finite and positive"),
                              ("origin", (np.nan, 0.0, 0.0), "grid.origin must be finite")):
        gg = pkg.ProbeGrid.from_dict(dict(g, **{field: value}))
        b, k = broken(grid=C.pointer(gg))
        refused(b, msg)
    refused(broken(n=None)[0], "volume.n is NULL")
    refused(broken(sh=None)[0], "volume.sh is NULL")
    for R in (1, 17):
        d = pkg.ProbeDepth(R, 3.0, depth["count"].ctypes.data, depth["moments"].ctypes.data)
        refused(broken(depth=C.pointer(d))[0], "depth.res must be 2 .. 16")
    for D in (0.0, np.nan, np.inf, 2e12):
        d = pkg.ProbeDepth(int(depth["res"]), D, depth["count"].ctypes.data, depth["moments"].ctypes.data)
        refused(broken(depth=C.pointer(d))[0], "depth.max_distance must be finite, > 0 and <= 1e12")
    d = pkg.ProbeDepth(int(depth["res"]), 3.0, None, depth["moments"].ctypes.data)
    refused(broken(depth=C.pointer(d))[0], "depth.count is NULL")
    d = pkg.ProbeDepth(int(depth["res"]), 3.0, depth["count"].ctypes.data, None)
    refused(broken(depth=C.pointer(d))[0], "depth.moments is NULL")
    b, k = broken(); b.vc = None
    refused(b, "vc is NULL")
    vc = pkg.ProbeVisConfig(4, 0.0)
    refused(broken(vc=C.pointer(vc))[0], "vc.flags: unknown bits (MI355RT_VIS_CHEBYSHEV, MI355RT_VIS_FACING)")
    vc = pkg.ProbeVisConfig(3, np.nan)
    refused(broken(vc=C.pointer(vc))[0], "vc.normal_bias must be finite")
    # depth NULL with vc or offsets given
    b, k = broken(); b.depth = None
    refused(b, "volume.vc is given without volume.depth")
    b, k = broken(); b.depth = None; b.vc = None
    refused(b, "volume.offsets is given without volume.depth")
    for poison in (np.nan, np.inf, -np.inf):
        off = plc.offsets_for(g, "seeded"); off[-1, 2] = poison
        refused(broken(offsets=off.ctypes.data)[0], "volume.offsets holds a value that is not finite")
    for flags in (2, 3, 0x80000000):
        refused(v, "flags: unknown bits (MI355RT_PROBE_LIT_CLAMP)", flags=flags)
    refused(v, "point is NULL", point=None)
    refused(v, "normal is NULL", normal=None)
    refused(v, "indirect is NULL", indirect=None)
    # the statement's volume() refuses offsets without depth too
    with pytest.raises(ValueError, match="offsets"):
        plit.volume(g, res, offsets=plc.offsets_for(g, "zero"))


# ---- mi355rt_probe_lit_one against probe_lit.hemi, bit for bit ----------------------------------------------------------------------------------------------
def test_probe_lit_one_equals_hemi_on_every_lookup_case(pkg, plit):
    vols = plc.lookup_volumes(plit)
    assert len(vols) == len(pv.lookup_cases()) * 13
    used = unused = negative = 0
    for name, vol, pts, nrm in vols:
        for clamp in (True, False):
            want, got = plit.hemi(vol, pts, nrm, clamp), plc.c_hemi(pkg, vol, pts, nrm, clamp)
            assert same(got, want), (name, clamp)
            if clamp:
                assert not (want[0] < 0).any() and not np.isnan(want[0]).any() and not np.signbit(want[0]).any(), name
            else:
                negative += int((want[0] < 0).any(axis=1).sum())
        used += int(want[1].sum()); unused += int((want[1] == 0).sum())
        assert (want[0][want[1] == 0] == 0).all()
    assert used > 10000 and unused > 1000 and negative > 1000


def test_hemi_without_depth_has_lookups_weights(pkg, plit, pr):
    """without depth films the corner weights are LOOKUP's t_j: hemi with clamp off equals a lookup whose read-out is re-made here from lookup's own corner sums"""
    for name, g, res, depth, usable, pts, dirs, nrm in pv.lookup_cases():
        vol = plit.volume(g, res, usable=usable)
        a = plit.hemi(vol, pts, nrm, False)
        b = plit.hemi(plit.volume(g, res, depth=depth, usable=usable, chebyshev=False, facing=False, normal_bias=0.3, offsets=plc.offsets_for(g, "seeded")), pts, nrm, False)
        assert same(a, b), name                                                       # no position is made: the offsets and the bias change nothing
        _, ok = pr.lookup(g, res, pts, nrm, "radiance", usable)
        assert np.array_equal(ok, a[1]), name


def rich_case(plit):
    """the first lookup case with at least 8 probes most of whose queries use a corner"""
    for case in pv.lookup_cases():
        name, g, res, depth, usable, pts, dirs, nrm = case
        if len(res["n"]) >= 8 and plit.hemi(plit.volume(g, res, depth=depth, usable=usable), pts, nrm)[1].sum() > 150:
            return case
    raise AssertionError("no such case")


def poisoned(vol, **kw):
    v = dict(vol)
    v["sh"] = np.array(vol["sh"], F, copy=True)
    v.update(kw)
    return v


def test_hemi_reads_four_coefficients_and_no_skipped_corner(pkg, plit):
    name, g, res, depth, usable, pts, dirs, nrm = rich_case(plit)
    vol = plit.volume(g, res, depth=depth, usable=usable, offsets=plc.offsets_for(g, "seeded"))
    for clamp in (True, False):
        base = plit.hemi(vol, pts, nrm, clamp)
        assert same(plc.c_hemi(pkg, vol, pts, nrm, clamp), base)
        # an infinity and a NaN in coefficients 4 .. 8: unchanged
        hi = poisoned(vol)
        hi["sh"][:, 4:, :] = np.inf; hi["sh"][::2, 5, :] = np.nan; hi["sh"][1::3, 8, 1] = -np.inf
        assert same(plit.hemi(hi, pts, nrm, clamp), base) and same(plc.c_hemi(pkg, hi, pts, nrm, clamp), base)
        # an infinity in a skipped corner (n == 0, or not usable): unchanged
        n = np.array(vol["n"], np.uint32, copy=True)
        use = np.ones(len(n), np.uint8) if vol["usable"] is None else np.array(vol["usable"], np.uint8, copy=True)
        skip = (n == 0) | (use == 0)
        if skip.sum() < 2:
            use[[0, len(n) - 1]] = 0; skip = (n == 0) | (use == 0)
            base = plit.hemi(poisoned(vol, usable=use), pts, nrm, clamp)
        sk = poisoned(vol, usable=use)
        sk["sh"][skip] = np.inf
        assert same(plit.hemi(sk, pts, nrm, clamp), base) and same(plc.c_hemi(pkg, sk, pts, nrm, clamp), base)
    # a NaN in a used coefficient: 0 clamped, NaN unclamped
    bad = poisoned(vol)
    bad["sh"][:, 2, 1] = np.nan
    on, off = plit.hemi(bad, pts, nrm, True), plit.hemi(bad, pts, nrm, False)
    used = on[1] == 1
    assert used.sum() > 50 and np.isnan(off[0][used, 1]).all() and (bits(on[0][used, 1]) == 0).all()
    assert np.array_equal(bits(on[0][:, [0, 2]]), bits(plit.hemi(vol, pts, nrm, True)[0][:, [0, 2]]))      # the other channels do not see it
    assert same(plc.c_hemi(pkg, bad, pts, nrm, True), on) and same(plc.c_hemi(pkg, bad, pts, nrm, False), off)
    # a query whose unclamped value is negative: clamped to +0
    neg = poisoned(vol)
    neg["sh"][:, 0, :] = -np.abs(neg["sh"][:, 0, :]) - F(1.0); neg["sh"][:, 1:4, :] = 0.0
    on, off = plit.hemi(neg, pts, nrm, True), plit.hemi(neg, pts, nrm, False)
    used = on[1] == 1
    assert (off[0][used] < 0).all() and (bits(on[0]) == 0).all()
    assert same(plc.c_hemi(pkg, neg, pts, nrm, True), on) and same(plc.c_hemi(pkg, neg, pts, nrm, False), off)
    # every corner unusable: ok 0, indirect 0
    none = poisoned(vol, usable=np.zeros(len(vol["n"]), np.uint8))
    for clamp in (True, False):
        got = plit.hemi(none, pts, nrm, clamp)
        assert (got[1] == 0).all() and (bits(got[0]) == 0).all() and same(plc.c_hemi(pkg, none, pts, nrm, clamp), got)


def test_hemi_is_the_irradiance_lookup_with_other_band_factors(pkg, plit, pr, monkeypatch):
    """hemi with clamp off equals probes.lookup_placed(mode="irradiance") run with the band factors (1, 1/2, 1/2, 1/2, 0, ...) in the place of the cosine lobe's:
    by value on finite inputs, a zero's sign excepted"""
    monkeypatch.setattr(pr, "A", (F(1.0), F(0.5), F(0.5), F(0.5), F(0.0), F(0.0), F(0.0), F(0.0), F(0.0)))
    checked = 0
    for k, (name, g, res, depth, usable, pts, dirs, nrm) in enumerate(pv.lookup_cases()):
        finite = np.isfinite(pts).all(axis=1)
        p, nr = np.ascontiguousarray(pts[finite]), np.ascontiguousarray(nrm[finite])
        for kind in (None, "seeded"):
            off = plc.offsets_for(g, kind, 9 + k)
            for cheb, facing in pv.FLAGS:
                want, wok = pr.lookup_placed(g, res, depth, p, nr, nr, "irradiance", usable, cheb, facing, 0.05, off)
                got, gok = plit.hemi(plit.volume(g, res, depth=depth, usable=usable, offsets=off, chebyshev=cheb, facing=facing, normal_bias=0.05), p, nr, False)
                assert np.array_equal(wok, gok) and np.isfinite(want).all(), name
                assert np.array_equal(want, got), name                                # by value: -0 == +0
                checked += int(gok.sum())
    assert checked > 10000


def test_hemi_of_an_analytic_field(pkg, plit, pr):
    """Every probe of a 2x2x2 grid holds the same band-limited field: n = 4 and sh = 4 c / (4 pi) for fixed-seed c ~ N(0, 1) in all nine coefficients.  The
    uniform hemisphere mean of sum c_k b_k around N is c_0 b_0 + 0.5 sum_{k=1..3} c_k b_k(N) (band factors 1, 1/2, 0), whatever the interpolation weights.
    Measured with numpy: 1.0e-7 at values up to 0.5; the bound 1e-5 leaves two orders for other seeds and still catches any wrong factor (a factor 1 in the
    place of 1/2 in band 1, or a band-2 factor that is not 0, moves the value by 1e-1)."""
    rng = np.random.default_rng(20)
    c = rng.normal(size=(9, 3))
    grid = dict(origin=np.array([-1.0, -1.0, -1.0], F), spacing=np.array([2.0, 2.0, 2.0], F), counts=np.array([2, 2, 2], np.uint32))
    sh = np.broadcast_to(((4.0 * c.astype(F)) / pr.SPHERE).astype(F)[None], (8, 9, 3)).copy()
    res = dict(n=np.full(8, 4, np.uint32), sh=sh)
    pts = rng.uniform(-1.2, 1.2, (2000, 3)).astype(F)
    nrm = rng.normal(size=(2000, 3)); nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm = nrm.astype(F)
    b = pr.basis(nrm).astype(np.float64)
    cq = ((4.0 * c.astype(F)) / pr.SPHERE).astype(F).astype(np.float64) * float(pr.SPHERE) / 4.0          # the coefficients the probes actually hold
    want = cq[0][None, :] * b[:, 0, None] + 0.5 * sum(cq[k][None, :] * b[:, k, None] for k in (1, 2, 3))
    depth = pv.flat_film(4, 8, mean=8.0)                                                 # everything is visible: vis 1
    for vol in (plit.volume(grid, res), plit.volume(grid, res, depth=depth, offsets=plc.offsets_for(grid, "seeded")),
                plit.volume(grid, res, depth=pv.film(8, 8, 3), normal_bias=0.05)):
        got, ok = plit.hemi(vol, pts, nrm, False)
        assert (ok == 1).all()
        err = np.abs(got.astype(np.float64) - want).max()
        print("analytic field: max abs error %.3g at values up to %.3g" % (err, np.abs(want).max()))
        assert err <= 1e-5
        cl, _ = plit.hemi(vol, pts, nrm, True)
        assert np.array_equal(cl, np.where(got >= 0, got, F(0.0)))
        assert same(plc.c_hemi(pkg, vol, pts[:300], nrm[:300], False), (got[:300], ok[:300]))


# ---- probe_lit.shade against the CPU oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", plc.SCENES)
def test_shade_equals_the_oracles_root_light_sum(pkg, oracle, scenes, plit, ga, name):
    """For pixels of the scene take the oracle's primary ray, its hit, its verdict on gather.shadow_rays at the hit point by the reference's rule (a hit with
    0.01 < t < 1 blocks), and shade() must equal node_L[0] of the oracle's sample bit for bit, misses included: the statement is established before any GPU run"""
    sc = plc.scene_of(scenes, name)
    w, h = 24, 18
    orc = oracle.Oracle(sc, w, h, seed=plc.SEED)
    pixels = np.arange(0, w * h, 1 if name != "4boxes" else 1)
    sampleno = 2
    rays = np.stack([orc.primary_ray(int(p), sampleno) for p in pixels]).astype(F)
    tuv, prim = orc.intersect(rays)
    hit = prim != plc.MISS
    assert hit.sum() > 40 and (~hit).sum() > 40
    sr = plit.shadow_rays(sc, rays, tuv, prim)
    P = plit.hit_points(rays[hit], tuv[hit])
    nl = len(sc["lights"])
    assert np.array_equal(bits(sr.reshape(nl, -1, 6)[:, hit]), bits(ga.shadow_rays(P, sc["lights"]).reshape(nl, -1, 6)))      # gather.shadow_rays unchanged
    stuv, sprim = orc.intersect(sr)
    blocked = (sprim != plc.MISS) & (stuv[:, 0] > F(0.01)) & (stuv[:, 0] < F(1.0))
    got = plit.shade(sc, rays, tuv, prim, blocked)
    want = np.stack([orc.sample_debug(int(p), sampleno)[1][0] for p in pixels])
    orc.close()
    assert np.array_equal(bits(got), bits(want))
    assert (bits(got[~hit]) == 0).all() and (got[hit] > 0).any()
    b = blocked.reshape(nl, -1)[:, hit]
    assert b.any() and (~b).any()                                                      # both verdicts occur
    if name == "ico3_tex":
        assert (np.asarray(sc["mat_kind"])[np.asarray(sc["tri_geom"])[prim[hit]]] == 1).any()      # textured hits occur
    # the whole call per ray: rgb is the one addition, misses are zeros and keep their tuv
    name0, g, res, depth, usable, _, _, _ = rich_case(plit)
    vol = plit.volume(g, res, depth=depth, usable=usable)
    before = np.full((len(rays), 3), 7.0, F)
    r = plit.rays(sc, vol, rays, tuv, prim, blocked, True, before)
    assert np.array_equal(bits(r["light"]), bits(want)) and np.array_equal(bits(r["rgb"]), bits(r["light"] + r["indirect"]))
    assert (r["tuv"][~hit] == 7.0).all() and np.array_equal(bits(r["tuv"][hit]), bits(tuv[hit]))
    assert (r["ok"][~hit] == 0).all() and (bits(r["indirect"][~hit]) == 0).all()


def test_frame_mean_is_one_addition_per_sample(plit):
    rng = np.random.default_rng(4)
    npix, spp = 37, 3
    rgb = rng.normal(size=(spp * npix, 3)).astype(F)
    acc = np.zeros((npix, 3), F)
    for s in range(spp):
        acc = acc + rgb[s * npix:(s + 1) * npix]
    assert np.array_equal(bits(plit.frame_mean(rgb, npix)), bits(acc / F(3)))
    assert np.array_equal(bits(plit.frame_mean(rgb[:npix], npix)), bits(rgb[:npix] + F(0.0)))
    with pytest.raises(ValueError):
        plit.frame_mean(rgb[:50], npix)
