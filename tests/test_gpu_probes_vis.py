"""Probe visibility on the device (include/mi355rt.h "PROBE VISIBILITY"): the depth film of a probe gather, and the weighted grid lookup.

The yardstick is the statement (raytracer_rs_amd.probes, numpy f32) over entries that are pinned elsewhere: probes_gather_depth must equal
gather.rays(normals=None) -> trace_rays(rgb, tuv, prim) -> probes.project / probes.project_depth on every bit, and probes_lookup_vis must equal
probes.lookup_vis on every bit, on the hand-made films and queries of tests/test_probes_vis_abi.py (tests/probe_vis_cases.py) and on a grid that
probes_gather_depth filled.  The lookup is arithmetic: its queries include NaN and infinite coordinates.  No test feeds a non-finite position to a tracing
call."""
import ctypes as C
import importlib

import numpy as np
import pytest

import probe_cases as pc
import probe_vis_cases as pv

pytestmark = pytest.mark.gpu

W = H = 16
SEED = 5
MISS = 0xFFFFFFFF
E_INVALID = -1
SH = ("n", "hits", "near", "sh")
ALL = SH + ("count", "moments")
F = np.float32
SENTINEL = 0xA5A5A5A5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pr(pkg):
    return importlib.import_module("raytracer_rs_amd.probes")


@pytest.fixture(scope="module")
def ga(pkg):
    return importlib.import_module("raytracer_rs_amd.gather")


@pytest.fixture(scope="module")
def cams(pkg):
    return importlib.import_module("raytracer_rs_amd.cameras")


def make(pkg, scene, w=W, h=H, **kw):
    kw.setdefault("seed", SEED)
    return pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, **kw)


@pytest.fixture(scope="module")
def handles(pkg, scenes):
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = make(pkg, scenes(name), **kw)
        return made[key]
    yield get
    for rt in made.values():
        rt.close()


_POINTS = {}


def probe_points(pkg, cams, scenes, name):
    """(points, ids, surface points, normals): free-space points around the camera first, then points 0.05 off the scene's surfaces (the hit points of the
    camera's rays moved along the face normal turned against the ray), and random ids with repeats; computed once per scene and never written to"""
    if name not in _POINTS:
        sc = scenes(name)
        rt = make(pkg, sc, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
        origin = rt.camera.matrices()[1][12:15]
        rays = cams.pinhole(rt.camera.matrices(), W, H, 8, SEED)
        tuv, prim = rt.intersect_rays(rays)
        rt.close()
        hit = np.nonzero(prim != MISS)[0]
        hit = hit[np.random.default_rng(2).permutation(hit.size)][:280]
        assert hit.size >= 257
        o, d, t = rays[hit, :3], rays[hit, 3:], tuv[hit, 0]
        on = (o + t[:, None] * d).astype(F)
        v = sc["tri_verts"][prim[hit]].astype(np.float64)
        n = np.cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
        n /= np.linalg.norm(n, axis=1)[:, None]
        n[(n * d).sum(axis=1) > 0] *= -1
        n = n.astype(F)
        free = origin[None] + np.array([[0, 0, 0], [0.1, 0.2, -0.1], [-0.3, 0.1, 0.2], [0.05, -0.2, 0.3], [0.2, 0.2, 0.2]], F)
        pts = np.concatenate([free, on + F(0.05) * n]).astype(F)
        ids = np.random.default_rng(4).integers(0, 2**32, len(pts), dtype=np.uint64).astype(np.uint32)
        ids[1::7] = ids[0]                                   # repeats
        res = (np.ascontiguousarray(pts), ids, np.ascontiguousarray(on), np.ascontiguousarray(n))
        assert np.isfinite(pts).all()
        for a in res:
            a.setflags(write=False)
        _POINTS[name] = res
    return _POINTS[name]


def traced(rt, ga, pts, ids, first, spp):
    """gather.rays(normals=None) -> trace_rays: (directions, t, hit, rgb)"""
    rays, keys, valid, w = ga.rays(rt.sample_table(), SEED, pts, None, ids, first, spp)
    assert valid.all()
    got = rt.trace_rays(rays, keys, want=("rgb", "tuv", "prim"))
    return rays[:, 3:], got["tuv"][:, 0], got["prim"] != MISS, got["rgb"]


def statement(rt, ga, pr, pts, ids, first, spp, R, D, near=np.inf, prev=None):
    """... -> probes.project and probes.project_depth"""
    d, t, hit, rgb = traced(rt, ga, pts, ids, first, spp)
    res = pr.project(rgb, t, hit, d, len(pts), near, prev)
    res.update(pr.project_depth(t, hit, d, len(pts), R, D, prev))
    return res


def same(got, want, keys=ALL):
    for k in keys:
        assert tuple(got[k].shape) == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


# lanes per point R * R: 9 lanes put 7 points in a wave but for one lane and 28 in a block but for four; at R = 8 a point is a wave, four a block; at R = 16 a
# point is a block
SHAPES = [(3, 1), (3, 7), (3, 8), (3, 28), (3, 29), (3, 64), (3, 257), (8, 1), (8, 3), (8, 4), (8, 5), (8, 257), (16, 1), (16, 2), (16, 17), (2, 1), (2, 65)]


# ---- 1. the statement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4boxes", "ico3_tex"])
def test_probes_gather_depth_equals_the_statement(pkg, ga, pr, cams, scenes, handles, sem3, name):
    pts, ids, _, _ = probe_points(pkg, cams, scenes, name)
    rt = handles(name, flags=sem3.gpu)
    d, t, hit, _ = traced(rt, ga, pts[:257], ids[:257], 0, 8)
    D = float(F(0.8 * np.median(t[hit])))                    # below the median t: the clamp, the miss branch and the plain branch all occur
    assert (hit & (t < F(D))).sum() > 100 and (hit & ~(t < F(D))).sum() > 100 and (~hit).sum() > 100
    near = float(F(0.5 * D))
    k = 0
    for R, npts in SHAPES:
        spp = 1 + k % 8; first = (0, 5, 0xFFFFFFFF - 8, 0xFFFFFFF0 - 3)[k % 4]; k += 1
        p, i = np.ascontiguousarray(pts[:npts]), np.ascontiguousarray(ids[:npts])
        want = statement(rt, ga, pr, p, i, first, spp, R, D, near)
        got = rt.probes_gather_depth(p, i, spp=spp, first_sample=first, near_distance=near, res=R, max_distance=D, want=ALL)
        same(got, want)
        assert got["count"].shape == (npts, R * R) and got["moments"].shape == (npts, R * R, 2) and (got["count"].sum(axis=1) == spp).all()
        assert got["depth_res"] == R and got["max_distance"] == D
        assert rt.last_counts().primary == npts * spp
        # n, hits, near and sh are those of probes_gather on the same points and ids: same samples, same keys
        same(got, rt.probes_gather(p, i, spp=spp, first_sample=first, near_distance=near, want=SH), SH)
        assert rt.last_counts().primary == npts * spp
    big = rt.probes_gather_depth(pts[:257], ids[:257], spp=8, res=8, max_distance=D)
    assert set(big) == {"n", "sh", "count", "moments", "depth_res", "max_distance"}
    m = big["moments"]
    assert (m[..., 0] > 0).sum() > 1000 and (big["count"] == 0).any() and (big["count"] > 1).any()
    assert (m[..., 0] <= big["count"] * F(D) * F(1.0001)).all()                                                 # no distance beyond D
    # ids=None is i; the depth film alone (out NULL) is what it is among all the outputs
    want = statement(rt, ga, pr, pts[:29], None, 2, 3, 8, D)
    same(rt.probes_gather_depth(pts[:29], None, spp=3, first_sample=2, res=8, max_distance=D, want=ALL), want)
    part = rt.probes_gather_depth(pts[:29], np.arange(29, dtype=np.uint32), spp=3, first_sample=2, res=8, max_distance=D, want=("count", "moments"))
    assert set(part) == {"count", "moments", "depth_res", "max_distance"}
    same(part, want, ("count", "moments"))
    same(rt.probes_gather_depth(pts[:29], None, spp=3, first_sample=2, res=8, max_distance=D, want=("moments", "hits", "count")), want, ("hits", "count", "moments"))
    # without the depth film in `want` the call is probes_gather
    only = rt.probes_gather_depth(pts[:29], None, spp=3, first_sample=2, want=("n", "sh"))
    assert set(only) == {"n", "sh"}
    same(only, want, ("n", "sh"))


# ---- 2. chunks, stripes, accumulate ------------------------------------------------------------------------------------------------------------------------
def test_chunks_stripes_and_into(pkg, ga, pr, cams, scenes, handles, sem3):
    """An 8 x 8 handle with samples_per_pass = 1 has passes of 64 rays.  65 points x 3 spp on it: chunks of 64 points and of 1, one sample each.  20 points x 8
    spp: chunks of 3, 3 and 2 samples, in ascending order.  Every output equals the same call on a default handle (one chunk), and a striped handle serves the
    call as an unstriped one does."""
    pts, ids, _, _ = probe_points(pkg, cams, scenes, "4boxes")
    rt = handles("4boxes", flags=sem3.gpu)
    small = make(pkg, scenes("4boxes"), 8, 8, flags=sem3.gpu, samples_per_pass=1)
    striped = make(pkg, scenes("4boxes"), flags=sem3.gpu, stripe_rows=2, stripe_rank=1, stripe_world=3)
    for (npts, spp), R in zip(((65, 3), (20, 8), (64, 1), (130, 2), (7, 8)), (3, 8, 16, 2, 3)):
        p, i = np.ascontiguousarray(pts[:npts]), np.ascontiguousarray(ids[:npts])
        want = rt.probes_gather_depth(p, i, spp=spp, first_sample=1, near_distance=3.0, res=R, max_distance=2.0, want=ALL)
        same(want, statement(rt, ga, pr, p, i, 1, spp, R, 2.0, 3.0))
        for other in (small, striped):
            same(other.probes_gather_depth(p, i, spp=spp, first_sample=1, near_distance=3.0, res=R, max_distance=2.0, want=ALL), want)
            assert other.last_counts().primary == npts * spp
    # into= of 3 + 5 samples equals 8, on the chunked handle and on the default one
    kw = dict(near_distance=3.0, res=8, max_distance=2.0, want=ALL)
    one = rt.probes_gather_depth(pts[:65], ids[:65], spp=8, **kw)
    for h in (small, rt):
        a = h.probes_gather_depth(pts[:65], ids[:65], spp=3, **kw)
        first = {k: (v.copy() if k in ALL else v) for k, v in a.items()}
        b = h.probes_gather_depth(pts[:65], ids[:65], spp=5, first_sample=3, into=a, **kw)
        same(b, one)
        assert all(b[k] is a[k] for k in ALL) and (first["n"] == 3).all() and (first["count"].sum(axis=1) == 3).all() and b["depth_res"] == 8
        # max_distance None: that of `into`
        c = h.probes_gather_depth(pts[:65], ids[:65], spp=5, first_sample=3, near_distance=3.0, res=8, want=ALL, into={k: (v.copy() if k in ALL else v) for k, v in first.items()})
        same(c, one)
        # without `into` the outputs start from 0 whatever they held
        same(h.probes_gather_depth(pts[:65], ids[:65], spp=3, **kw), first)
    with pytest.raises(ValueError, match="into"):
        rt.probes_gather_depth(pts[:65], ids[:65], spp=1, res=8, max_distance=2.0, into=dict(n=one["n"], sh=one["sh"], count=one["count"], moments=one["moments"]))
    with pytest.raises(ValueError, match="into"):
        rt.probes_gather_depth(pts[:65], ids[:65], spp=1, res=4, max_distance=2.0, into=one)
    with pytest.raises(ValueError, match="into"):
        rt.probes_gather_depth(pts[:65], ids[:65], spp=1, res=8, max_distance=2.5, into=one)
    small.close(); striped.close()


# ---- 3. the lookup ---------------------------------------------------------------------------------------------------------------------------------------------
def test_probes_lookup_vis_equals_the_statement(pkg, pr, scenes, handles):
    rt = handles("4boxes")
    counts_before = rt.last_counts().as_dict()
    used = unused = 0
    for k, (name, g, res, depth, usable, pts, dirs, nrm) in enumerate(pv.lookup_cases()):
        full = dict(res, count=depth["count"], moments=depth["moments"], depth_res=depth["res"], max_distance=depth["max_distance"])
        plain, pok = rt.probes_lookup(g, res, pts, dirs, "irradiance", usable, want_ok=True)
        for c, (cheb, facing) in enumerate(pv.FLAGS):
            mode = ("radiance", "irradiance")[(k + c) % 2]
            for normals, bias in ((nrm, 0.0), (nrm, 0.13), (None, 0.0)):
                want, wok = pr.lookup_vis(g, res, depth, pts, dirs, normals, mode, usable, cheb, facing, bias)
                got, gok = rt.probes_lookup_vis(g, full, pts, dirs, normals, mode, usable, cheb, facing, bias, want_ok=True)
                assert got.dtype == F and gok.dtype == np.uint8 and got.shape == want.shape
                assert np.array_equal(gok, wok), (name, cheb, facing, bias)
                assert np.array_equal(bits(got), bits(want)), (name, cheb, facing, bias)
                used += int(wok.sum()); unused += int((wok == 0).sum())
        # the flags-0 call is probes_lookup on every bit
        zero, zok = rt.probes_lookup_vis(g, full, pts, dirs, nrm, "irradiance", usable, False, False, 0.0, want_ok=True)
        assert np.array_equal(bits(zero), bits(plain)) and np.array_equal(zok, pok)
        assert np.array_equal(bits(rt.probes_lookup_vis(g, full, pts, dirs, None, "irradiance", usable, False, True)), bits(plain))     # without normals facing has no effect, and without ok
    assert used > 10000 and unused > 2000
    # the wave and block edges of one lane per query; the NaN and infinite coordinates are among the queries
    g = pc.grid((5, 5, 5)); res = pc.values((5, 5, 5)); depth = pv.film(8, 125, 90)
    full = dict(res, count=depth["count"], moments=depth["moments"], depth_res=8, max_distance=3.0)
    pts, dirs = pc.queries(g, 257)
    nrm = pv.normals(257)
    assert np.isnan(pts).any() and np.isinf(pts).any()
    for m in (1, 63, 64, 65, 257):
        p, d, n = np.ascontiguousarray(pts[:m]), np.ascontiguousarray(dirs[:m]), np.ascontiguousarray(nrm[:m])
        for mode in ("radiance", "irradiance"):
            want, wok = pr.lookup_vis(g, res, depth, p, d, n, mode, None, True, True, 0.05)
            got, gok = rt.probes_lookup_vis(g, full, p, d, n, mode, normal_bias=0.05, want_ok=True)
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(gok, wok), (m, mode)
    assert rt.last_counts().as_dict() == counts_before                               # the lookup traces nothing and reports nothing


def test_lookup_vis_in_a_grid_that_probes_gather_depth_filled(pkg, pr, cams, scenes, handles):
    _, _, on, nrm = probe_points(pkg, cams, scenes, "4boxes")
    rt = handles("4boxes")
    verts = scenes("4boxes")["tri_verts"].reshape(-1, 3)
    g = pr.grid_over(verts.min(axis=0), verts.max(axis=0), (3, 2, 3))
    gp = pr.grid_points(g)
    D = pr.grid_max_distance(g)
    res = rt.probes_gather_depth(gp, spp=8, near_distance=0.2, res=4, max_distance=D, want=ALL)
    assert (res["n"] == 8).all() and res["sh"].any() and (res["count"].sum(axis=1) == 8).all() and res["max_distance"] == D
    depth = dict(res=4, max_distance=D, count=res["count"], moments=res["moments"])
    usable = pr.usable(res, 0.25)
    differs = 0
    for mask in (None, usable):
        plain = rt.probes_lookup(g, res, on, nrm, "irradiance", mask)
        for cheb, facing in pv.FLAGS:
            for bias in (0.0, 0.2 * float(g["spacing"].min())):
                want, wok = pr.lookup_vis(g, res, depth, on, nrm, nrm, "irradiance", mask, cheb, facing, bias)
                got, gok = rt.probes_lookup_vis(g, res, on, nrm, nrm, "irradiance", mask, cheb, facing, bias, want_ok=True)
                assert np.array_equal(bits(got), bits(want)) and np.array_equal(gok, wok), (cheb, facing, bias)
                assert wok.any() and want[wok == 1].any()
                if cheb or facing:
                    differs += int((bits(got) != bits(plain)).any())
                else:
                    assert np.array_equal(bits(got), bits(plain))
    assert differs == 12                                                              # the weights change the answer in this scene


# ---- 4. device memory, and what the calls leave alone ----------------------------------------------------------------------------------------------------
def test_device_tensors_and_an_untouched_handle(pkg, ga, pr, cams, scenes, sem3):
    import torch
    pts, ids, on, nrm = probe_points(pkg, cams, scenes, "4boxes")
    rt = make(pkg, scenes("4boxes"), flags=sem3.gpu | pkg.FLAG_DIRECT_FILM | pkg.FLAG_LIGHT_FILMS)
    rt.set_lens("thin", radius=0.05, focus=4.0)
    rt.render(2)
    s, q, n = rt.film.pixel_datas()
    before = (bits(s).copy(), bits(q).copy(), n.copy(), bits(rt.film.direct_sums()).copy(), bits(rt.light_films.get()).copy())
    row, cam, lens = rt.current_row, [a.copy() for a in rt.camera.matrices()], rt.lens.as_dict()
    p, i = np.ascontiguousarray(pts[:130]), np.ascontiguousarray(ids[:130])
    kw = dict(near_distance=3.0, res=8, max_distance=2.0, want=ALL)
    host = rt.probes_gather_depth(p, i, spp=3, **kw)
    dev = torch.device("cuda", 0)
    tp, ti = torch.from_numpy(p.copy()).to(dev), torch.from_numpy(i.copy().view(np.int32)).to(dev)
    got = rt.probes_gather_depth(tp, ti, spp=3, **kw)
    hbm = rt.hbm_allocated_bytes()
    got = rt.probes_gather_depth(tp, ti, spp=3, **kw)
    assert rt.hbm_allocated_bytes() == hbm                                            # every temporary, the chunk's bins among them, is freed and counted
    for k in ALL:
        assert isinstance(got[k], torch.Tensor) and got[k].device == dev
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), host[k].view(np.uint32)), k
    assert got["count"].dtype == torch.int32 and tuple(got["moments"].shape) == (130, 64, 2)
    # in place on the device: accumulate into tensors
    a = rt.probes_gather_depth(tp, ti, spp=1, **kw)
    b = rt.probes_gather_depth(tp, ti, spp=2, first_sample=1, into=a, **kw)
    assert all(b[k] is a[k] for k in ALL)
    for k in ALL:
        assert np.array_equal(b[k].cpu().numpy().view(np.uint32), host[k].view(np.uint32)), k
    rt.probes_gather_depth(p, i, spp=3, **kw)
    assert rt.hbm_allocated_bytes() == hbm
    # the lookup on tensors, in place
    counts_before = rt.last_counts().as_dict()
    g = pc.grid((5, 5, 5)); res = pc.values((5, 5, 5)); depth = pv.film(16, 125, 91)
    full = dict(res, count=depth["count"], moments=depth["moments"], depth_res=16, max_distance=3.0)
    qp, qd = pc.queries(g, 257)
    qn = pv.normals(257)
    mask = (np.arange(125) % 3 != 0).astype(np.uint8)
    want, wok = rt.probes_lookup_vis(g, full, qp, qd, qn, "irradiance", mask, normal_bias=0.1, want_ok=True)
    assert np.array_equal(bits(want), bits(pr.lookup_vis(g, res, depth, qp, qd, qn, "irradiance", mask, True, True, 0.1)[0]))
    t = lambda a: torch.from_numpy(a.copy()).to(dev)
    tfull = dict(n=t(res["n"].view(np.int32)), sh=t(res["sh"]), count=t(depth["count"].view(np.int32)), moments=t(depth["moments"]), depth_res=16, max_distance=3.0)
    tq, td, tn, tm = t(qp), t(qd), t(qn), t(mask)
    trgb, tok = rt.probes_lookup_vis(g, tfull, tq, td, tn, "irradiance", tm, normal_bias=0.1, want_ok=True)
    assert isinstance(trgb, torch.Tensor) and trgb.device == dev and tok.dtype == torch.uint8
    assert np.array_equal(bits(trgb.cpu().numpy()), bits(want)) and np.array_equal(tok.cpu().numpy(), wok)
    assert rt.hbm_allocated_bytes() == hbm
    assert rt.last_counts().as_dict() == counts_before
    with pytest.raises(ValueError, match="GPU"):
        rt.probes_gather_depth(tp.cpu(), None, max_distance=2.0)
    with pytest.raises(ValueError, match="must live where points live"):
        rt.probes_lookup_vis(g, full, tq, td, tn)
    with pytest.raises(ValueError, match="must live where points live"):
        rt.probes_lookup_vis(g, tfull, tq, td, qn)
    with pytest.raises(ValueError, match="must live where points live"):
        rt.probes_gather_depth(tp, ti, spp=1, into=host, **kw)
    with pytest.raises(TypeError, match="dtype"):
        rt.probes_gather_depth(tp.double(), None, max_distance=2.0)
    # the handle is what it was: film, direct film, light films, current row, camera, lens; the caller-ray mark is not set (the denoiser still answers)
    s, q, n = rt.film.pixel_datas()
    after = (bits(s), bits(q), n, bits(rt.film.direct_sums()), bits(rt.light_films.get()))
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert rt.current_row == row and rt.lens.as_dict() == lens
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(cam, rt.camera.matrices()))
    rt.get_denoised_pixels()
    # ... and the next samples of the film are the ones it would have taken without the calls
    twin = make(pkg, scenes("4boxes"), flags=sem3.gpu | pkg.FLAG_DIRECT_FILM | pkg.FLAG_LIGHT_FILMS)
    twin.set_lens("thin", radius=0.05, focus=4.0)
    twin.render(2); twin.render(1); rt.render(1)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(rt.film.pixel_datas()[:2], twin.film.pixel_datas()[:2]))
    rt.close(); twin.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
GUARD = 4
R0 = 3


def raw_gather(pkg, rt, points, ids, npoints, want=ALL, where=0, null_cfg=False, null_depth=False, null_out=False, res=R0, max_distance=2.0, **cfg_kw):
    """mi355rt_probes_gather_depth through ctypes into sentinel-filled outputs; returns (code, {name: uint32 array})"""
    cfg = pkg.ProbeConfig()
    pkg.lib().mi355rt_probes_default_config(C.byref(cfg))
    cfg.spp = 2
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    per = {"sh": 27, "count": R0 * R0, "moments": R0 * R0 * 2}
    o, d, arrs = pkg.ProbeOutputs(), pkg.ProbeDepth(res, max_distance, None, None), {}
    for w in want:
        arrs[w] = np.full((npoints + GUARD) * per.get(w, 1), SENTINEL, np.uint32)
        setattr(d if w in ("count", "moments") else o, w, arrs[w].ctypes.data)
    ptr = lambda a: None if a is None else a.ctypes.data
    code = pkg.lib().mi355rt_probes_gather_depth(rt._h, ptr(points), ptr(ids), npoints, None if null_cfg else C.byref(cfg), where, None if null_out else C.byref(o),
                                                 None if null_depth else C.byref(d))
    return code, arrs


def raw_lookup(pkg, rt, grid, res, depth, points, dirs, normals, npoints, mode=0, where=0, usable=None, null=(), flags=3, bias=0.0, null_vc=False, d_res=None, d_max=None):
    """mi355rt_probes_lookup_vis through ctypes into sentinel-filled outputs; null: names of arguments passed as NULL; returns (code, rgb words, ok bytes)"""
    g = None if grid is None else (grid if isinstance(grid, pkg.ProbeGrid) else pkg.ProbeGrid.from_dict(grid))
    rgb = np.full((npoints + GUARD) * 3, SENTINEL, np.uint32); ok = np.full(npoints + GUARD, 0xA5, np.uint8)
    ptr = lambda name, a: None if (a is None or name in null) else a.ctypes.data
    d = pkg.ProbeDepth(int(depth["res"]), float(depth["max_distance"]), ptr("count", depth["count"]), ptr("moments", depth["moments"]))
    if d_res is not None:
        d.res = d_res
    if d_max is not None:
        d.max_distance = d_max
    vc = pkg.ProbeVisConfig(flags, bias)
    code = pkg.lib().mi355rt_probes_lookup_vis(rt._h, None if g is None else C.byref(g), ptr("n", res["n"]), ptr("sh", res["sh"]), ptr("usable", usable),
                                               None if "depth" in null else C.byref(d), None if null_vc else C.byref(vc), ptr("points3", points), ptr("dirs3", dirs),
                                               ptr("normals3", normals), npoints, mode, where, ptr("rgb3", rgb), ptr("ok", ok))
    return code, rgb, ok


def test_refusals_name_the_argument_and_write_nothing(pkg, pr, cams, scenes):
    pts, ids, _, _ = probe_points(pkg, cams, scenes, "4boxes")
    p, i = np.ascontiguousarray(pts[:10]), np.ascontiguousarray(ids[:10])
    rt = make(pkg, scenes("4boxes"))
    rt.render(1)
    s, q, cnt = rt.film.pixel_datas()
    film = (bits(s).copy(), bits(q).copy(), cnt.copy())
    lib = pkg.lib()
    err = lambda h=rt: (lib.mi355rt_last_error(h._h) or b"").decode()

    def film_untouched():
        s2, q2, n2 = rt.film.pixel_datas()
        assert np.array_equal(bits(s2), film[0]) and np.array_equal(bits(q2), film[1]) and np.array_equal(n2, film[2])

    def refused(result, *names):
        code, arrs = result
        assert code == E_INVALID
        assert "mi355rt_probes_gather_depth" in err() and all(nm in err() for nm in names), err()
        assert all(np.all(v == SENTINEL) for v in arrs.values())
        film_untouched()

    refused(raw_gather(pkg, rt, None, i, 10), "points3")
    refused(raw_gather(pkg, rt, p, i, 10, want=("count", "moments")), "out")                         # an `out` without a pointer; NULL would have been fine
    refused(raw_gather(pkg, rt, p, i, 10, null_cfg=True), "cfg")
    refused(raw_gather(pkg, rt, p, i, 10, null_depth=True), "depth")
    refused(raw_gather(pkg, rt, p, i, 10, want=SH + ("moments",)), "count")
    refused(raw_gather(pkg, rt, p, i, 10, want=SH + ("count",)), "moments")
    for bad in (0, 1, 17, 2**32 - 1):
        refused(raw_gather(pkg, rt, p, i, 10, res=bad), "res")
    for bad in (0.0, -2.0, float("nan"), float("inf"), 1.0001e12):
        refused(raw_gather(pkg, rt, p, i, 10, max_distance=bad), "max_distance")
    refused(raw_gather(pkg, rt, p, i, 10, spp=0), "spp")
    refused(raw_gather(pkg, rt, p, i, 10, where=2), "where")
    refused(raw_gather(pkg, rt, p, i, 10, near_distance=float("nan")), "near_distance")
    refused(raw_gather(pkg, rt, p, i, 10, spp=2**32 // 10 + 1), "npoints * spp")
    refused(raw_gather(pkg, rt, p, i, 10, spp=3, first_sample=0xFFFFFFFE), "first_sample")
    # what is allowed right at those edges: out NULL, max_distance 1e12, the last sample numbers; the guard behind every output stays
    code, arrs = raw_gather(pkg, rt, p, i, 10, want=("count", "moments"), null_out=True, max_distance=1e12, spp=2, first_sample=0xFFFFFFFD)
    assert code == 0 and (arrs["count"][:90].reshape(10, 9).sum(axis=1) == 2).all() and (arrs["count"][90:] == SENTINEL).all()
    assert not (arrs["moments"][:180] == SENTINEL).any() and (arrs["moments"][180:] == SENTINEL).all()
    code, arrs = raw_gather(pkg, rt, p, None, 10, spp=1)
    per = {"sh": 27, "count": 9, "moments": 18}
    assert code == 0 and all((v[10 * per.get(k, 1):] == SENTINEL).all() and not (v[:10 * per.get(k, 1)] == SENTINEL).any() for k, v in arrs.items())
    # npoints == 0 succeeds and writes nothing, with or without pointers
    code, arrs = raw_gather(pkg, rt, p, i, 0)
    assert code == 0 and all(np.all(v == SENTINEL) for v in arrs.values())
    code, arrs = raw_gather(pkg, rt, None, None, 0, want=("count", "moments"), null_out=True)
    assert code == 0 and all(np.all(v == SENTINEL) for v in arrs.values())
    empty = rt.probes_gather_depth(np.zeros((0, 3), F), res=4, max_distance=1.0)
    assert empty["moments"].shape == (0, 16, 2) and empty["sh"].shape == (0, 9, 3)

    # ---- the lookup
    g = pc.grid((4, 3, 2)); res = pc.values((4, 3, 2)); depth = pv.film(3, 24, 92)
    qp, qd = pc.queries(g, 10)
    qn = pv.normals(10)

    def lrefused(result, *names):
        code, rgb, ok = result
        assert code == E_INVALID
        assert "mi355rt_probes_lookup_vis" in err() and all(nm in err() for nm in names), err()
        assert np.all(rgb == SENTINEL) and np.all(ok == 0xA5)
        film_untouched()

    def grid_with(field, value):
        b = pkg.ProbeGrid.from_dict(g)
        for a in range(3):
            getattr(b, field)[a] = value[a]
        return b

    lrefused(raw_lookup(pkg, rt, None, res, depth, qp, qd, qn, 10), "grid")
    lrefused(raw_lookup(pkg, rt, grid_with("counts", (4, 0, 2)), res, depth, qp, qd, qn, 10), "counts")
    lrefused(raw_lookup(pkg, rt, grid_with("counts", (2048, 2048, 512)), res, depth, qp, qd, qn, 10), "counts", "2^31")
    lrefused(raw_lookup(pkg, rt, grid_with("spacing", (0.7, 0.0, 0.9)), res, depth, qp, qd, qn, 10), "spacing")
    lrefused(raw_lookup(pkg, rt, grid_with("origin", (float("nan"), 0.0, 0.0)), res, depth, qp, qd, qn, 10), "origin")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("n",)), "n is NULL")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("sh",)), "sh")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("depth",)), "depth")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("count",)), "count")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("moments",)), "moments")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, d_res=1), "res")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, d_res=17), "res")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, d_max=float("nan")), "max_distance")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, d_max=0.0), "max_distance")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null_vc=True), "vc")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, flags=4), "flags")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, bias=float("nan")), "normal_bias")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, bias=float("-inf")), "normal_bias")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("normals3",), flags=2), "MI355RT_VIS_FACING", "normals3")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("normals3",), flags=1, bias=0.1), "normal_bias", "normals3")
    code, rgb, ok = raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("rgb3",))
    assert code == E_INVALID and "rgb3" in err() and np.all(ok == 0xA5)
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("points3",)), "points3")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("dirs3",)), "dirs3")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, mode=2), "mode")
    lrefused(raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, where=2), "where")
    # what is allowed: ok, usable and normals NULL (with CHEBYSHEV alone), npoints == 0 (nothing written), and the guard behind the outputs stays
    code, rgb, ok = raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, null=("ok", "normals3"), flags=1)
    assert code == 0 and np.all(ok == 0xA5) and np.all(rgb[30:] == SENTINEL)
    assert np.array_equal(rgb[:30], bits(pr.lookup_vis(g, res, depth, qp, qd, None, "radiance", None, True, False)[0]).reshape(-1))
    code, rgb, ok = raw_lookup(pkg, rt, g, res, depth, qp, qd, qn, 10, mode=1, bias=0.25)
    want, wok = pr.lookup_vis(g, res, depth, qp, qd, qn, "irradiance", None, True, True, 0.25)
    assert code == 0 and np.array_equal(ok[:10], wok) and np.all(ok[10:] == 0xA5) and np.array_equal(rgb[:30], bits(want).reshape(-1)) and np.all(rgb[30:] == SENTINEL)
    code, rgb, ok = raw_lookup(pkg, rt, g, res, depth, None, None, None, 0, flags=1)
    assert code == 0 and np.all(rgb == SENTINEL) and np.all(ok == 0xA5)
    # the Python face
    full = dict(res, count=depth["count"], moments=depth["moments"], depth_res=3, max_distance=3.0)
    with pytest.raises(ValueError, match="want"):
        rt.probes_gather_depth(p, want=("sum",), max_distance=1.0)
    with pytest.raises(ValueError, match="together"):
        rt.probes_gather_depth(p, want=("n", "count"), max_distance=1.0)
    with pytest.raises(ValueError, match="max_distance"):
        rt.probes_gather_depth(p)
    with pytest.raises(ValueError, match="max_distance"):
        rt.probes_gather_depth(p, max_distance=float("inf"))
    with pytest.raises(ValueError, match="res"):
        rt.probes_gather_depth(p, res=1, max_distance=1.0)
    with pytest.raises(RuntimeError, match="spp"):
        rt.probes_gather_depth(p, spp=0, max_distance=1.0)
    with pytest.raises(ValueError, match="mode"):
        rt.probes_lookup_vis(g, full, qp, qd, qn, mode="sine")
    with pytest.raises(ValueError, match="shape"):
        rt.probes_lookup_vis(g, dict(full, moments=depth["moments"][:5]), qp, qd, qn)
    with pytest.raises(ValueError, match="count"):
        rt.probes_lookup_vis(g, res, qp, qd, qn)
    with pytest.raises(RuntimeError, match="normal_bias"):
        rt.probes_lookup_vis(g, full, qp, qd, None, normal_bias=0.1)
    rt.get_denoised_pixels()
    rt.close()
    # a device group (here: two members sharing the one GPU) refuses both
    grp = make(pkg, scenes("4boxes"), device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    code, arrs = raw_gather(pkg, grp, p, i, 10)
    assert code == E_INVALID and "device group" in err(grp) and "mi355rt_probes_gather_depth" in err(grp) and all(np.all(v == SENTINEL) for v in arrs.values())
    code, rgb, ok = raw_lookup(pkg, grp, g, res, depth, qp, qd, qn, 10)
    assert code == E_INVALID and "device group" in err(grp) and "mi355rt_probes_lookup_vis" in err(grp) and np.all(rgb == SENTINEL) and np.all(ok == 0xA5)
    grp.close()
