"""Probes on the device (include/mi355rt.h "PROBES"): gathered light as SH coefficients, and the grid lookup.

The yardstick is the statement (raytracer_rs_amd.probes, numpy f32) over entries that are pinned elsewhere: probes_gather must equal
gather.rays(normals=None) -> trace_rays(rgb, tuv, prim) -> probes.project on every bit, and probes_lookup must equal probes.lookup on every bit, on the
hand-made grids and queries of tests/test_probes_abi.py (tests/probe_cases.py) and on a grid that probes_gather filled.  The lookup is arithmetic: its
queries include NaN and infinite coordinates.  No test feeds a non-finite position to a tracing call."""
import ctypes as C
import importlib

import numpy as np
import pytest

import probe_cases as pc

pytestmark = pytest.mark.gpu

W = H = 16
SEED = 5
MISS = 0xFFFFFFFF
E_INVALID = -1
ALL = ("n", "hits", "near", "sh")
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


def statement(rt, ga, pr, pts, ids, first, spp, near=np.inf, prev=None):
    """gather.rays(normals=None) -> trace_rays -> probes.project"""
    rays, keys, valid, w = ga.rays(rt.sample_table(), SEED, pts, None, ids, first, spp)
    assert valid.all()
    got = rt.trace_rays(rays, keys, want=("rgb", "tuv", "prim"))
    return pr.project(got["rgb"], got["tuv"][:, 0], got["prim"] != MISS, rays[:, 3:], len(pts), near, prev)


def same(got, want, keys=ALL):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


# ---- 1. the statement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4boxes", "ico3_tex"])
def test_probes_gather_equals_the_statement(pkg, ga, pr, cams, scenes, handles, sem3, name):
    pts, ids, _, _ = probe_points(pkg, cams, scenes, name)
    rt = handles(name, flags=sem3.gpu)
    tuv = rt.intersect_rays(ga.rays(rt.sample_table(), SEED, pts[:257], None, ids[:257], 0, 8)[0])[0]
    near = float(np.median(tuv[:, 0][tuv[:, 0] > 0]))
    big = statement(rt, ga, pr, pts[:257], ids[:257], 0, 8, near)
    # the input decides something: light arrives, rays hit and miss, some hits are near
    assert big["sh"].any() and 0 < big["hits"].sum() < big["n"].sum() and 0 < big["near"].sum() < big["hits"].sum()
    assert big["sh"][:, 1:].any() and (big["sh"] < 0).any()
    k = 0
    for npts in (1, 7, 8, 28, 29, 65, 257):               # 9 lanes per point: 7 points fill a wave but for one lane, 28 a block but for four
        spp = (1, 3, 8)[k % 3]; first = (0, 5, 0xFFFFFFF0)[(k // 2) % 3]; k += 1
        p, i = np.ascontiguousarray(pts[:npts]), np.ascontiguousarray(ids[:npts])
        want = statement(rt, ga, pr, p, i, first, spp, near)
        got = rt.probes_gather(p, i, spp=spp, first_sample=first, near_distance=near, want=ALL)
        same(got, want)
        assert got["sh"].shape == (npts, 9, 3) and (got["n"] == spp).all()
        assert rt.last_counts().primary == npts * spp
        # n, hits and near are those of gather in sphere mode on the same points and ids
        g = rt.gather(p, None, i, spp=spp, first_sample=first, near_distance=near, want=("n", "hits", "near"))
        same(got, g, ("n", "hits", "near"))
    # ids=None is i
    want = statement(rt, ga, pr, pts[:29], None, 2, 3)
    same(rt.probes_gather(pts[:29], None, spp=3, first_sample=2, want=ALL), want)
    same(rt.probes_gather(pts[:29], np.arange(29, dtype=np.uint32), spp=3, first_sample=2, want=ALL), want)
    # only some outputs: each is what it is among all of them
    part = rt.probes_gather(pts[:65], ids[:65], spp=3, first_sample=2, near_distance=near, want=("sh",))
    full = statement(rt, ga, pr, pts[:65], ids[:65], 2, 3, near)
    assert set(part) == {"sh"}
    same(part, full, ("sh",))
    same(rt.probes_gather(pts[:65], ids[:65], spp=3, first_sample=2, near_distance=near, want=("near", "hits")), full, ("near", "hits"))
    assert (rt.probes_gather(pts[:65], ids[:65], spp=3, want=("n",))["n"] == 3).all()


# ---- 2. chunks, stripes, accumulate ------------------------------------------------------------------------------------------------------------------------
def test_chunks_stripes_and_into(pkg, ga, pr, cams, scenes, handles, sem3):
    """An 8 x 8 handle with samples_per_pass = 1 has passes of 64 rays.  65 points x 3 spp on it: chunks of 64 points and of 1, one sample each.  20 points x 8
    spp: chunks of 3, 3 and 2 samples, in ascending order.  Every output equals the same call on a default handle (one chunk), and a striped handle serves the
    call as an unstriped one does."""
    pts, ids, _, _ = probe_points(pkg, cams, scenes, "4boxes")
    rt = handles("4boxes", flags=sem3.gpu)
    small = make(pkg, scenes("4boxes"), 8, 8, flags=sem3.gpu, samples_per_pass=1)
    striped = make(pkg, scenes("4boxes"), flags=sem3.gpu, stripe_rows=2, stripe_rank=1, stripe_world=3)
    for npts, spp in ((65, 3), (20, 8), (64, 1), (130, 2), (7, 8)):
        p, i = np.ascontiguousarray(pts[:npts]), np.ascontiguousarray(ids[:npts])
        want = rt.probes_gather(p, i, spp=spp, first_sample=1, near_distance=3.0, want=ALL)
        same(want, statement(rt, ga, pr, p, i, 1, spp, 3.0))
        for other in (small, striped):
            same(other.probes_gather(p, i, spp=spp, first_sample=1, near_distance=3.0, want=ALL), want)
            assert other.last_counts().primary == npts * spp
    # into= of 3 + 5 samples equals 8, on the chunked handle and on the default one
    one = rt.probes_gather(pts[:65], ids[:65], spp=8, near_distance=3.0, want=ALL)
    for h in (small, rt):
        a = h.probes_gather(pts[:65], ids[:65], spp=3, near_distance=3.0, want=ALL)
        first = {k: v.copy() for k, v in a.items()}
        b = h.probes_gather(pts[:65], ids[:65], spp=5, first_sample=3, near_distance=3.0, want=ALL, into=a)
        same(b, one)
        assert all(b[k] is a[k] for k in ALL) and (first["n"] == 3).all()
        # without `into` the outputs start from 0 whatever they held
        same(h.probes_gather(pts[:65], ids[:65], spp=3, near_distance=3.0, want=ALL), first)
    with pytest.raises(ValueError, match="into"):
        rt.probes_gather(pts[:65], ids[:65], spp=1, want=("n", "sh"), into=dict(n=one["n"]))
    small.close(); striped.close()


# ---- 3. the lookup ---------------------------------------------------------------------------------------------------------------------------------------------
def test_probes_lookup_equals_the_statement(pkg, pr, scenes, handles):
    rt = handles("4boxes")
    counts_before = rt.last_counts().as_dict()
    used = unused = 0
    for name, g, res, usable, pts, dirs in pc.cases():
        for mode in ("radiance", "irradiance"):
            want, wok = pr.lookup(g, res, pts, dirs, mode, usable)
            got, gok = rt.probes_lookup(g, res, pts, dirs, mode, usable, want_ok=True)
            assert got.dtype == F and gok.dtype == np.uint8 and got.shape == want.shape
            assert np.array_equal(gok, wok), (name, mode)
            assert np.array_equal(bits(got), bits(want)), (name, mode)
            assert np.array_equal(bits(rt.probes_lookup(g, res, pts, dirs, mode, usable)), bits(want))       # without ok
            used += int(wok.sum()); unused += int((wok == 0).sum())
            if name.startswith("infinity"):
                assert np.isfinite(got).all() and gok.all()
    assert used > 1000 and unused > 100
    # the wave and block edges of one lane per query; the NaN and infinite coordinates are among the queries
    g = pc.grid((5, 5, 5)); res = pc.values((5, 5, 5))
    pts, dirs = pc.queries(g, 257)
    assert np.isnan(pts).any() and np.isinf(pts).any()
    for m in (1, 63, 64, 65, 257):
        p, d = np.ascontiguousarray(pts[:m]), np.ascontiguousarray(dirs[:m])
        for mode in ("radiance", "irradiance"):
            want, wok = pr.lookup(g, res, p, d, mode)
            got, gok = rt.probes_lookup(g, res, p, d, mode, want_ok=True)
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(gok, wok), (m, mode)
    assert rt.last_counts().as_dict() == counts_before                               # the lookup traces nothing and reports nothing


def test_lookup_in_a_grid_that_probes_gather_filled(pkg, pr, cams, scenes, handles):
    _, _, on, nrm = probe_points(pkg, cams, scenes, "4boxes")
    rt = handles("4boxes")
    verts = scenes("4boxes")["tri_verts"].reshape(-1, 3)
    g = pr.grid_over(verts.min(axis=0), verts.max(axis=0), (4, 3, 5))
    gp = pr.grid_points(g)
    res = rt.probes_gather(gp, spp=8, near_distance=0.2, want=ALL)
    assert (res["n"] == 8).all() and res["sh"].any()
    usable = pr.usable(res, 0.25)
    for mask in (None, usable):
        for mode in ("irradiance", "radiance"):
            want, wok = pr.lookup(g, res, on, nrm, mode, mask)
            got, gok = rt.probes_lookup(g, res, on, nrm, mode, mask, want_ok=True)
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(gok, wok)
            assert wok.any() and want[wok == 1].any()


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
    host = rt.probes_gather(p, i, spp=3, near_distance=3.0, want=ALL)
    dev = torch.device("cuda", 0)
    tp, ti = torch.from_numpy(p.copy()).to(dev), torch.from_numpy(i.copy().view(np.int32)).to(dev)
    got = rt.probes_gather(tp, ti, spp=3, near_distance=3.0, want=ALL)
    hbm = rt.hbm_allocated_bytes()
    got = rt.probes_gather(tp, ti, spp=3, near_distance=3.0, want=ALL)
    assert rt.hbm_allocated_bytes() == hbm
    for k in ALL:
        assert isinstance(got[k], torch.Tensor) and got[k].device == dev
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), host[k].view(np.uint32)), k
    # in place on the device: accumulate into tensors
    a = rt.probes_gather(tp, ti, spp=1, near_distance=3.0, want=ALL)
    b = rt.probes_gather(tp, ti, spp=2, first_sample=1, near_distance=3.0, want=ALL, into=a)
    assert all(b[k] is a[k] for k in ALL)
    for k in ALL:
        assert np.array_equal(b[k].cpu().numpy().view(np.uint32), host[k].view(np.uint32)), k
    rt.probes_gather(p, i, spp=3, want=ALL)
    assert rt.hbm_allocated_bytes() == hbm
    # the lookup on tensors, in place
    counts_before = rt.last_counts().as_dict()
    g = pc.grid((5, 5, 5)); res = pc.values((5, 5, 5))
    qp, qd = pc.queries(g, 257)
    mask = (np.arange(125) % 3 != 0).astype(np.uint8)
    want, wok = rt.probes_lookup(g, res, qp, qd, "irradiance", mask, want_ok=True)
    assert np.array_equal(bits(want), bits(pr.lookup(g, res, qp, qd, "irradiance", mask)[0]))
    tres = dict(n=torch.from_numpy(res["n"].view(np.int32).copy()).to(dev), sh=torch.from_numpy(res["sh"].copy()).to(dev))
    tq, td, tm = torch.from_numpy(qp.copy()).to(dev), torch.from_numpy(qd.copy()).to(dev), torch.from_numpy(mask.copy()).to(dev)
    trgb, tok = rt.probes_lookup(g, tres, tq, td, "irradiance", tm, want_ok=True)
    assert isinstance(trgb, torch.Tensor) and trgb.device == dev and tok.dtype == torch.uint8
    assert np.array_equal(bits(trgb.cpu().numpy()), bits(want)) and np.array_equal(tok.cpu().numpy(), wok)
    assert rt.hbm_allocated_bytes() == hbm
    assert rt.last_counts().as_dict() == counts_before
    with pytest.raises(ValueError, match="GPU"):
        rt.probes_gather(tp.cpu(), None)
    with pytest.raises(ValueError, match="must live where points live"):
        rt.probes_lookup(g, res, tq, td)
    with pytest.raises(TypeError, match="dtype"):
        rt.probes_gather(tp.double(), None)
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


def raw_gather(pkg, rt, points, ids, npoints, want=ALL, where=0, null_cfg=False, **cfg_kw):
    """mi355rt_probes_gather through ctypes into sentinel-filled outputs; returns (code, {name: uint32 array})"""
    cfg = pkg.ProbeConfig()
    pkg.lib().mi355rt_probes_default_config(C.byref(cfg))
    cfg.spp = 2
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    o, arrs = pkg.ProbeOutputs(), {}
    for w in want:
        arrs[w] = np.full((npoints + GUARD) * (27 if w == "sh" else 1), SENTINEL, np.uint32)
        setattr(o, w, arrs[w].ctypes.data)
    ptr = lambda a: None if a is None else a.ctypes.data
    code = pkg.lib().mi355rt_probes_gather(rt._h, ptr(points), ptr(ids), npoints, None if null_cfg else C.byref(cfg), where, C.byref(o))
    return code, arrs


def raw_lookup(pkg, rt, grid, res, points, dirs, npoints, mode=0, where=0, usable=None, null=()):
    """mi355rt_probes_lookup through ctypes into sentinel-filled outputs; null: names of arguments passed as NULL; returns (code, rgb words, ok bytes)"""
    g = None if grid is None else (grid if isinstance(grid, pkg.ProbeGrid) else pkg.ProbeGrid.from_dict(grid))
    rgb = np.full((npoints + GUARD) * 3, SENTINEL, np.uint32); ok = np.full(npoints + GUARD, 0xA5, np.uint8)
    ptr = lambda name, a: None if (a is None or name in null) else a.ctypes.data
    code = pkg.lib().mi355rt_probes_lookup(rt._h, None if g is None else C.byref(g), ptr("n", res["n"]), ptr("sh", res["sh"]), ptr("usable", usable), ptr("points3", points),
                                           ptr("dirs3", dirs), npoints, mode, where, ptr("rgb3", rgb), ptr("ok", ok))
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
        assert "mi355rt_probes_gather" in err() and all(nm in err() for nm in names), err()
        assert all(np.all(v == SENTINEL) for v in arrs.values())
        film_untouched()

    refused(raw_gather(pkg, rt, None, i, 10), "points3")
    refused(raw_gather(pkg, rt, p, i, 10, want=()), "out")
    cfg = pkg.ProbeConfig(); lib.mi355rt_probes_default_config(C.byref(cfg))
    assert lib.mi355rt_probes_gather(rt._h, p.ctypes.data, None, 10, C.byref(cfg), 0, None) == E_INVALID and "out" in err()
    refused(raw_gather(pkg, rt, p, i, 10, null_cfg=True), "cfg")
    refused(raw_gather(pkg, rt, p, i, 10, spp=0), "spp")
    refused(raw_gather(pkg, rt, p, i, 10, want=("n",), spp=0), "spp")
    refused(raw_gather(pkg, rt, p, i, 10, where=2), "where")
    refused(raw_gather(pkg, rt, p, i, 10, near_distance=float("nan")), "near_distance")
    refused(raw_gather(pkg, rt, p, i, 10, spp=2**32 // 10 + 1), "npoints * spp")
    refused(raw_gather(pkg, rt, p, i, 10, spp=3, first_sample=0xFFFFFFFE), "first_sample")
    # what is allowed right at those edges
    code, arrs = raw_gather(pkg, rt, p, i, 10, want=("n",), spp=2, first_sample=0xFFFFFFFD)
    assert code == 0 and (arrs["n"][:10] == 2).all() and (arrs["n"][10:] == SENTINEL).all()
    code, arrs = raw_gather(pkg, rt, p, None, 10, near_distance=float("-inf"), spp=1)
    assert code == 0 and not arrs["near"][:10].any() and all((v[10 * (27 if k == "sh" else 1):] == SENTINEL).all() for k, v in arrs.items())
    assert not (arrs["sh"][:270] == SENTINEL).any()
    # npoints == 0 succeeds and writes nothing, with or without pointers
    code, arrs = raw_gather(pkg, rt, p, i, 0)
    assert code == 0 and all(np.all(v == SENTINEL) for v in arrs.values())
    code, arrs = raw_gather(pkg, rt, None, None, 0, want=("n",))
    assert code == 0 and np.all(arrs["n"] == SENTINEL)
    assert rt.probes_gather(np.zeros((0, 3), F))["sh"].shape == (0, 9, 3)

    # ---- the lookup
    g = pc.grid((4, 3, 2)); res = pc.values((4, 3, 2))
    qp, qd = pc.queries(g, 10)

    def lrefused(result, *names):
        code, rgb, ok = result
        assert code == E_INVALID
        assert "mi355rt_probes_lookup" in err() and all(nm in err() for nm in names), err()
        assert np.all(rgb == SENTINEL) and np.all(ok == 0xA5)
        film_untouched()

    def grid_with(field, value):
        b = pkg.ProbeGrid.from_dict(g)
        for a in range(3):
            getattr(b, field)[a] = value[a]
        return b

    lrefused(raw_lookup(pkg, rt, None, res, qp, qd, 10), "grid")
    lrefused(raw_lookup(pkg, rt, grid_with("counts", (4, 0, 2)), res, qp, qd, 10), "counts")
    lrefused(raw_lookup(pkg, rt, grid_with("counts", (2048, 2048, 512)), res, qp, qd, 10), "counts", "2^31")
    for bad in ((0.7, 0.0, 0.9), (0.7, -1.0, 0.9), (float("inf"), 1.3, 0.9), (0.7, 1.3, float("nan"))):
        lrefused(raw_lookup(pkg, rt, grid_with("spacing", bad), res, qp, qd, 10), "spacing")
    for bad in ((float("nan"), 0.0, 0.0), (0.0, float("-inf"), 0.0)):
        lrefused(raw_lookup(pkg, rt, grid_with("origin", bad), res, qp, qd, 10), "origin")
    lrefused(raw_lookup(pkg, rt, g, res, qp, qd, 10, null=("n",)), "n is NULL")
    lrefused(raw_lookup(pkg, rt, g, res, qp, qd, 10, null=("sh",)), "sh")
    code, rgb, ok = raw_lookup(pkg, rt, g, res, qp, qd, 10, null=("rgb3",))
    assert code == E_INVALID and "rgb3" in err() and np.all(ok == 0xA5)
    lrefused(raw_lookup(pkg, rt, g, res, qp, qd, 10, null=("points3",)), "points3")
    lrefused(raw_lookup(pkg, rt, g, res, qp, qd, 10, null=("dirs3",)), "dirs3")
    lrefused(raw_lookup(pkg, rt, g, res, qp, qd, 10, mode=2), "mode")
    lrefused(raw_lookup(pkg, rt, g, res, qp, qd, 10, where=2), "where")
    # what is allowed: ok and usable NULL, npoints == 0 (nothing written), and the guard behind the outputs stays
    code, rgb, ok = raw_lookup(pkg, rt, g, res, qp, qd, 10, null=("ok",))
    assert code == 0 and np.all(ok == 0xA5) and np.all(rgb[30:] == SENTINEL)
    assert np.array_equal(rgb[:30], bits(pr.lookup(g, res, qp, qd, "radiance")[0]).reshape(-1))
    code, rgb, ok = raw_lookup(pkg, rt, g, res, qp, qd, 10, mode=1)
    want, wok = pr.lookup(g, res, qp, qd, "irradiance")
    assert code == 0 and np.array_equal(ok[:10], wok) and np.all(ok[10:] == 0xA5) and np.array_equal(rgb[:30], bits(want).reshape(-1)) and np.all(rgb[30:] == SENTINEL)
    code, rgb, ok = raw_lookup(pkg, rt, g, res, None, None, 0)
    assert code == 0 and np.all(rgb == SENTINEL) and np.all(ok == 0xA5)
    # the Python face
    with pytest.raises(ValueError, match="want"):
        rt.probes_gather(p, want=("sum",))
    with pytest.raises(ValueError, match="mode"):
        rt.probes_lookup(g, res, qp, qd, mode="sine")
    with pytest.raises(ValueError, match="shape"):
        rt.probes_lookup(g, dict(n=res["n"], sh=res["sh"][:5]), qp, qd)
    with pytest.raises(RuntimeError, match="spp"):
        rt.probes_gather(p, spp=0)
    rt.get_denoised_pixels()
    rt.close()
    # a device group (here: two members sharing the one GPU) refuses both
    grp = make(pkg, scenes("4boxes"), device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    code, arrs = raw_gather(pkg, grp, p, i, 10)
    assert code == E_INVALID and "device group" in err(grp) and "mi355rt_probes_gather" in err(grp) and all(np.all(v == SENTINEL) for v in arrs.values())
    code, rgb, ok = raw_lookup(pkg, grp, g, res, qp, qd, 10)
    assert code == E_INVALID and "device group" in err(grp) and "mi355rt_probes_lookup" in err(grp) and np.all(rgb == SENTINEL) and np.all(ok == 0xA5)
    grp.close()
