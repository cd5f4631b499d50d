"""Probe placement on the device (include/mi355rt.h "PROBE PLACEMENT"): the survey of a probe gather's closest hits, the placement kernel
and the offset-aware lookup.

The yardstick is the statement (raytracer_rs_amd.probes, numpy f32) over entries that are pinned elsewhere: probes_survey must equal
gather.rays(normals=None) -> intersect_rays -> probes.survey on every word, probes_place must equal probes.place / probes.classify and probes_lookup_placed
probes.lookup_placed on every bit, on the hand-made cases of tests/probe_place_cases.py.  On the four hand-made scenes the outcomes are the ones
tests/test_probes_place_abi.py has established for the statement through the CPU oracle, and the device must reach them through the same statement."""
import ctypes as C
import importlib

import numpy as np
import pytest

import probe_cases as pc
import probe_place_cases as pp
import probe_vis_cases as pv

pytestmark = pytest.mark.gpu

W = H = pp.W
SEED = pp.SEED
MISS = pp.MISS
E_INVALID = -1
KEYS = ("n", "back", "front", "near_back", "near_front", "far")
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
def ft(pkg):
    return importlib.import_module("raytracer_rs_amd.features")


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
            made[key] = make(pkg, scenes(name) if isinstance(name, str) else name(), **kw)
        return made[key]
    yield get
    for rt in made.values():
        rt.close()


_NORMALS = {}


def normals_of(ft, scenes, name):
    if name not in _NORMALS:
        _NORMALS[name] = ft.tri_normals(scenes(name))
    return _NORMALS[name]


def closest(rt, ga, pts, ids, first, spp):
    """gather.rays(normals=None) -> intersect_rays: (directions, t, prim)"""
    rays, keys, valid, w = ga.rays(rt.sample_table(), SEED, pts, None, ids, first, spp)
    assert valid.all()
    tuv, prim = rt.intersect_rays(rays)
    return rays[:, 3:], tuv[:, 0], prim


def statement(rt, ga, pr, N, pts, ids, first, spp, D, flip=False, prev=None):
    d, t, prim = closest(rt, ga, pts, ids, first, spp)
    return pr.survey(t, prim, d, N, len(pts), D, flip, prev)


def same(got, want, keys=KEYS):
    for k in keys:
        assert tuple(got[k].shape) == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


# points x spp; the block is 256 lanes, one per point: 1, a wave but one, a wave, a wave and one, a block and one
SHAPES = [(1, 1), (63, 2), (64, 3), (65, 4), (257, 5), (1, 6), (63, 7), (64, 8), (65, 1), (257, 2), (29, 64)]
FIRSTS = (0, 5, 0xFFFFFFFF - 10, 0xFFFFFFFD - 8)


# ---- 1. the statement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4boxes", "ico3_tex"])
def test_probes_survey_equals_the_statement(pkg, ga, pr, ft, cams, scenes, handles, sem3, name):
    pts, ids = pp.probe_points(pkg, cams, scenes, name)
    N = normals_of(ft, scenes, name)
    rt = handles(name, flags=sem3.gpu)
    d, t, prim = closest(rt, ga, pts[:257], ids[:257], 0, 8)
    hit = prim != MISS
    D = float(F(0.8 * np.median(t[hit])))                    # below the median t: many samples tie at exactly D in far
    assert (hit & (t < F(D))).sum() > 100 and (hit & ~(t < F(D))).sum() > 100 and (~hit).sum() > 100
    for k, (npts, spp) in enumerate(SHAPES):
        first, flip = FIRSTS[k % 4] if spp <= 8 else 0xFFFFFFFD - 64, bool(k % 2)
        p, i = np.ascontiguousarray(pts[:npts]), np.ascontiguousarray(ids[:npts])
        want = statement(rt, ga, pr, N, p, i, first, spp, D, flip)
        got = rt.probes_survey(p, i, spp=spp, first_sample=first, max_distance=D, flip=flip)
        same(got, want)
        assert set(got) == set(KEYS) | {"max_distance"} and got["max_distance"] == D and (got["n"] == spp).all()
        c = rt.last_counts()
        assert (c.primary, c.bounce, c.shadow) == (npts * spp, 0, 0)                                           # closest hits only: no bounce tree
    # sample numbers up to 2^32 - 3: the last sample of the 64-spp case is number 2^32 - 4, of this one 2^32 - 3
    same(rt.probes_survey(pts[:65], ids[:65], spp=2, first_sample=0xFFFFFFFC, max_distance=D), statement(rt, ga, pr, N, pts[:65], ids[:65], 0xFFFFFFFC, 2, D))
    # ties at exactly D: of the samples of a point whose recorded distance is D, the first in order holds far
    big = rt.probes_survey(pts[:257], ids[:257], spp=8, max_distance=D)
    same(big, statement(rt, ga, pr, N, pts[:257], ids[:257], 0, 8, D))
    dd, tt, pm = d.reshape(8, 257, 3), t.reshape(8, 257), prim.reshape(8, 257)
    nrm = N[np.where(pm != MISS, pm, 0)]
    is_hit = (pm != MISS) & (tt > 0) & np.isfinite(tt)
    back = is_hit & (((dd[..., 0] * nrm[..., 0] + dd[..., 1] * nrm[..., 1]) + dd[..., 2] * nrm[..., 2]) > 0)
    at_D = ~back & ~(is_hit & (tt < F(D)))                                                                      # misses and front hits at or beyond D
    tied = at_D.sum(axis=0) >= 2
    assert tied.sum() > 100                                                                                     # ties occur
    first_at = at_D.argmax(axis=0)
    for i in np.nonzero(tied)[0]:
        assert big["far"][i, 0] == F(D) and np.array_equal(bits(big["far"][i, 1:]), bits(dd[first_at[i], i])), i
    assert (big["front"] > 0).sum() > 200
    assert (big["back"] + big["front"] <= big["n"]).all() and np.isinf(big["near_back"][big["back"] == 0, 0]).all()
    # the same sample range accumulated twice: the counts double, every record keeps the first call's direction (and the bits of the first call)
    once = rt.probes_survey(pts[:257], ids[:257], spp=8, max_distance=D)
    twice = rt.probes_survey(pts[:257], ids[:257], spp=8, max_distance=D, into={k: (v.copy() if k in KEYS else v) for k, v in once.items()})
    for k in ("n", "back", "front"):
        assert np.array_equal(twice[k], 2 * once[k]), k
    same(twice, once, ("near_back", "near_front", "far"))
    # ids=None is i
    same(rt.probes_survey(pts[:29], None, spp=3, first_sample=2, max_distance=D), statement(rt, ga, pr, N, pts[:29], None, 2, 3, D))


# ---- 2. chunks, stripes, accumulate ------------------------------------------------------------------------------------------------------------------------
def test_chunks_stripes_and_into(pkg, ga, pr, ft, cams, scenes, handles, sem3):
    """An 8 x 8 handle with samples_per_pass = 1 has chunks of 64 rays.  65 points x 3 spp on it: chunks of 64 points and of 1, one sample each, so the chunks
    cut both points and samples.  20 points x 8 spp: chunks of 3, 3 and 2 samples, in ascending order.  Every word equals the same call on a default handle
    (one chunk), and a striped handle serves the call as an unstriped one does."""
    pts, ids = pp.probe_points(pkg, cams, scenes, "4boxes")
    N = normals_of(ft, scenes, "4boxes")
    rt = handles("4boxes", flags=sem3.gpu)
    small = make(pkg, scenes("4boxes"), 8, 8, flags=sem3.gpu, samples_per_pass=1)
    striped = make(pkg, scenes("4boxes"), flags=sem3.gpu, stripe_rows=2, stripe_rank=1, stripe_world=3)
    for k, (npts, spp) in enumerate(((65, 3), (20, 8), (64, 1), (130, 2), (7, 8))):
        p, i = np.ascontiguousarray(pts[:npts]), np.ascontiguousarray(ids[:npts])
        want = rt.probes_survey(p, i, spp=spp, first_sample=1, max_distance=2.0, flip=bool(k % 2))
        same(want, statement(rt, ga, pr, N, p, i, 1, spp, 2.0, bool(k % 2)))
        for other in (small, striped):
            same(other.probes_survey(p, i, spp=spp, first_sample=1, max_distance=2.0, flip=bool(k % 2)), want)
            assert other.last_counts().primary == npts * spp
    # into= of 3 + 5 samples equals 8, on the chunked handle and on the default one
    one = rt.probes_survey(pts[:65], ids[:65], spp=8, max_distance=2.0)
    for h in (small, rt):
        a = h.probes_survey(pts[:65], ids[:65], spp=3, max_distance=2.0)
        first = {k: (v.copy() if k in KEYS else v) for k, v in a.items()}
        b = h.probes_survey(pts[:65], ids[:65], spp=5, first_sample=3, max_distance=2.0, into=a)
        same(b, one)
        assert all(b[k] is a[k] for k in KEYS) and (first["n"] == 3).all() and b["max_distance"] == 2.0
        c = h.probes_survey(pts[:65], ids[:65], spp=5, first_sample=3, into={k: (v.copy() if k in KEYS else v) for k, v in first.items()})      # max_distance None: that of `into`
        same(c, one)
        same(h.probes_survey(pts[:65], ids[:65], spp=3, max_distance=2.0), first)                               # without `into` the state starts empty whatever it held
    with pytest.raises(ValueError, match="into"):
        rt.probes_survey(pts[:65], ids[:65], spp=1, max_distance=2.5, into=one)
    with pytest.raises(ValueError, match="into"):
        rt.probes_survey(pts[:65], ids[:65], spp=1, into={k: one[k] for k in KEYS})
    small.close(); striped.close()


# ---- 3. placement and the offset-aware lookup ----------------------------------------------------------------------------------------------------------------
SIZES = [((1, 1, 1), 1), ((7, 3, 3), 63), ((4, 4, 4), 64), ((13, 5, 1), 65), ((257, 1, 1), 257)]


def test_probes_place_equals_the_statement(pkg, pr, handles):
    rt = handles("4boxes")
    counts_before = rt.last_counts().as_dict()
    names, sv, off = pp.place_cases()
    for offsets in (off, None):
        want, verdict = pr.place(sv, offsets, pp.GRID, min_front=pp.MIN_FRONT, want_verdict=True)
        got, gv, gs = rt.probes_place(pp.GRID, sv, offsets, min_front=pp.MIN_FRONT)
        assert got.dtype == F and gv.dtype == np.uint8 and gs.dtype == np.uint8
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(gv, verdict) and np.array_equal(gs, pr.classify(sv))
    assert {0, 1, 2, 3, 4, 5, 9, 10} <= set(verdict.tolist()) | set(pr.place(sv, off, pp.GRID, min_front=pp.MIN_FRONT, want_verdict=True)[1].tolist())
    # any selection of the outputs, in the order asked; the default min_front is grid_min_front
    (s_only,) = rt.probes_place(pp.GRID, sv, off, want=("state",))
    v_first, o_second = rt.probes_place(pp.GRID, sv, off, want=("verdict", "offsets"))
    w, v = pr.place(sv, off, pp.GRID, min_front=pr.grid_min_front(pp.GRID), want_verdict=True)
    assert np.array_equal(s_only, pr.classify(sv)) and np.array_equal(v_first, v) and np.array_equal(bits(o_second), bits(w))
    seen = set()
    for k, (counts, nprobes) in enumerate(SIZES):
        g = dict(origin=np.array([0.5, -1.0, 2.0], F), spacing=np.array([0.7, 1.3, 0.9], F), counts=np.array(counts, np.uint32))
        svr, offr = pp.random_surveys(nprobes, 20 + k, g)
        bs, mo, mf = (0.25, 0.45, 0.2) if k % 2 else (0.1, 0.3, 0.35)
        want, verdict = pr.place(svr, offr, g, bs, mo, mf, want_verdict=True)
        got, gv, gs = rt.probes_place(g, svr, offr, bs, mo, mf)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(gv, verdict) and np.array_equal(gs, pr.classify(svr, bs)), counts
        seen |= set(gv.tolist())
    assert seen >= {0, 1, 2, 4, 5}
    assert rt.last_counts().as_dict() == counts_before                               # placement traces nothing and reports nothing


def test_probes_lookup_placed_equals_the_statement(pkg, pr, handles):
    rt = handles("4boxes")
    counts_before = rt.last_counts().as_dict()
    used = unused = 0
    for k, (name, g, res, depth, usable, pts, dirs, nrm) in enumerate(pv.lookup_cases()):
        full = dict(res, count=depth["count"], moments=depth["moments"], depth_res=depth["res"], max_distance=depth["max_distance"])
        nprobes = len(res["n"])
        rng = np.random.default_rng(80 + k)
        off = np.ascontiguousarray((rng.uniform(-0.45, 0.45, (nprobes, 3)) * g["spacing"].astype(np.float64)).astype(F))
        gp = pc.probe_positions(g)
        if np.isfinite(pts[0]).all():
            j = int(np.abs(gp - pts[0]).sum(axis=1).argmin())
            off[j] = pts[0] - gp[j]                                  # a probe on the first query
        plain, pok = rt.probes_lookup(g, res, pts, dirs, "irradiance", usable, want_ok=True)
        for c, (cheb, facing) in enumerate(pv.FLAGS):
            mode = ("radiance", "irradiance")[(k + c) % 2]
            normals, bias = ((nrm, 0.0), (nrm, 0.13), (None, 0.0))[(k + c) % 3]
            for offsets in (off, None, np.zeros_like(off)):
                want, wok = pr.lookup_placed(g, res, depth, pts, dirs, normals, mode, usable, cheb, facing, bias, offsets)
                got, gok = rt.probes_lookup_placed(g, full, pts, dirs, normals, mode, usable, cheb, facing, bias, offsets, want_ok=True)
                assert got.dtype == F and gok.dtype == np.uint8 and got.shape == want.shape
                assert np.array_equal(gok, wok) and np.array_equal(bits(got), bits(want)), (name, cheb, facing, bias, offsets is None)
                used += int(wok.sum()); unused += int((wok == 0).sum())
            # offsets None is probes_lookup_vis on every bit
            vis, vok = rt.probes_lookup_vis(g, full, pts, dirs, normals, mode, usable, cheb, facing, bias, want_ok=True)
            none, nok = rt.probes_lookup_placed(g, full, pts, dirs, normals, mode, usable, cheb, facing, bias, None, want_ok=True)
            assert np.array_equal(bits(none), bits(vis)) and np.array_equal(nok, vok)
        # with both flags off the offsets cannot matter: probes_lookup on every bit
        zero, zok = rt.probes_lookup_placed(g, full, pts, dirs, nrm, "irradiance", usable, False, False, 0.0, off, want_ok=True)
        assert np.array_equal(bits(zero), bits(plain)) and np.array_equal(zok, pok)
    assert used > 10000 and unused > 2000
    # the wave and block edges of one lane per query; NaN and infinite coordinates are among the queries
    g = pc.grid((5, 5, 5)); res = pc.values((5, 5, 5)); depth = pv.film(8, 125, 90)
    full = dict(res, count=depth["count"], moments=depth["moments"], depth_res=8, max_distance=3.0)
    pts, dirs = pc.queries(g, 257)
    nrm = pv.normals(257)
    off = np.ascontiguousarray((np.random.default_rng(7).uniform(-0.45, 0.45, (125, 3)) * g["spacing"].astype(np.float64)).astype(F))
    assert np.isnan(pts).any() and np.isinf(pts).any()
    for m in (1, 63, 64, 65, 257):
        p, d, n = np.ascontiguousarray(pts[:m]), np.ascontiguousarray(dirs[:m]), np.ascontiguousarray(nrm[:m])
        for mode in ("radiance", "irradiance"):
            want, wok = pr.lookup_placed(g, res, depth, p, d, n, mode, None, True, True, 0.05, off)
            got, gok = rt.probes_lookup_placed(g, full, p, d, n, mode, normal_bias=0.05, offsets=off, want_ok=True)
            assert np.array_equal(bits(got), bits(want)) and np.array_equal(gok, wok), (m, mode)
    assert rt.last_counts().as_dict() == counts_before                               # the lookup traces nothing and reports nothing


# ---- 4. device memory, and what the calls leave alone ----------------------------------------------------------------------------------------------------
def test_device_tensors_and_an_untouched_handle(pkg, ga, pr, cams, scenes, sem3):
    import torch
    pts, ids = pp.probe_points(pkg, cams, scenes, "4boxes")
    rt = make(pkg, scenes("4boxes"), flags=sem3.gpu | pkg.FLAG_DIRECT_FILM | pkg.FLAG_LIGHT_FILMS)
    rt.set_lens("thin", radius=0.05, focus=4.0)
    rt.render(2)
    s, q, n = rt.film.pixel_datas()
    before = (bits(s).copy(), bits(q).copy(), n.copy(), bits(rt.film.direct_sums()).copy(), bits(rt.light_films.get()).copy())
    row, cam, lens = rt.current_row, [a.copy() for a in rt.camera.matrices()], rt.lens.as_dict()
    p, i = np.ascontiguousarray(pts[:130]), np.ascontiguousarray(ids[:130])
    host = rt.probes_survey(p, i, spp=3, max_distance=2.0)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a.view(np.int32).copy() if a.dtype == np.uint32 else a.copy()).to(dev)
    tp, ti = t(p), t(i)
    got = rt.probes_survey(tp, ti, spp=3, max_distance=2.0)
    hbm = rt.hbm_allocated_bytes()
    got = rt.probes_survey(tp, ti, spp=3, max_distance=2.0)
    assert rt.hbm_allocated_bytes() == hbm                                            # every temporary, the chunk's hits among them, is freed and counted
    for k in KEYS:
        assert isinstance(got[k], torch.Tensor) and got[k].device == dev
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), host[k].view(np.uint32)), k
    assert got["n"].dtype == torch.int32 and tuple(got["far"].shape) == (130, 4)
    # in place on the device: continue a survey held in tensors
    a = rt.probes_survey(tp, ti, spp=1, max_distance=2.0)
    b = rt.probes_survey(tp, ti, spp=2, first_sample=1, into=a)
    assert all(b[k] is a[k] for k in KEYS)
    for k in KEYS:
        assert np.array_equal(b[k].cpu().numpy().view(np.uint32), host[k].view(np.uint32)), k
    rt.probes_survey(p, i, spp=3, max_distance=2.0)
    assert rt.hbm_allocated_bytes() == hbm
    counts_before = rt.last_counts().as_dict()
    # placement on tensors
    names, sv, off = pp.place_cases()
    want, wv, ws = rt.probes_place(pp.GRID, sv, off, min_front=pp.MIN_FRONT)
    tsv = {k: (t(v) if k in KEYS else v) for k, v in sv.items()}
    to, tv, ts = rt.probes_place(pp.GRID, tsv, t(off), min_front=pp.MIN_FRONT)
    assert all(isinstance(x, torch.Tensor) and x.device == dev for x in (to, tv, ts)) and tv.dtype == torch.uint8
    assert np.array_equal(bits(to.cpu().numpy()), bits(want)) and np.array_equal(tv.cpu().numpy(), wv) and np.array_equal(ts.cpu().numpy(), ws)
    assert np.array_equal(pr.usable_states(ts).cpu().numpy(), pr.usable_states(ws))
    # the lookup on tensors
    g = pc.grid((5, 5, 5)); res = pc.values((5, 5, 5)); depth = pv.film(16, 125, 91)
    full = dict(res, count=depth["count"], moments=depth["moments"], depth_res=16, max_distance=3.0)
    qp, qd = pc.queries(g, 257)
    qn = pv.normals(257)
    mask = (np.arange(125) % 3 != 0).astype(np.uint8)
    qo = np.ascontiguousarray((np.random.default_rng(8).uniform(-0.4, 0.4, (125, 3)) * g["spacing"].astype(np.float64)).astype(F))
    want, wok = rt.probes_lookup_placed(g, full, qp, qd, qn, "irradiance", mask, normal_bias=0.1, offsets=qo, want_ok=True)
    assert np.array_equal(bits(want), bits(pr.lookup_placed(g, res, depth, qp, qd, qn, "irradiance", mask, True, True, 0.1, qo)[0]))
    tfull = dict(n=t(res["n"]), sh=t(res["sh"]), count=t(depth["count"]), moments=t(depth["moments"]), depth_res=16, max_distance=3.0)
    trgb, tok = rt.probes_lookup_placed(g, tfull, t(qp), t(qd), t(qn), "irradiance", t(mask), normal_bias=0.1, offsets=t(qo), want_ok=True)
    assert isinstance(trgb, torch.Tensor) and trgb.device == dev and tok.dtype == torch.uint8
    assert np.array_equal(bits(trgb.cpu().numpy()), bits(want)) and np.array_equal(tok.cpu().numpy(), wok)
    assert rt.hbm_allocated_bytes() == hbm
    assert rt.last_counts().as_dict() == counts_before
    with pytest.raises(ValueError, match="GPU"):
        rt.probes_survey(tp.cpu(), None, max_distance=2.0)
    with pytest.raises(ValueError, match="must live where points live"):
        rt.probes_lookup_placed(g, tfull, t(qp), t(qd), t(qn), offsets=qo)
    with pytest.raises(ValueError, match="must live where"):
        rt.probes_place(pp.GRID, tsv, off)
    with pytest.raises(ValueError, match="must live where points live"):
        rt.probes_survey(tp, ti, spp=1, into=host)
    with pytest.raises(TypeError, match="dtype"):
        rt.probes_survey(tp.double(), None, max_distance=2.0)
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


def raw_survey(pkg, rt, points, ids, npoints, where=0, null=(), **cfg_kw):
    """mi355rt_probes_survey through ctypes into sentinel-filled outputs; null: names passed as NULL; returns (code, {name: uint32 array})"""
    cfg = pkg.ProbeSurveyConfig()
    pkg.lib().mi355rt_probes_survey_default_config(C.byref(cfg))
    cfg.spp, cfg.max_distance = 2, 2.0
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    o, arrs = pkg.ProbeSurvey(), {}
    for w in KEYS:
        arrs[w] = np.full((npoints + GUARD) * (1 if w in ("n", "back", "front") else 4), SENTINEL, np.uint32)
        setattr(o, w, None if w in null else arrs[w].ctypes.data)
    ptr = lambda a: None if a is None else a.ctypes.data
    code = pkg.lib().mi355rt_probes_survey(rt._h, ptr(points), ptr(ids), npoints, None if "cfg" in null else C.byref(cfg), where, None if "out" in null else C.byref(o))
    return code, arrs


def test_refusals_name_the_argument_and_write_nothing(pkg, pr, cams, scenes):
    pts, ids = pp.probe_points(pkg, cams, scenes, "4boxes")
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
        assert "mi355rt_probes_survey" in err() and all(nm in err() for nm in names), err()
        assert all(np.all(v == SENTINEL) for v in arrs.values())
        film_untouched()

    refused(raw_survey(pkg, rt, None, i, 10), "points3")
    refused(raw_survey(pkg, rt, p, i, 10, null=("cfg",)), "cfg")
    refused(raw_survey(pkg, rt, p, i, 10, null=("out",)), "out")
    for k in KEYS:
        refused(raw_survey(pkg, rt, p, i, 10, null=(k,)), "out." + k)
    for bad in (0.0, -2.0, float("nan"), float("inf"), 1.0001e12):
        refused(raw_survey(pkg, rt, p, i, 10, max_distance=bad), "max_distance")
    refused(raw_survey(pkg, rt, p, i, 10, flags=2), "flags")
    refused(raw_survey(pkg, rt, p, i, 10, spp=0), "spp")
    refused(raw_survey(pkg, rt, p, i, 10, where=2), "where")
    refused(raw_survey(pkg, rt, p, i, 10, spp=2**32 // 10 + 1), "npoints * spp")
    refused(raw_survey(pkg, rt, p, i, 10, spp=3, first_sample=0xFFFFFFFE), "first_sample")
    # what is allowed right at those edges: max_distance 1e12, the last sample numbers, ids NULL; the guard behind every output stays
    code, arrs = raw_survey(pkg, rt, p, None, 10, max_distance=1e12, spp=2, first_sample=0xFFFFFFFD, flags=1)
    assert code == 0 and (arrs["n"][:10] == 2).all()
    assert all((v[10 * (1 if k in ("n", "back", "front") else 4):] == SENTINEL).all() and not (v[:10 * (1 if k in ("n", "back", "front") else 4)] == SENTINEL).any() for k, v in arrs.items())
    code, arrs = raw_survey(pkg, rt, p, i, 0)
    assert code == 0 and all(np.all(v == SENTINEL) for v in arrs.values())                                      # npoints == 0 succeeds and writes nothing
    assert rt.probes_survey(np.zeros((0, 3), F), max_distance=1.0)["far"].shape == (0, 4)

    # ---- placement
    names, sv, off = pp.place_cases()
    g = pkg.ProbeGrid.from_dict(pp.GRID)

    def raw_place(grid=g, null=(), cfg=(0.25, 0.45, 0.2, 3.0), offsets=off, where=0, outs=("new", "verdict", "state")):
        s_ = pkg.ProbeSurvey()
        for k in KEYS:
            setattr(s_, k, None if k in null else sv[k].ctypes.data)
        new = np.full((48 + GUARD) * 3, SENTINEL, np.uint32); verdict = np.full(48 + GUARD, 0xA5, np.uint8); state = np.full(48 + GUARD, 0xA5, np.uint8)
        code = lib.mi355rt_probes_place(rt._h, None if grid is None else C.byref(grid), None if "survey" in null else C.byref(s_), None if cfg is None else C.byref(pkg.ProbePlaceConfig(*cfg)),
                                        None if offsets is None else offsets.ctypes.data, where, new.ctypes.data if "new" in outs else None,
                                        verdict.ctypes.data if "verdict" in outs else None, state.ctypes.data if "state" in outs else None)
        return code, new, verdict, state

    def prefused(result, *words):
        code, new, verdict, state = result
        assert code == E_INVALID and "mi355rt_probes_place" in err() and all(w in err() for w in words), err()
        assert np.all(new == SENTINEL) and np.all(verdict == 0xA5) and np.all(state == 0xA5)
        film_untouched()

    bad = pkg.ProbeGrid.from_dict(pp.GRID); bad.counts[1] = 0
    prefused(raw_place(grid=None), "grid")
    prefused(raw_place(grid=bad), "counts")
    prefused(raw_place(null=("survey",)), "survey")
    for k in KEYS:
        prefused(raw_place(null=(k,)), "survey." + k)
    prefused(raw_place(cfg=None), "cfg")
    prefused(raw_place(cfg=(1.5, 0.45, 0.2, 3.0)), "back_share")
    prefused(raw_place(cfg=(0.25, float("nan"), 0.2, 3.0)), "max_offset")
    prefused(raw_place(cfg=(0.25, 0.45, 0.0, 3.0)), "min_front")
    prefused(raw_place(cfg=(0.25, 0.45, 0.2, 0.0)), "max_distance")
    prefused(raw_place(outs=()), "all NULL")
    prefused(raw_place(where=2), "where")
    nan_off = off.copy(); nan_off[5, 1] = np.nan
    prefused(raw_place(offsets=nan_off), "offsets")
    code, new, verdict, state = raw_place(cfg=(0.25, 0.45, 0.2, 0.0), outs=("new",))                             # the move alone needs no max_distance
    assert code == 0 and np.array_equal(new[:144], bits(pr.place(sv, off, pp.GRID, min_front=0.2)).reshape(-1)) and np.all(new[144:] == SENTINEL) and np.all(state == 0xA5)
    code, new, verdict, state = raw_place(cfg=(0.25, 0.45, 0.0, 3.0), outs=("state",), offsets=None)              # the state alone needs no min_front
    assert code == 0 and np.array_equal(state[:48], pr.classify(sv)) and np.all(state[48:] == 0xA5) and np.all(new == SENTINEL)

    # ---- the lookup: what mi355rt_probes_lookup_vis refuses, and the offsets
    gl = pc.grid((4, 3, 2)); res = pc.values((4, 3, 2)); depth = pv.film(3, 24, 92)
    qp, qd = pc.queries(gl, 10)
    qn = pv.normals(10)
    qo = np.zeros((24, 3), F)

    def raw_lookup(null=(), flags=3, bias=0.0, mode=0, where=0, offsets=qo, npoints=10, d_res=3):
        rgb = np.full((10 + GUARD) * 3, SENTINEL, np.uint32); ok = np.full(10 + GUARD, 0xA5, np.uint8)
        ptr = lambda name, a: None if (a is None or name in null) else a.ctypes.data
        d = pkg.ProbeDepth(d_res, 3.0, ptr("count", depth["count"]), ptr("moments", depth["moments"]))
        code = lib.mi355rt_probes_lookup_placed(rt._h, None if "grid" in null else C.byref(pkg.ProbeGrid.from_dict(gl)), ptr("n", res["n"]), ptr("sh", res["sh"]), None,
                                                None if "depth" in null else C.byref(d), None if "vc" in null else C.byref(pkg.ProbeVisConfig(flags, bias)), ptr("offsets", offsets),
                                                ptr("points3", qp), ptr("dirs3", qd), ptr("normals3", qn), npoints, mode, where, ptr("rgb3", rgb), ptr("ok", ok))
        return code, rgb, ok

    def lrefused(result, *words):
        code, rgb, ok = result
        assert code == E_INVALID and "mi355rt_probes_lookup_placed" in err() and all(w in err() for w in words), err()
        assert np.all(rgb == SENTINEL) and np.all(ok == 0xA5)
        film_untouched()

    for nm, word in (("grid", "grid"), ("n", "n is NULL"), ("sh", "sh"), ("depth", "depth"), ("count", "count"), ("moments", "moments"), ("vc", "vc"), ("points3", "points3"),
                     ("dirs3", "dirs3"), ("normals3", "normals3")):
        lrefused(raw_lookup(null=(nm,)), word)
    lrefused(raw_lookup(flags=4), "flags")
    lrefused(raw_lookup(bias=float("nan")), "normal_bias")
    lrefused(raw_lookup(mode=2), "mode")
    lrefused(raw_lookup(where=2), "where")
    lrefused(raw_lookup(d_res=17), "res")
    inf_off = qo.copy(); inf_off[23, 2] = np.inf
    lrefused(raw_lookup(offsets=inf_off), "offsets")
    code, rgb, ok = raw_lookup(null=("rgb3",))
    assert code == E_INVALID and "rgb3" in err() and np.all(ok == 0xA5)
    code, rgb, ok = raw_lookup(null=("ok", "offsets"), mode=1, bias=0.25)
    want, wok = pr.lookup_vis(gl, res, depth, qp, qd, qn, "irradiance", None, True, True, 0.25)
    assert code == 0 and np.all(ok == 0xA5) and np.array_equal(rgb[:30], bits(want).reshape(-1)) and np.all(rgb[30:] == SENTINEL)
    code, rgb, ok = raw_lookup(npoints=0)
    assert code == 0 and np.all(rgb == SENTINEL) and np.all(ok == 0xA5)
    # the Python face
    with pytest.raises(ValueError, match="max_distance"):
        rt.probes_survey(p)
    with pytest.raises(ValueError, match="max_distance"):
        rt.probes_survey(p, max_distance=float("inf"))
    with pytest.raises(RuntimeError, match="spp"):
        rt.probes_survey(p, spp=0, max_distance=1.0)
    with pytest.raises(ValueError, match="want"):
        rt.probes_place(pp.GRID, sv, off, want=("moved",))
    with pytest.raises(ValueError, match="near_front"):
        rt.probes_place(pp.GRID, {k: v for k, v in sv.items() if k != "near_front"}, off)
    with pytest.raises(ValueError, match="shape"):
        rt.probes_place(pp.GRID, sv, off[:5])
    with pytest.raises(RuntimeError, match="offsets"):
        rt.probes_place(pp.GRID, sv, nan_off)
    rt.get_denoised_pixels()
    rt.close()
    # a device group (here: two members sharing the one GPU) refuses all three
    grp = make(pkg, scenes("4boxes"), device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    code, arrs = raw_survey(pkg, grp, p, i, 10)
    assert code == E_INVALID and "device group" in err(grp) and "mi355rt_probes_survey" in err(grp) and all(np.all(v == SENTINEL) for v in arrs.values())
    rt = grp
    code, new, verdict, state = raw_place()
    assert code == E_INVALID and "device group" in err(grp) and "mi355rt_probes_place" in err(grp) and np.all(new == SENTINEL) and np.all(state == 0xA5)
    code, rgb, ok = raw_lookup()
    assert code == E_INVALID and "device group" in err(grp) and "mi355rt_probes_lookup_placed" in err(grp) and np.all(rgb == SENTINEL) and np.all(ok == 0xA5)
    grp.close()


# ---- 6. behaviour on hand-made scenes ------------------------------------------------------------------------------------------------------------------------------
def on_device_and_statement(pkg, pr, ga, ft, scene, grid, rounds, spp=64, device=None, **kw):
    """probes_relocate on a handle of the scene, every survey of it re-made by the statement from the handle's own closest hits and every placement by
    probes.place: the device must match the statement on the bits.  Returns (rt, result with numpy arrays)."""
    rt = make(pkg, scene, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    res = rt.probes_relocate(grid, rounds=rounds, spp=spp, device=device, **kw)
    if device is not None:
        res = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}
        res["survey"] = {k: (v.cpu().numpy().view(np.uint32 if k in ("n", "back", "front") else F) if hasattr(v, "cpu") else v) for k, v in res["survey"].items()}
    N = ft.tri_normals(scene)
    mf = kw.get("min_front", pr.grid_min_front(grid))
    D = pr.grid_max_distance(grid)
    gp = pr.grid_points(grid)
    off = np.zeros_like(gp)
    for r in range(rounds + 1):
        sv = statement(rt, ga, pr, N, (gp + off).astype(F), None, r * spp, spp, D)
        if r < rounds:
            off, verdict = pr.place(sv, off, grid, min_front=mf, want_verdict=True)
    same(res["survey"], sv)
    assert np.array_equal(bits(res["offsets"]), bits(off)) and np.array_equal(res["verdict"], verdict) and np.array_equal(res["state"], pr.classify(sv))
    assert np.array_equal(res["usable"], pr.usable_states(res["state"])) and np.array_equal(bits(res["points"]), bits((gp + off).astype(F)))
    return rt, res


def test_a_buried_probe_within_reach_and_the_grid_around_it(pkg, pr, ga, ft):
    import torch
    c, grid = pp.CENTRE, pp.GRID3
    scene = pp.scene_a()
    rt, res = on_device_and_statement(pkg, pr, ga, ft, scene, grid, 4, min_front=0.2, device=torch.device("cuda", 0))
    gp, D = pr.grid_points(grid), pr.grid_max_distance(grid)
    before = rt.probes_survey(gp, spp=64, max_distance=D)
    assert before["back"][c] == before["n"][c] == 64 and pr.classify(before)[c] == pr.BURIED
    fresh = rt.probes_survey(res["points"], spp=64, first_sample=1000, max_distance=D)
    assert fresh["back"][c] == 0 and (np.abs(res["offsets"]) < F(0.45)).all() and res["state"][c] != pr.BURIED and np.abs(res["offsets"][c]).max() > 0.1
    # host arrays give the same result as tensors
    host = rt.probes_relocate(grid, rounds=4, spp=64, min_front=0.2)
    assert np.array_equal(bits(host["offsets"]), bits(res["offsets"])) and np.array_equal(host["state"], res["state"])
    # end to end: films gathered at the moved points, the offset-aware lookup and usable_states give a query beside the box all eight corners; the unmoved grid
    # with usable_states has seven
    q = np.array([[1.4, 1.3, 1.35]], F); nq = np.array([[0.0, 1.0, 0.0]], F)
    moved = rt.probes_gather_depth(res["points"], spp=64, res=8, max_distance=D)
    unmoved = rt.probes_gather_depth(gp, spp=64, res=8, max_distance=D)
    depth = lambda f: dict(res=8, max_distance=D, count=f["count"], moments=f["moments"])
    w, probe = pr.corner_weights(grid, moved, depth(moved), q, None, res["usable"], True, False, 0.0, res["offsets"])
    assert c in probe[0] and (w[0] > 0).sum() == 8
    use0 = pr.usable_states(pr.classify(before))
    w0, _ = pr.corner_weights(grid, unmoved, depth(unmoved), q, None, use0, True, False, 0.0, None)
    assert (w0[0] > 0).sum() == 7 and w0[0][list(probe[0]).index(c)] == 0
    rgb, ok = rt.probes_lookup_placed(grid, moved, q, nq, None, "irradiance", res["usable"], True, False, 0.0, res["offsets"], want_ok=True)
    want, wok = pr.lookup_placed(grid, moved, depth(moved), q, nq, None, "irradiance", res["usable"], True, False, 0.0, res["offsets"])
    assert ok[0] == 1 and wok[0] == 1 and np.array_equal(bits(rgb), bits(want)) and np.isfinite(rgb).all()
    rt.close()


def test_a_buried_probe_out_of_reach(pkg, pr, ga, ft):
    rt, res = on_device_and_statement(pkg, pr, ga, ft, pp.scene_b(), pp.GRID3, 4, min_front=0.2)
    c = pp.CENTRE
    assert res["verdict"][c] == pr.PLACE_THROUGH | pr.PLACE_REFUSED and not res["offsets"][c].any() and res["state"][c] == pr.BURIED and res["usable"][c] == 0
    assert res["survey"]["back"][c] == 64
    rt.close()


def test_a_probe_against_a_wall_and_without_it(pkg, pr, ga, ft):
    grid = pp.GRID_WALL
    rt, res = on_device_and_statement(pkg, pr, ga, ft, pp.scene_c(), grid, 4, min_front=0.2)
    gp, D = pr.grid_points(grid), pr.grid_max_distance(grid)
    near = np.nonzero(gp[:, 2] == F(0.02))[0]
    assert len(near) == 4 and (res["points"][near, 2] > gp[near, 2] + F(0.05)).all() and (res["state"] == pr.ACTIVE).all()
    gone = make(pkg, pp.scene_d(), flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    sv = gone.probes_survey(res["points"], spp=64, first_sample=500, max_distance=D)
    off, verdict = gone.probes_place(grid, sv, res["offsets"], min_front=0.2, want=("offsets", "verdict"))
    assert (verdict[near] == pr.PLACE_BACK).all() and not off.any()
    rt.close(); gone.close()


def test_a_probe_in_empty_space(pkg, pr, ga, ft):
    rt, res = on_device_and_statement(pkg, pr, ga, ft, pp.scene_d(), pp.GRID3, 2, spp=16)
    assert not res["offsets"].any() and (res["state"] == pr.IDLE).all() and (res["usable"] == 1).all() and (res["verdict"] == pr.PLACE_REST).all()
    rt.close()
