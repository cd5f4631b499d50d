"""Gather on the device (include/mi355rt.h "GATHER"): the light arriving at caller-given points.

The yardstick is the statement (raytracer_rs_amd.gather, numpy f32) over entries that are pinned elsewhere: gather must equal
gather.rays -> trace_rays(rgb, tuv, prim) -> gather.reduce on every bit (the radiance of trace_rays is held to the CPU oracle by tests/test_gpu_rays.py), the
hit counts are held to the CPU oracle's intersector directly, and `direct` to gather.direct over occluded_rays.  Points are hit points of the camera's rays
with the face normal turned against the ray; a few free-space points cover sphere mode.  No test feeds non-finite positions to the GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 16
SEED = 5
MISS = 0xFFFFFFFF
E_INVALID = -1
SAMPLED = ("n", "hits", "near", "sum", "sumsq")
ALL = SAMPLED + ("direct",)
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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


def surface(pkg, cams, scenes, name, scene=None):
    """(points, normals, ids) on the scene's surfaces: the hit points of the camera's rays (true closest hits), the face normal turned against the ray, and
    random ids with repeats; computed once per scene and never written to"""
    if name not in _POINTS:
        sc = scenes(name) if scene is None else scene
        rt = make(pkg, sc, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
        rays = cams.pinhole(rt.camera.matrices(), W, H, 8, SEED)
        tuv, prim = rt.intersect_rays(rays)
        rt.close()
        hit = np.nonzero(prim != MISS)[0]
        hit = hit[np.random.default_rng(2).permutation(hit.size)][:300]
        assert hit.size >= 257
        o, d, t = rays[hit, :3], rays[hit, 3:], tuv[hit, 0]
        pts = (o + t[:, None] * d).astype(F)
        v = sc["tri_verts"][prim[hit]].astype(np.float64)
        n = np.cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
        n /= np.linalg.norm(n, axis=1)[:, None]
        n[(n * d).sum(axis=1) > 0] *= -1
        ids = np.random.default_rng(4).integers(0, 2**32, hit.size, dtype=np.uint64).astype(np.uint32)
        ids[1::7] = ids[0]                                   # repeats
        res = (np.ascontiguousarray(pts), np.ascontiguousarray(n.astype(F)), ids)
        for a in res:
            a.setflags(write=False)
        _POINTS[name] = res
    return _POINTS[name]


def free_points(rt):
    """a few points in free space around the camera position (sphere mode)"""
    origin = rt.camera.matrices()[1][12:15]
    return np.ascontiguousarray(origin[None] + np.array([[0, 0, 0], [0.1, 0.2, -0.1], [-0.3, 0.1, 0.2], [0.05, -0.2, 0.3], [0.2, 0.2, 0.2]], F))


def statement(rt, ga, pts, nrm, ids, first, spp, weight="mean", near=np.inf, prev=None):
    """gather.rays -> trace_rays -> gather.reduce; returns (result, rays6)"""
    rays, keys, valid, w = ga.rays(rt.sample_table(), SEED, pts, nrm, ids, first, spp, weight)
    got = rt.trace_rays(rays, keys, want=("rgb", "tuv", "prim"))
    return ga.reduce(got["rgb"], got["tuv"][:, 0], got["prim"] != MISS, valid, w, near, prev), rays


def same(got, want, keys=SAMPLED):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


# ---- 1. the statement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4boxes", "ico3_tex"])
def test_gather_equals_the_statement(pkg, ga, cams, scenes, handles, sem3, name):
    pts, nrm, ids = surface(pkg, cams, scenes, name)
    rt = handles(name, flags=sem3.gpu)
    big, _ = statement(rt, ga, pts[:257], nrm[:257], ids[:257], 0, 8)
    tuv = rt.intersect_rays(ga.rays(rt.sample_table(), SEED, pts[:257], nrm[:257], ids[:257], 0, 8)[0])[0]
    near = float(np.median(tuv[:, 0][tuv[:, 0] > 0])) if (tuv[:, 0] > 0).any() else 1.0
    # the input decides something: light arrives, rays hit and miss
    assert big["sum"].any() and 0 < big["hits"].sum() < big["n"].sum()
    k = 0
    for npts in (1, 63, 64, 65, 257):
        for spp in (1, 3, 8):
            weight = ("mean", "cosine")[k % 2]; k += 1
            first = (0, 5, 0xFFFFFFF0)[k % 3]
            p, n, i = (np.ascontiguousarray(a[:npts]) for a in (pts, nrm, ids))
            want, _ = statement(rt, ga, p, n, i, first, spp, weight, near)
            got = rt.gather(p, n, i, spp=spp, first_sample=first, weight=weight, near_distance=near, want=SAMPLED)
            same(got, want)
            assert (got["n"] == spp).all()
            assert rt.last_counts().primary == npts * spp
    assert 0 < rt.gather(pts[:257], nrm[:257], ids[:257], spp=8, near_distance=near, want=("near",))["near"].sum() < big["hits"].sum()
    # ids=None is i
    want, _ = statement(rt, ga, pts[:65], nrm[:65], None, 2, 3)
    same(rt.gather(pts[:65], nrm[:65], None, spp=3, first_sample=2, want=SAMPLED), want)
    same(rt.gather(pts[:65], nrm[:65], np.arange(65, dtype=np.uint32), spp=3, first_sample=2, want=SAMPLED), want)
    # two points with the same id and the same normal take the same directions: at the same position, the same sums
    twin_p, twin_n = np.ascontiguousarray(pts[[3, 3, 9]]), np.ascontiguousarray(nrm[[3, 3, 9]])
    got = rt.gather(twin_p, twin_n, np.array([77, 77, 78], np.uint32), spp=8, want=SAMPLED)
    for key in SAMPLED:
        assert np.array_equal(got[key][0].view(np.uint32), got[key][1].view(np.uint32)), key
    # sphere mode: free-space points, no normals
    fp = free_points(rt)
    want, rays = statement(rt, ga, fp, None, None, 1, 8, "mean", near)
    same(rt.gather(fp, None, None, spp=8, first_sample=1, near_distance=near, want=SAMPLED), want)
    assert (want["n"] == 8).all()
    # only some outputs: each is what it is among all of them
    part = rt.gather(pts[:65], nrm[:65], None, spp=3, first_sample=2, want=("sumsq", "hits"))
    full, _ = statement(rt, ga, pts[:65], nrm[:65], None, 2, 3)
    assert set(part) == {"sumsq", "hits"}
    same(part, full, ("sumsq", "hits"))
    assert (rt.gather(pts[:65], nrm[:65], None, spp=3, want=("n",))["n"] == 3).all()


# ---- 2. the oracle: the independent side ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4boxes", "ico3_tex"])
def test_hits_and_near_equal_the_oracles_intersector(pkg, oracle, ga, cams, scenes, handles, sem, name):
    pts, nrm, ids = surface(pkg, cams, scenes, name)
    rt = handles(name, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), W, H, seed=SEED, flags=sem.orc)
    npts, spp, first = 130, 5, 2
    for normals, points in ((nrm[:npts], pts[:npts]), (None, free_points(rt))):
        n = len(points)
        rays, keys, valid, w = ga.rays(orc.sample_table(), SEED, points, normals, ids[:n], first, spp)
        tuv, prim = orc.intersect(rays, brute=bool(sem.orc & oracle.FLAG_BRUTE_FORCE))
        hit = (prim != MISS).reshape(spp, n)
        near = float(np.median(tuv[prim != MISS, 0])) if hit.any() else 1.0
        got = rt.gather(points, normals, ids[:n], spp=spp, first_sample=first, near_distance=near, want=("n", "hits", "near"))
        assert np.array_equal(got["hits"], hit.sum(axis=0).astype(np.uint32))
        assert np.array_equal(got["near"], (hit & (tuv[:, 0].reshape(spp, n) < F(near))).sum(axis=0).astype(np.uint32))
        assert (got["n"] == spp).all() and valid.all()
        assert normals is None or 0 < got["near"].sum() < got["hits"].sum()
    orc.close()


# ---- 3. chunks ----------------------------------------------------------------------------------------------------------------------------------------------
def test_chunks_cut_points_and_samples(pkg, ga, cams, scenes, handles, sem3):
    """An 8 x 8 handle with samples_per_pass = 1 has passes of 64 rays.  65 points x 3 spp on it: chunks of 64 points and of 1, one sample each.  20 points x 8
    spp: chunks of 3, 3 and 2 samples, in ascending order.  Every output equals the same call on a default handle (one chunk).  A striped handle serves the
    call as an unstriped one does."""
    pts, nrm, ids = surface(pkg, cams, scenes, "4boxes")
    rt = handles("4boxes", flags=sem3.gpu)
    small = make(pkg, scenes("4boxes"), 8, 8, flags=sem3.gpu, samples_per_pass=1)
    striped = make(pkg, scenes("4boxes"), flags=sem3.gpu, stripe_rows=2, stripe_rank=1, stripe_world=3)
    tuv = rt.intersect_rays(ga.rays(rt.sample_table(), SEED, pts[:65], nrm[:65], ids[:65], 0, 3)[0])[0]
    near = float(np.median(tuv[:, 0][tuv[:, 0] > 0]))
    for npts, spp, weight in ((65, 3, "cosine"), (20, 8, "mean"), (64, 1, "mean"), (130, 2, "cosine")):
        p, n, i = (np.ascontiguousarray(a[:npts]) for a in (pts, nrm, ids))
        want = rt.gather(p, n, i, spp=spp, first_sample=1, weight=weight, near_distance=near, want=ALL)
        same(want, statement(rt, ga, p, n, i, 1, spp, weight, near)[0])
        for other in (small, striped):
            got = other.gather(p, n, i, spp=spp, first_sample=1, weight=weight, near_distance=near, want=ALL)
            same(got, want, ALL)
            assert other.last_counts().primary == npts * spp
    # accumulating across calls on the chunked handle
    a = small.gather(pts[:65], nrm[:65], ids[:65], spp=3, want=SAMPLED)
    b = small.gather(pts[:65], nrm[:65], ids[:65], spp=5, first_sample=3, want=SAMPLED, into=a)
    same(b, rt.gather(pts[:65], nrm[:65], ids[:65], spp=8, want=SAMPLED))
    small.close(); striped.close()


# ---- 4. accumulate -----------------------------------------------------------------------------------------------------------------------------------------
def test_accumulate(pkg, ga, cams, scenes, handles, sem3):
    pts, nrm, ids = surface(pkg, cams, scenes, "ico3_tex")
    rt = handles("ico3_tex", flags=sem3.gpu)
    p, n, i = (np.ascontiguousarray(a[:65]) for a in (pts, nrm, ids))
    one = rt.gather(p, n, i, spp=8, weight="cosine", near_distance=3.0, want=SAMPLED)
    a = rt.gather(p, n, i, spp=3, weight="cosine", near_distance=3.0, want=SAMPLED)
    first = {k: v.copy() for k, v in a.items()}
    b = rt.gather(p, n, i, spp=5, first_sample=3, weight="cosine", near_distance=3.0, want=SAMPLED, into=a)
    same(b, one)
    assert all(b[k] is a[k] for k in SAMPLED)                      # added to in place
    assert (first["n"] == 3).all() and (b["n"] == 8).all()
    # without `into` the outputs start from 0 whatever they held
    c = rt.gather(p, n, i, spp=3, weight="cosine", near_distance=3.0, want=SAMPLED)
    same(c, first)
    # `into` with `direct`: direct is overwritten, never accumulated
    d1 = rt.gather(p, n, i, spp=1, want=("n", "direct"))
    d2 = rt.gather(p, n, i, spp=1, first_sample=1, want=("n", "direct"), into=dict(n=d1["n"]))
    assert (d2["n"] == 2).all() and np.array_equal(bits(d2["direct"]), bits(d1["direct"]))
    with pytest.raises(ValueError, match="into"):
        rt.gather(p, n, i, spp=1, want=("n", "sum"), into=dict(n=d1["n"]))


# ---- 5. direct ---------------------------------------------------------------------------------------------------------------------------------------------
def three_lights(scene):
    """4boxes with three lights: its own, one far below the floor of the boxes (behind most upward faces), one to the side"""
    sc = dict(scene)
    own = scene["lights"][0]
    sc["lights"] = np.array([own, [own[0], own[1] - 40.0, own[2], 0.25, 0.5, 1.0], [own[0] + 6.0, own[1] + 1.0, own[2] - 2.0, 0.9, 0.1, 0.3]], F)
    return sc


@pytest.mark.parametrize("name", ["4boxes", "ico3_tex", "three_lights"])
def test_direct(pkg, ga, cams, scenes, sem3, name):
    scene = three_lights(scenes("4boxes")) if name == "three_lights" else scenes(name)
    pts, nrm, ids = surface(pkg, cams, scenes, name, scene)
    rt = make(pkg, scene, flags=sem3.gpu)
    lights = np.ascontiguousarray(scene["lights"], F)
    assert rt.nlights == len(lights) >= 1
    l = lights[:, None, :3] - pts[None]
    ndl = (nrm[None] * (l / np.linalg.norm(l, axis=2)[:, :, None])).sum(axis=2)
    for npts in (1, 65, 257):
        p, n = np.ascontiguousarray(pts[:npts]), np.ascontiguousarray(nrm[:npts])
        blocked = rt.occluded_rays(ga.shadow_rays(p, lights))
        want = ga.direct(p, n, lights, blocked)
        got = rt.gather(p, n, None, spp=0, want=("direct",))["direct"]
        assert np.array_equal(bits(got), bits(want))
        both = rt.gather(p, n, None, spp=2, want=("direct", "n"))
        assert np.array_equal(bits(both["direct"]), bits(want)) and (both["n"] == 2).all()
    blocked = rt.occluded_rays(ga.shadow_rays(pts[:257], lights)).reshape(len(lights), 257).astype(bool)
    assert want.any() and blocked.any() and not blocked.all()
    if name == "three_lights":
        assert (ndl[1, :257] < -0.01).any() and (ndl[1, :257] > 0.01).any()     # a light behind some surfaces: skipped there, whatever its shadow ray says
    # one light, nothing in the way: color * ndl, recomputed here
    if len(lights) == 1:
        free = ~blocked[0]
        lv = lights[0, :3][None] - pts[:257]
        ln = lv / np.sqrt(lv[:, 0] * lv[:, 0] + lv[:, 1] * lv[:, 1] + lv[:, 2] * lv[:, 2])[:, None]
        d = nrm[:257, 0] * ln[:, 0] + nrm[:257, 1] * ln[:, 1] + nrm[:257, 2] * ln[:, 2]
        lit = free & ~(d < 0)
        assert lit.any()
        assert np.array_equal(bits(got[lit]), bits(np.zeros(3, F)[None] + lights[0, 3:][None] * d[lit, None]))
        assert not got[~lit].any()
    rt.close()


# ---- 6. void -----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_zero_normal_is_void_and_harms_no_neighbour(pkg, ga, cams, scenes, handles):
    """Runs only after tests/test_gather_abi.py passes: that file shows on the CPU, through the very header gather_rays_kernel compiles (csrc/gather_walk.hpp),
    that the walk on a zero normal returns after one turn of the table with valid == 0.  Here: such a point has n == 0 and sums of 0, and its neighbours are what
    they are in a call without it."""
    pts, nrm, ids = surface(pkg, cams, scenes, "4boxes")
    rt = handles("4boxes")
    p, i = np.ascontiguousarray(pts[:65]), np.ascontiguousarray(ids[:65])
    n = nrm[:65].copy()
    n[7] = 0.0; n[64] = [-0.0, 0.0, 0.0]
    srays, _, svalid, _ = ga.rays(rt.sample_table(), SEED, p, n, i, 0, 3)
    assert not svalid[:, [7, 64]].any() and svalid[:, :7].all() and np.isfinite(srays).all()
    got = rt.gather(p, n, i, spp=3, near_distance=3.0, want=SAMPLED)
    same(got, statement(rt, ga, p, n, i, 0, 3, "mean", 3.0)[0])
    for k in SAMPLED:
        assert not got[k][[7, 64]].view(np.uint32).any(), k
    keep = np.ones(65, bool); keep[[7, 64]] = False
    without = rt.gather(np.ascontiguousarray(p[keep]), np.ascontiguousarray(n[keep]), np.ascontiguousarray(i[keep]), spp=3, near_distance=3.0, want=SAMPLED)
    for k in SAMPLED:
        assert np.array_equal(got[k][keep].view(np.uint32), without[k].view(np.uint32)), k
    assert (got["n"][keep] == 3).all()
    # accumulating onto a void point leaves what it held
    again = rt.gather(p, n, i, spp=2, first_sample=3, near_distance=3.0, want=SAMPLED, into=got)
    assert not again["n"][[7, 64]].any() and (again["n"][keep] == 5).all()


# ---- 7. device memory, and what a gather leaves alone -----------------------------------------------------------------------------------------------------
def test_device_tensors_and_an_untouched_handle(pkg, ga, cams, scenes, sem3):
    import torch
    pts, nrm, ids = surface(pkg, cams, scenes, "4boxes")
    rt = make(pkg, scenes("4boxes"), flags=sem3.gpu | pkg.FLAG_DIRECT_FILM | pkg.FLAG_LIGHT_FILMS)
    rt.set_lens("thin", radius=0.05, focus=4.0)
    rt.render(2)
    s, q, n = rt.film.pixel_datas()
    before = (bits(s).copy(), bits(q).copy(), n.copy(), bits(rt.film.direct_sums()).copy(), bits(rt.light_films.get()).copy())
    row, cam, lens = rt.current_row, [a.copy() for a in rt.camera.matrices()], rt.lens.as_dict()
    p, nn, i = (np.ascontiguousarray(a[:130]) for a in (pts, nrm, ids))
    host = rt.gather(p, nn, i, spp=3, weight="cosine", near_distance=3.0, want=ALL)
    dev = torch.device("cuda", 0)
    tp, tn, ti = torch.from_numpy(p.copy()).to(dev), torch.from_numpy(nn.copy()).to(dev), torch.from_numpy(i.copy().view(np.int32)).to(dev)
    got = rt.gather(tp, tn, ti, spp=3, weight="cosine", near_distance=3.0, want=ALL)
    hbm = rt.hbm_allocated_bytes()
    got = rt.gather(tp, tn, ti, spp=3, weight="cosine", near_distance=3.0, want=ALL)
    assert rt.hbm_allocated_bytes() == hbm
    for k in ALL:
        assert isinstance(got[k], torch.Tensor) and got[k].device == dev
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), host[k].view(np.uint32)), k
    # in place on the device: accumulate into tensors
    a = rt.gather(tp, tn, ti, spp=1, want=SAMPLED)
    b = rt.gather(tp, tn, ti, spp=2, first_sample=1, want=SAMPLED, into=a)
    assert all(b[k] is a[k] for k in SAMPLED)
    one = rt.gather(p, nn, i, spp=3, want=SAMPLED)
    for k in SAMPLED:
        assert np.array_equal(b[k].cpu().numpy().view(np.uint32), one[k].view(np.uint32)), k
    hbm_host = rt.hbm_allocated_bytes()
    rt.gather(p, nn, i, spp=3, want=ALL)
    assert rt.hbm_allocated_bytes() == hbm_host == hbm
    with pytest.raises(ValueError, match="GPU"):
        rt.gather(tp.cpu(), None)
    with pytest.raises(ValueError, match="normals must live where points live"):
        rt.gather(tp, nn)
    with pytest.raises(TypeError, match="dtype"):
        rt.gather(tp.double(), None)
    # the handle is what it was: film, direct film, light films, current row, camera, lens; the caller-ray mark is not set (the denoiser still answers)
    s, q, n = rt.film.pixel_datas()
    after = (bits(s), bits(q), n, bits(rt.film.direct_sums()), bits(rt.light_films.get()))
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert rt.current_row == row and rt.lens.as_dict() == lens
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(cam, rt.camera.matrices()))
    rt.get_denoised_pixels()
    # ... and the next samples of the film are the ones it would have taken without the gather
    twin = make(pkg, scenes("4boxes"), flags=sem3.gpu | pkg.FLAG_DIRECT_FILM | pkg.FLAG_LIGHT_FILMS)
    twin.set_lens("thin", radius=0.05, focus=4.0)
    twin.render(2); twin.render(1); rt.render(1)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(rt.film.pixel_datas()[:2], twin.film.pixel_datas()[:2]))
    rt.close(); twin.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------------------------
GUARD = 4


def raw_gather(pkg, rt, points, normals, ids, npoints, want=ALL, where=0, null_cfg=False, **cfg_kw):
    """mi355rt_gather through ctypes into sentinel-filled outputs; returns (code, {name: uint32 array})"""
    cfg = pkg.GatherConfig()
    pkg.lib().mi355rt_gather_default_config(C.byref(cfg))
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    o, arrs = pkg.GatherOutputs(), {}
    for w in want:
        arrs[w] = np.full((npoints + GUARD) * (3 if w in ("sum", "sumsq", "direct") else 1), 0xA5A5A5A5, np.uint32)
        setattr(o, w, arrs[w].ctypes.data)
    ptr = lambda a: None if a is None else a.ctypes.data
    code = pkg.lib().mi355rt_gather(rt._h, ptr(points), ptr(normals), ptr(ids), npoints, None if null_cfg else C.byref(cfg), where, C.byref(o))
    return code, arrs


def test_errors_name_the_argument_and_write_nothing(pkg, cams, scenes):
    pts, nrm, ids = surface(pkg, cams, scenes, "4boxes")
    p, n, i = (np.ascontiguousarray(a[:10]) for a in (pts, nrm, ids))
    rt = make(pkg, scenes("4boxes"))
    rt.render(1)
    s, q, cnt = rt.film.pixel_datas()
    film = (bits(s).copy(), bits(q).copy(), cnt.copy())
    lib = pkg.lib()
    err = lambda h=rt: (lib.mi355rt_last_error(h._h) or b"").decode()

    def refused(result, *names):
        code, arrs = result
        assert code == E_INVALID
        assert "mi355rt_gather" in err() and all(nm in err() for nm in names), err()
        assert all(np.all(v == 0xA5A5A5A5) for v in arrs.values())
        s2, q2, n2 = rt.film.pixel_datas()
        assert np.array_equal(bits(s2), film[0]) and np.array_equal(bits(q2), film[1]) and np.array_equal(n2, film[2])

    refused(raw_gather(pkg, rt, None, n, i, 10), "points3")
    refused(raw_gather(pkg, rt, p, n, i, 10, want=()), "out")
    cfg = pkg.GatherConfig(); lib.mi355rt_gather_default_config(C.byref(cfg))
    assert lib.mi355rt_gather(rt._h, p.ctypes.data, n.ctypes.data, None, 10, C.byref(cfg), 0, None) == E_INVALID and "out" in err()
    refused(raw_gather(pkg, rt, p, n, i, 10, null_cfg=True), "cfg")
    refused(raw_gather(pkg, rt, p, n, i, 10, want=("n", "direct"), spp=0), "spp")
    refused(raw_gather(pkg, rt, p, n, i, 10, want=("sum",), spp=0), "spp")
    refused(raw_gather(pkg, rt, p, None, i, 10, want=SAMPLED, weight=pkg.GATHER_COSINE), "COSINE", "normals3")
    refused(raw_gather(pkg, rt, p, None, i, 10, want=("direct",)), "direct", "normals3")
    refused(raw_gather(pkg, rt, p, n, i, 10, weight=2), "weight")
    refused(raw_gather(pkg, rt, p, n, i, 10, where=2), "where")
    refused(raw_gather(pkg, rt, p, n, i, 10, near_distance=float("nan")), "near_distance")
    refused(raw_gather(pkg, rt, p, n, i, 10, spp=2**32 // 10 + 1), "npoints * spp")
    refused(raw_gather(pkg, rt, p, n, i, 10, spp=3, first_sample=0xFFFFFFFE), "first_sample")
    # what is allowed right at those edges
    code, arrs = raw_gather(pkg, rt, p, n, i, 10, want=("n",), spp=2, first_sample=0xFFFFFFFD)
    assert code == 0 and (arrs["n"][:10] == 2).all() and (arrs["n"][10:] == 0xA5A5A5A5).all()
    code, arrs = raw_gather(pkg, rt, p, n, i, 10, want=("direct",), spp=0)
    assert code == 0 and (arrs["direct"][30:] == 0xA5A5A5A5).all() and not (arrs["direct"][:30] == 0xA5A5A5A5).any()
    code, arrs = raw_gather(pkg, rt, p, None, None, 10, near_distance=float("-inf"), want=SAMPLED, spp=1)
    assert code == 0 and not arrs["near"][:10].any() and all((v[10 * (3 if k in ("sum", "sumsq") else 1):] == 0xA5A5A5A5).all() for k, v in arrs.items())
    # npoints == 0 succeeds and writes nothing, with or without pointers
    code, arrs = raw_gather(pkg, rt, p, n, i, 0)
    assert code == 0 and all(np.all(v == 0xA5A5A5A5) for v in arrs.values())
    code, arrs = raw_gather(pkg, rt, None, None, None, 0, want=("n",))
    assert code == 0 and np.all(arrs["n"] == 0xA5A5A5A5)
    assert rt.gather(np.zeros((0, 3), F), want=("n", "sum"))["sum"].shape == (0, 3)
    # the Python face
    with pytest.raises(ValueError, match="want"):
        rt.gather(p, n, want=("rgb",))
    with pytest.raises(ValueError, match="weight"):
        rt.gather(p, n, weight="sine")
    with pytest.raises(ValueError, match="shape"):
        rt.gather(p, np.ascontiguousarray(n[:9]))
    with pytest.raises(RuntimeError, match="normals3"):
        rt.gather(p, None, weight="cosine")
    rt.get_denoised_pixels()
    rt.close()
    # a device group (here: two members sharing the one GPU) refuses
    g = make(pkg, scenes("4boxes"), device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    code, arrs = raw_gather(pkg, g, p, n, i, 10)
    assert code == E_INVALID and "device group" in err(g) and "mi355rt_gather" in err(g) and all(np.all(v == 0xA5A5A5A5) for v in arrs.values())
    g.close()
