"""Probe-lit shading on the device (include/mi355rt.h "PROBE-LIT"): closest hit, shade() with shadow rays and the hemisphere mean of a probe
volume along caller-given rays, and that mean at caller-given surface points.

The yardstick is the statement (raytracer_rs_amd.probe_lit, numpy f32) over entries that are pinned elsewhere: given intersect_rays' and occluded_rays'
answers for the same handle, every output of probe_lit_rays must equal probe_lit.rays on every bit, `light` must equal trace_rays' `direct` on every bit, and
probe_lit_points must equal probe_lit.hemi.  tests/test_probe_lit_abi.py holds the statement to the CPU oracle and to the analytic hemisphere mean."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import probe_lit_cases as plc
import probe_vis_cases as pv

pytestmark = pytest.mark.gpu

W, H = plc.W, plc.H
SEED = plc.SEED
MISS = plc.MISS
F = np.float32
bits = plc.bits
COUNTS = (1, 63, 64, 65, 257)                       # the block is 256 lanes, one per ray: 1, a wave but one, a wave, a wave and one, a block and one
GRIDS = ((2, 2, 2), (3, 2, 4), (1, 3, 2))
KEYS = ("rgb", "light", "indirect", "tuv", "prim", "ok")


@pytest.fixture(scope="module")
def plit(pkg):
    return importlib.import_module("raytracer_rs_amd.probe_lit")


@pytest.fixture(scope="module")
def pr(pkg):
    return importlib.import_module("raytracer_rs_amd.probes")


def make(pkg, scene, w=W, h=H, **kw):
    kw.setdefault("seed", SEED)
    return pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, **kw)


@pytest.fixture(scope="module")
def handles(pkg, scenes):
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = make(pkg, plc.scene_of(scenes, name), **kw)
        return made[key]
    yield get
    for rt in made.values():
        rt.close()


_VOLUMES = {}


def volume_of(handles, pr, plit, scenes, name, counts, relocated, states):
    """A volume gathered on the device at 8 spp with depth films of 4 x 4 texels over the scene's box; relocated: at the offsets of two rounds of relocation;
    states: with the usable mask of the probes' states.  Made once, by the default handle of the scene, and never written to"""
    key = (name, counts, relocated, states)
    if key not in _VOLUMES:
        rt = handles(name)
        v = np.asarray(plc.scene_of(scenes, name)["tri_verts"], F).reshape(-1, 3)
        grid = pr.grid_over(v.min(axis=0) - F(0.5), v.max(axis=0) + F(0.5), counts)
        rel = rt.probes_relocate(grid, rounds=2 if relocated else 0, spp=8)
        res = rt.probes_gather_depth(rel["points"], spp=8, res=4, max_distance=pr.grid_max_distance(grid))
        vol = plit.volume(grid, res, depth=res, usable=rel["usable"] if states else None, offsets=rel["offsets"] if relocated else None, normal_bias=0.01 * len(_VOLUMES))
        assert (np.asarray(vol["n"]) == 8).all()
        _VOLUMES[key] = vol
    return _VOLUMES[key]


def all_volumes(handles, pr, plit, scenes, name):
    out = [volume_of(handles, pr, plit, scenes, name, counts, relocated, states) for counts in GRIDS for relocated, states in ((False, False), (True, True))]
    out += [volume_of(handles, pr, plit, scenes, name, GRIDS[1], True, False), volume_of(handles, pr, plit, scenes, name, GRIDS[0], False, True)]
    nodepth = dict(out[0], depth=None, chebyshev=False, facing=False, normal_bias=0.0)
    return out + [nodepth, plc.hand_volume(plit)]


def rays_for(rt, scenes, name, spp=4):
    """the hand-made rays, then the handle's lens rays in an order that mixes hits and misses three to one (in pixel order a block would be mostly sky)"""
    sc = plc.scene_of(scenes, name)
    origin = rt.camera.matrices()[1][12:15]
    v = np.asarray(sc["tri_verts"], F).reshape(-1, 9)
    inside = v[:12].reshape(-1, 3).mean(axis=0) if name != "ico3_tex" else v.reshape(-1, 3).mean(axis=0)      # the middle of the first box; the middle of the ball
    lens = rt.lens_rays(spp)
    hit = rt.intersect_rays(lens)[1] != MISS
    h, m, order = list(np.nonzero(hit)[0]), list(np.nonzero(~hit)[0]), []
    while h or m:
        order += h[:3] + m[:1]
        h, m = h[3:], m[1:]
    return np.ascontiguousarray(np.concatenate([plc.hand_rays(origin, inside), lens[order]]).astype(F))


def statement(rt, plit, sc, vol, rays, clamp=True, before=None):
    tuv, prim = rt.intersect_rays(rays)
    blocked = rt.occluded_rays(plit.shadow_rays(sc, rays, tuv, prim)) if len(sc["lights"]) else np.zeros(0, np.uint8)
    return plit.rays(sc, vol, rays, tuv, prim, blocked, clamp, before)


def same_bits(a, b):
    """bit for bit; a NaN equals a NaN whatever its sign and payload (a NaN ray is data, and what it makes is a NaN on either side)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32:
        return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype.itemsize == 4 else a, b.view(np.uint32) if b.dtype.itemsize == 4 else b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def same(got, want, keys=KEYS):
    for k in keys:
        assert tuple(got[k].shape) == want[k].shape and got[k].dtype == want[k].dtype, k
        assert same_bits(got[k], want[k]), k


# ---- 1. the statement -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", plc.SCENES)
def test_probe_lit_rays_equals_the_statement(pkg, plit, pr, scenes, handles, sem3, name):
    sc = plc.scene_of(scenes, name)
    rt = handles(name, flags=sem3.gpu)
    rays = rays_for(rt, scenes, name)
    vols = all_volumes(handles, pr, plit, scenes, name)
    assert len(rays) >= 257 + 16
    hits = oks = 0
    for k, (vol, n) in enumerate(itertools.product(vols, COUNTS)):
        if n == 257 and k % 3:                                                       # the full block for every third volume
            continue
        r = np.ascontiguousarray(rays[:n] if n > 1 else rays[16 + 5 * (k % 30):][:1])
        clamp = bool((k // len(COUNTS)) % 2 == 0)
        before = np.full((len(r), 3), 7.0, F)
        want = statement(rt, plit, sc, vol, r, clamp, before)
        into = dict(tuv=before.copy())
        got = rt.probe_lit_rays(vol, r, want=KEYS, clamp=clamp, into=into)
        assert got["tuv"] is into["tuv"]
        same(got, want)
        c = rt.last_counts()
        assert (c.primary, c.bounce, c.shadow) == (len(r), 0, 0)                       # the shadow rays go through occluded_rays' launch, which counts nothing
        hit = want["prim"] != MISS
        # tuv, prim equal intersect_rays; light equals trace_rays' direct, bit for bit
        tr = rt.trace_rays(r, want=("direct", "tuv", "prim"))
        assert np.array_equal(got["prim"], tr["prim"]) and same_bits(got["tuv"][hit], tr["tuv"][hit]) and (got["tuv"][~hit] == 7.0).all()
        assert same_bits(got["light"], tr["direct"])
        with np.errstate(all="ignore"):
            assert same_bits(got["rgb"], got["light"] + got["indirect"])
        assert (bits(got["rgb"][~hit]) == 0).all() and (got["ok"][~hit] == 0).all()
        # probe_lit_points at the statement's P, N gives the same indirect
        if hit.any():
            P, N = np.ascontiguousarray(want["points"][hit]), np.ascontiguousarray(want["normals"][hit])
            ind, ok = rt.probe_lit_points(vol, P, N, clamp=clamp, want_ok=True)
            assert same_bits(ind, got["indirect"][hit]) and np.array_equal(ok, got["ok"][hit])
            assert same_bits(ind, plit.hemi(vol, P, N, clamp)[0])
            assert rt.last_counts().primary == len(r)                                 # the lookup traces nothing and reports nothing
        hits += int(hit.sum()); oks += int(got["ok"].sum())
    assert hits > 1000 and oks > 100
    # the hand-made rays are data: a zero direction hits nothing, the rays at the scene hit it, and misses and hits are both among the rest
    w16 = statement(rt, plit, sc, vols[0], rays[:16])
    assert (w16["prim"][[8, 9]] == MISS).all() and (w16["prim"][13:16] != MISS).all() and (w16["prim"][:8] == MISS).any()


def test_every_subset_of_outputs_gives_the_same_bits(pkg, plit, pr, scenes, handles):
    name = "4boxes_3lights"
    rt = handles(name)
    rays = np.ascontiguousarray(rays_for(rt, scenes, name)[:65])
    vol = volume_of(handles, pr, plit, scenes, name, GRIDS[1], True, True)
    full = rt.probe_lit_rays(vol, rays, want=KEYS, into=dict(tuv=np.full((65, 3), 7.0, F)))
    for m in range(1, 1 << len(KEYS)):
        want = tuple(k for i, k in enumerate(KEYS) if m >> i & 1)
        got = rt.probe_lit_rays(vol, rays, want=want, into=dict(tuv=np.full((65, 3), 7.0, F)))
        assert tuple(got) == want
        same(got, full, want)
    with pytest.raises(ValueError, match="want"):
        rt.probe_lit_rays(vol, rays, want=())
    with pytest.raises(ValueError, match="want"):
        rt.probe_lit_rays(vol, rays, want=("rgb", "direct"))


# ---- 2. chunks, stripes ---------------------------------------------------------------------------------------------------------------------------------
def test_chunks_and_stripes(pkg, plit, pr, scenes, handles, sem3, monkeypatch):
    """2 500 rays under MI355RT_PASS_SAMPLES=1024 run as chunks of 1024, 1024 and 452: the bits of the uncut run.  A striped handle serves both entries."""
    name = "4boxes_3lights"
    sc = plc.scene_of(scenes, name)
    rt = handles(name, flags=sem3.gpu)
    rays = np.ascontiguousarray(rt.lens_rays(14)[:2500])
    vol = volume_of(handles, pr, plit, scenes, name, GRIDS[1], True, True)
    before = np.full((2500, 3), 7.0, F)
    whole = rt.probe_lit_rays(vol, rays, want=KEYS, into=dict(tuv=before.copy()))
    same(whole, statement(rt, plit, sc, vol, rays, True, before))
    hbm = rt.hbm_allocated_bytes()
    monkeypatch.setenv("MI355RT_PASS_SAMPLES", "1024")
    cut = rt.probe_lit_rays(vol, rays, want=KEYS, into=dict(tuv=before.copy()))
    monkeypatch.delenv("MI355RT_PASS_SAMPLES")
    same(cut, whole)
    assert rt.last_counts().primary == 2500 and rt.hbm_allocated_bytes() == hbm
    striped = make(pkg, sc, flags=sem3.gpu, stripe_rows=2, stripe_rank=1, stripe_world=3)
    same(striped.probe_lit_rays(vol, rays[:300], want=KEYS, into=dict(tuv=before[:300].copy())), {k: v[:300] for k, v in whole.items()})
    hit = whole["prim"][:300] != MISS
    st = statement(rt, plit, sc, vol, rays[:300])
    P, N = np.ascontiguousarray(st["points"][hit]), np.ascontiguousarray(st["normals"][hit])
    assert np.array_equal(bits(striped.probe_lit_points(vol, P, N)), bits(whole["indirect"][:300][hit]))
    striped.close()


# ---- 3. device memory, refusals, and what the calls leave alone -------------------------------------------------------------------------------------------
def test_device_tensors_refusals_and_an_untouched_handle(pkg, plit, pr, scenes, handles, sem3):
    import torch
    name = "4boxes_3lights"
    sc = plc.scene_of(scenes, name)
    vol = volume_of(handles, pr, plit, scenes, name, GRIDS[1], True, True)
    rt = make(pkg, sc, flags=sem3.gpu | pkg.FLAG_DIRECT_FILM | pkg.FLAG_LIGHT_FILMS)
    rt.set_lens("thin", radius=0.05, focus=4.0)
    rt.render(2)
    s, q, n = rt.film.pixel_datas()
    film_before = (bits(s).copy(), bits(q).copy(), n.copy(), bits(rt.film.direct_sums()).copy(), bits(rt.light_films.get()).copy())
    row, cam, lens = rt.current_row, [a.copy() for a in rt.camera.matrices()], rt.lens.as_dict()
    rays = np.ascontiguousarray(rays_for(rt, scenes, name)[:257])
    before = np.full((257, 3), 7.0, F)
    host = rt.probe_lit_rays(vol, rays, want=KEYS, into=dict(tuv=before.copy()))
    same(host, statement(rt, plit, sc, vol, rays, True, before))
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a.view(np.int32).copy() if a.dtype == np.uint32 else a.copy()).to(dev)
    tvol = dict(vol, n=t(vol["n"]), sh=t(vol["sh"]), usable=t(vol["usable"]), offsets=t(vol["offsets"]),
                depth=dict(vol["depth"], count=t(vol["depth"]["count"]), moments=t(vol["depth"]["moments"])))
    trays = t(rays)
    tinto = dict(tuv=t(before))
    got = rt.probe_lit_rays(tvol, trays, want=KEYS, into=tinto)
    hbm = rt.hbm_allocated_bytes()
    got = rt.probe_lit_rays(tvol, trays, want=KEYS, into=tinto)
    assert rt.hbm_allocated_bytes() == hbm                                            # every temporary, the chunk's among them, is freed and counted
    assert got["tuv"] is tinto["tuv"]                                                 # used in place
    for k in KEYS:
        assert isinstance(got[k], torch.Tensor) and got[k].device == dev
        a = got[k].cpu().numpy()
        assert np.array_equal(a if k == "ok" else a.view(np.uint32), host[k] if k == "ok" else host[k].view(np.uint32)), k
    assert got["prim"].dtype == torch.int32 and got["ok"].dtype == torch.uint8
    hit = host["prim"] != MISS
    st = statement(rt, plit, sc, vol, rays)
    P, N = np.ascontiguousarray(st["points"][hit]), np.ascontiguousarray(st["normals"][hit])
    counts_before = rt.last_counts().as_dict()
    tind, tok = rt.probe_lit_points(tvol, t(P), t(N), want_ok=True)
    assert isinstance(tind, torch.Tensor) and tind.device == dev and tok.dtype == torch.uint8
    assert np.array_equal(bits(tind.cpu().numpy()), bits(host["indirect"][hit])) and np.array_equal(tok.cpu().numpy(), host["ok"][hit])
    assert np.array_equal(bits(rt.probe_lit_points(vol, P, N)), bits(host["indirect"][hit]))
    assert rt.hbm_allocated_bytes() == hbm and rt.last_counts().as_dict() == counts_before
    with pytest.raises(ValueError, match="must live where"):
        rt.probe_lit_rays(vol, trays)
    with pytest.raises(ValueError, match="must live where"):
        rt.probe_lit_points(tvol, P, N)
    with pytest.raises(ValueError, match="one place"):
        rt.probe_lit_rays(dict(tvol, n=vol["n"]), trays)
    # every refusal leaves its outputs untouched
    lib = pkg.lib()
    last_error = lambda: (lib.mi355rt_last_error(rt._h) or b"").decode()
    v, keep = plc.c_volume(pkg, vol)
    out = {k: np.full((257,) if k in ("prim", "ok") else (257, 3), 7, np.uint32 if k == "prim" else np.uint8 if k == "ok" else F) for k in KEYS}
    o = pkg.ProbeLitOutputs(*[out[k].ctypes.data for k in KEYS])
    ind = np.full((257, 3), 7.0, F); okb = np.full(257, 7, np.uint8)

    def refused_rays(msg, vv=v, r=rays, nr=257, flags=1, where=0, oo=o):
        code = lib.mi355rt_probe_lit_rays(rt._h, None if vv is None else C.byref(vv), None if r is None else r.ctypes.data, nr, flags, where, None if oo is None else C.byref(oo))
        assert code == -1 and last_error() == "mi355rt_probe_lit_rays: " + msg, (code, last_error())
        assert all((a == 7).all() for a in out.values())

    def refused_points(msg, vv=v, p=P, nn=N, flags=1, where=0, i=ind):
        code = lib.mi355rt_probe_lit_points(rt._h, None if vv is None else C.byref(vv), None if p is None else p.ctypes.data, None if nn is None else nn.ctypes.data, len(P), flags,
                                            where, None if i is None else i.ctypes.data, okb.ctypes.data)
        assert code == -1 and last_error() == "mi355rt_probe_lit_points: " + msg, (code, last_error())
        assert (ind == 7.0).all() and (okb == 7).all()

    for refused in (refused_rays, refused_points):
        refused("volume is NULL", vv=None)
        refused("unknown `where` (MI355RT_RAYS_HOST or MI355RT_RAYS_DEVICE)", where=2)
        refused("flags: unknown bits (MI355RT_PROBE_LIT_CLAMP)", flags=2)
        b, k = plc.c_volume(pkg, vol); b.sh = None
        refused("volume.sh is NULL", vv=b)
        b, k = plc.c_volume(pkg, vol); b.depth = None
        refused("volume.vc is given without volume.depth", vv=b)
        b, k = plc.c_volume(pkg, vol); b.depth = None; b.vc = None
        refused("volume.offsets is given without volume.depth", vv=b)
        off = np.array(vol["offsets"], F, copy=True); off[3, 1] = np.inf
        b, k = plc.c_volume(pkg, dict(vol, offsets=off))
        refused("volume.offsets holds a value that is not finite", vv=b)
        vc = pkg.ProbeVisConfig(8, 0.0)
        b, k = plc.c_volume(pkg, vol); b.vc = C.pointer(vc)
        refused("vc.flags: unknown bits (MI355RT_VIS_CHEBYSHEV, MI355RT_VIS_FACING)", vv=b)
    refused_rays("out is NULL or every output pointer in it is NULL", oo=None)
    refused_rays("out is NULL or every output pointer in it is NULL", oo=pkg.ProbeLitOutputs())
    refused_rays("rays6 is NULL", r=None)
    refused_rays("nrays * max(nlights, 1) must be < 2^32", nr=(1 << 32) // 3 + 1)
    refused_points("points3 is NULL", p=None)
    refused_points("normals3 is NULL", nn=None)
    refused_points("indirect3 is NULL", i=None)
    # a count of 0 succeeds and writes nothing
    assert lib.mi355rt_probe_lit_rays(rt._h, C.byref(v), None, 0, 1, 0, C.byref(o)) == 0 and all((a == 7).all() for a in out.values())
    assert lib.mi355rt_probe_lit_points(rt._h, C.byref(v), None, None, 0, 1, 0, ind.ctypes.data, None) == 0 and (ind == 7.0).all()
    # the handle is what it was: film, direct film, light films, current row, camera, lens
    s, q, n = rt.film.pixel_datas()
    after = (bits(s), bits(q), n, bits(rt.film.direct_sums()), bits(rt.light_films.get()))
    assert all(np.array_equal(x, y) for x, y in zip(film_before, after))
    assert rt.current_row == row and rt.lens.as_dict() == lens
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(cam, rt.camera.matrices()))
    assert rt.hbm_allocated_bytes() == hbm
    # ... and the next samples of the film are the ones it would have taken without the calls
    twin = make(pkg, sc, flags=sem3.gpu | pkg.FLAG_DIRECT_FILM | pkg.FLAG_LIGHT_FILMS)
    twin.set_lens("thin", radius=0.05, focus=4.0)
    twin.render(2); twin.render(1); rt.render(1)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(rt.film.pixel_datas()[:2], twin.film.pixel_datas()[:2]))
    twin.close(); rt.close()


def test_a_device_group_refuses_both_entries(pkg, plit, pr, scenes, handles):
    name = "4boxes"
    vol = volume_of(handles, pr, plit, scenes, name, GRIDS[0], False, False)
    group = make(pkg, plc.scene_of(scenes, name), device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    rays = np.ascontiguousarray(handles(name).lens_rays(1)[:65])
    with pytest.raises(RuntimeError, match="mi355rt_probe_lit_rays: not available on a device group"):
        group.probe_lit_rays(vol, rays)
    with pytest.raises(RuntimeError, match="mi355rt_probe_lit_points: not available on a device group"):
        group.probe_lit_points(vol, np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:]))
    group.close()


# ---- 4. a probe-lit frame ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", ["pinhole", "thin"])
def test_render_probe_lit_is_the_frame_mean_of_the_statement(pkg, plit, pr, scenes, handles, sem, lens):
    import torch
    name = "ico3_tex"
    sc = plc.scene_of(scenes, name)
    vol = volume_of(handles, pr, plit, scenes, name, GRIDS[1], True, True)
    rt = make(pkg, sc, flags=sem.gpu)
    if lens == "thin":
        rt.set_lens("thin", radius=0.05, focus=4.0)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a.view(np.int32).copy() if a.dtype == np.uint32 else a.copy()).to(dev)
    tvol = dict(vol, n=t(vol["n"]), sh=t(vol["sh"]), usable=t(vol["usable"]), offsets=t(vol["offsets"]),
                depth=dict(vol["depth"], count=t(vol["depth"]["count"]), moments=t(vol["depth"]["moments"])))
    for spp in (1, 3):
        rays = rt.lens_rays(spp)
        st = statement(rt, plit, sc, vol, rays)
        got = rt.render_probe_lit(vol, spp=spp)
        assert set(got) == {"mean", "light", "indirect", "ok_share"}
        for k, s in (("mean", "rgb"), ("light", "light"), ("indirect", "indirect")):
            assert got[k].shape == (H, W, 3) and got[k].dtype == np.float32
            assert np.array_equal(bits(got[k]), bits(plit.frame_mean(st[s], W * H).reshape(H, W, 3))), (k, spp)
        assert np.array_equal(bits(got["ok_share"]), bits(plit.frame_mean(st["ok"].astype(F).reshape(-1, 1), W * H).reshape(H, W)))
        assert 0.0 < got["ok_share"].mean() < 1.0
        onto = rt.render_probe_lit(tvol, spp=spp, device=dev)
        for k in got:
            assert isinstance(onto[k], torch.Tensor) and onto[k].device == dev
            assert np.array_equal(bits(onto[k].cpu().numpy()), bits(got[k])), (k, spp)
        assert rt.film.pixel_datas()[2].sum() == 0                                    # no film is touched
    packed = rt.display_image(got["mean"].reshape(-1, 3))                             # to the screen through the existing display mapping
    assert packed.shape == (W * H,) and packed.dtype == np.uint32
    rt.close()
