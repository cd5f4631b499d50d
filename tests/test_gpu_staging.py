"""The caller's memory around the kernels (csrc/staging.hpp): every entry that takes host memory gives its temporaries back, what a kernel
leaves unwritten survives the round trip through them as it survives a call on device memory, empty and absent arguments write nothing, and the size of a
pass (MI355RT_PASS_SAMPLES) changes no result of any path that cuts its work into passes.  Comparisons are on the bits; the scenes are 16 x 16."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bake_charts

pytestmark = pytest.mark.gpu

W = H = 16
NPIX = W * H
SEED = 5
MISS = 0xFFFFFFFF
E_OK = 0
F = np.float32
SENTINEL = 0x7FC12345           # a quiet NaN with a payload: no arithmetic makes it, and a copy keeps it
AW, AH = 9, 7                   # an atlas that is no multiple of any tile


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sentinels(shape):
    return np.full(shape, SENTINEL, np.uint32).view(F)


@pytest.fixture(scope="module")
def cams(pkg):
    return importlib.import_module("raytracer_rs_amd.cameras")


@pytest.fixture(scope="module")
def bake(pkg):
    return importlib.import_module("raytracer_rs_amd.bake")


@pytest.fixture(scope="module")
def torch():
    import torch as t             # device memory is a torch tensor on the handle's GPU, as everywhere in the suite
    return t


def make(pkg, scenes, name, **kw):
    kw.setdefault("seed", SEED)
    return pkg.create_raytracer_from_arrays(scenes(name), pkg.DEFAULT_TRIANGLES_PER_LEAF, W, H, **kw)


def camera_rays(cams, rt, spp=1):
    return np.ascontiguousarray(cams.pinhole(rt.camera.matrices(), W, H, spp, SEED))


def surface_points(rt, rays, count):
    """`count` hit points of the rays, with the unit vector back along the ray as the normal, and ids with a repeat"""
    tuv, prim = rt.intersect_rays(rays)
    hit = np.nonzero(prim != MISS)[0][:count]
    assert hit.size == count
    o, d = rays[hit, :3].astype(np.float64), rays[hit, 3:].astype(np.float64)
    pts = (o + tuv[hit, :1] * d).astype(F)
    nrm = (-d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    ids = (np.arange(count, dtype=np.uint32) * 2654435761).astype(np.uint32)
    ids[1] = ids[0]
    return np.ascontiguousarray(pts), np.ascontiguousarray(nrm), ids


def half_covered_charts(ntri):
    """one chart over the upper left half of the atlas: texels on both sides of its edge"""
    return bake_charts._pad([[[0.05, 0.05], [0.95, 0.05], [0.05, 0.95]]], ntri)


def on_device(torch, a):
    """the array's bytes in device memory (uint32 as int32 bits)"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).cuda()
    torch.cuda.synchronize()
    return t


def back(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


# ---- 1. every host-staged entry gives its temporaries back --------------------------------------------------------------------------------------------
def test_host_entries_give_their_temporaries_back(pkg, cams, scenes, monkeypatch):
    monkeypatch.setenv("MI355RT_DEBUG_GUARD", "1")
    rt = make(pkg, scenes, "4boxes", flags=pkg.FLAG_DIRECT_FILM | pkg.FLAG_LIGHT_FILMS)
    rays = camera_rays(cams, rt)
    pts, nrm, ids = surface_points(rt, rays, 40)
    rng = np.random.default_rng(3)
    planes = dict(sum=rng.uniform(0, 2, (NPIX, 3)).astype(F), sumsq=rng.uniform(0, 4, (NPIX, 3)).astype(F), n=rng.integers(1, 9, NPIX).astype(np.uint32),
                  direct=rng.uniform(0, 1, (NPIX, 3)).astype(F))
    lights = rng.uniform(0, 1, (rt.nlights, NPIX, 3)).astype(F)
    assert rt.nlights >= 1
    uv = half_covered_charts(int(rt.triangle_count))
    texel_ids = np.array([0, 5, AW * AH - 1], np.uint32)
    a, b = rng.uniform(1, 2, 70).astype(F), rng.uniform(1, 2, 70).astype(F)
    entries = [
        ("intersect_rays", lambda: rt.intersect_rays(rays)),
        ("occluded_rays", lambda: rt.occluded_rays(rays)),
        ("trace_rays", lambda: rt.trace_rays(rays, want=("rgb", "direct", "tuv", "prim"))),
        ("render_rays", lambda: rt.render_rays(rays, 1)),
        ("lens_rays", lambda: rt.lens_rays(1)),
        ("features.render_rays", lambda: rt.features.render_rays(rays, 1)),
        ("features.alpha", lambda: rt.features.alpha()),
        ("film.set", lambda: rt.film.set(**planes)),
        ("film.add", lambda: rt.film.add(**planes)),
        ("film.get_pixels", lambda: rt.film.get_pixels()),
        ("film.get_estimated_variances", lambda: rt.film.get_estimated_variances()),
        ("light_films.set", lambda: rt.light_films.set(lights)),
        ("display_image", lambda: rt.display_image(planes["sum"])),
        ("gather", lambda: rt.gather(pts, nrm, ids, spp=3, want=("n", "hits", "near", "sum", "sumsq", "direct"))),
        ("bake_texels", lambda: rt.bake_texels(uv, AW, AH)),
        ("bake_atlas", lambda: rt.bake_atlas(texel_ids, planes["sum"][:3], AW, AH)),
        ("debug_numerics", lambda: rt.debug_numerics(a, b)),
        ("debug_slab", lambda: rt.debug_slab(rays[:70], np.tile(np.array([-1, -1, -1, 1, 1, 1], F), (70, 1)))),
    ]
    for name, call in entries:
        call()                                  # may grow buffers the handle keeps
        held = rt.hbm_allocated_bytes()
        call()
        assert rt.hbm_allocated_bytes() == held, name
    assert rt.debug_check_guards() == 0
    rt.close()


# ---- 2. what a kernel leaves unwritten survives the host path as it survives the device path ----------------------------------------------------------
def test_trace_rays_keeps_the_tuv_of_a_miss(pkg, cams, scenes, torch):
    rt = make(pkg, scenes, "ico2")
    n = 70                                      # one full wave and a tail
    rays = camera_rays(cams, rt)[93:93 + n].copy()
    rays[::3, 3:] *= -1.0                       # every third ray points away from the scene
    L = pkg.lib()

    def trace(where, rays_addr, tuv_addr, prim_addr):
        o = pkg.RayOutputs()
        o.tuv, o.prim = tuv_addr, prim_addr
        assert L.mi355rt_trace_rays(rt._h, rays_addr, None, n, where, C.byref(o)) == E_OK

    h_tuv, h_prim = sentinels((n, 3)), np.zeros(n, np.uint32)
    trace(pkg.RAYS_HOST, rays.ctypes.data, h_tuv.ctypes.data, h_prim.ctypes.data)
    d_rays, d_tuv, d_prim = on_device(torch, rays), on_device(torch, sentinels((n, 3))), on_device(torch, np.zeros(n, np.uint32))
    trace(pkg.RAYS_DEVICE, d_rays.data_ptr(), d_tuv.data_ptr(), d_prim.data_ptr())
    miss = h_prim == MISS
    assert miss[::3].all() and miss.sum() >= n // 3 and (~miss).sum() >= 10, (int(miss.sum()), n)
    assert np.array_equal(h_prim, back(d_prim))
    assert (bits(h_tuv)[miss] == SENTINEL).all()
    assert np.array_equal(bits(h_tuv), bits(back(d_tuv)))
    assert not (bits(h_tuv)[~miss] == SENTINEL).any()
    rt.close()


def test_bake_texels_keeps_the_bary_of_an_uncovered_texel(pkg, scenes, torch):
    rt = make(pkg, scenes, "4boxes")
    uv = half_covered_charts(int(rt.triangle_count))
    nt = AW * AH
    L = pkg.lib()

    def texels(where, uv_addr, owner_addr, bary_addr):
        o, n = pkg.BakeTexelOutputs(), C.c_uint32(0)
        o.owner, o.bary = owner_addr, bary_addr
        assert L.mi355rt_bake_texels(rt._h, uv_addr, AW, AH, 0, where, C.byref(o), C.byref(n)) == E_OK
        return n.value

    h_owner, h_bary = np.zeros(nt, np.uint32), sentinels((nt, 2))
    n_host = texels(pkg.RAYS_HOST, uv.ctypes.data, h_owner.ctypes.data, h_bary.ctypes.data)
    d_uv, d_owner, d_bary = on_device(torch, uv), on_device(torch, np.zeros(nt, np.uint32)), on_device(torch, sentinels((nt, 2)))
    n_dev = texels(pkg.RAYS_DEVICE, d_uv.data_ptr(), d_owner.data_ptr(), d_bary.data_ptr())
    covered = h_owner != MISS
    assert n_host == n_dev == int(covered.sum()) and 10 <= n_host <= nt - 10
    assert np.array_equal(h_owner, back(d_owner))
    assert (bits(h_bary)[~covered] == SENTINEL).all()
    assert np.array_equal(bits(h_bary), bits(back(d_bary)))
    assert not (bits(h_bary)[covered] == SENTINEL).any()
    rt.close()


def test_gather_accumulates_alike_in_host_and_device_memory(pkg, cams, scenes, torch):
    rt = make(pkg, scenes, "4boxes")
    pts, nrm, ids = surface_points(rt, camera_rays(cams, rt), 40)
    sampled = ("n", "hits", "near", "sum", "sumsq")
    zeros = lambda w: np.zeros((40, 3), F) if w in ("sum", "sumsq") else np.zeros(40, np.uint32)
    host = {w: zeros(w) for w in sampled}
    dev = {w: on_device(torch, zeros(w)) for w in sampled}
    d_pts, d_nrm, d_ids = on_device(torch, pts), on_device(torch, nrm), on_device(torch, ids)
    for first in (0, 3):                        # two calls of 3 samples, both adding to what the arrays hold
        rt.gather(pts, nrm, ids, spp=3, first_sample=first, want=sampled, into=host)
        rt.gather(d_pts, d_nrm, d_ids, spp=3, first_sample=first, want=sampled, into=dev)
    torch.cuda.synchronize()
    assert (host["n"] == 6).all() and host["hits"].any() and bits(host["sum"]).any()
    for w in sampled:
        assert np.array_equal(bits(host[w]), bits(back(dev[w]))), w
    rt.close()


# ---- 3. empty and absent arguments --------------------------------------------------------------------------------------------------------------------
def test_empty_and_absent_arguments_write_nothing(pkg, cams, bake, scenes, torch):
    rt = make(pkg, scenes, "4boxes")
    L = pkg.lib()
    rays = camera_rays(cams, rt)
    held = rt.hbm_allocated_bytes()

    # mi355rt_trace_rays, n == 0: "succeeds and writes nothing", with or without a rays pointer
    outs = {w: sentinels((4, 3)) for w in ("rgb", "direct", "tuv")}
    outs["prim"] = np.full(4, SENTINEL, np.uint32)
    o = pkg.RayOutputs()
    for w, a in outs.items():
        setattr(o, w, a.ctypes.data)
    assert L.mi355rt_trace_rays(rt._h, None, None, 0, pkg.RAYS_HOST, C.byref(o)) == E_OK
    assert L.mi355rt_trace_rays(rt._h, rays.ctypes.data, None, 0, pkg.RAYS_HOST, C.byref(o)) == E_OK
    assert all((bits(a) == SENTINEL).all() for a in outs.values())

    # mi355rt_intersect_rays / mi355rt_occluded_rays, n == 0
    tuv, prim, blocked = sentinels((4, 3)), np.full(4, SENTINEL, np.uint32), np.full(4, 0xA5, np.uint8)
    assert L.mi355rt_intersect_rays(rt._h, None, 0, pkg._fp(tuv), pkg._up(prim)) == E_OK
    assert L.mi355rt_occluded_rays(rt._h, None, 0, blocked.ctypes.data_as(C.POINTER(C.c_uint8))) == E_OK
    assert (bits(tuv) == SENTINEL).all() and (prim == SENTINEL).all() and (blocked == 0xA5).all()

    # mi355rt_bake_atlas, n == 0: every texel empty (zeros, valid 0), exactly width * height of them, in host and in device memory
    nt = AW * AH
    want_atlas, want_valid = bake.atlas(np.zeros(0, np.uint32), np.zeros((0, 3), F), AW, AH, 2)
    atlas, valid = sentinels((nt + 2, 3)), np.full(nt + 2, 0xA5, np.uint8)
    assert L.mi355rt_bake_atlas(rt._h, None, None, 0, AW, AH, 2, pkg.RAYS_HOST, atlas.ctypes.data, valid.ctypes.data) == E_OK
    assert np.array_equal(bits(atlas[:nt]), bits(want_atlas)) and np.array_equal(valid[:nt], want_valid)
    assert (bits(atlas[nt:]) == SENTINEL).all() and (valid[nt:] == 0xA5).all()
    d_atlas, d_valid = on_device(torch, sentinels((nt + 2, 3))), on_device(torch, np.full(nt + 2, 0xA5, np.uint8))
    assert L.mi355rt_bake_atlas(rt._h, None, None, 0, AW, AH, 2, pkg.RAYS_DEVICE, d_atlas.data_ptr(), d_valid.data_ptr()) == E_OK
    assert np.array_equal(bits(back(d_atlas)), bits(atlas)) and np.array_equal(back(d_valid), valid)

    # mi355rt_gather asking only for `direct`: exactly npoints x 3 floats, the ones a call on device memory writes
    pts, nrm, ids = surface_points(rt, rays, 40)
    direct = sentinels((42, 3))
    g = pkg.GatherOutputs()
    g.direct = direct.ctypes.data
    cfg = pkg.GatherConfig()
    L.mi355rt_gather_default_config(C.byref(cfg))
    assert L.mi355rt_gather(rt._h, pts.ctypes.data, nrm.ctypes.data, ids.ctypes.data, 40, C.byref(cfg), pkg.RAYS_HOST, C.byref(g)) == E_OK
    on_dev = rt.gather(on_device(torch, pts), on_device(torch, nrm), on_device(torch, ids), want=("direct",))["direct"]
    assert np.array_equal(bits(direct[:40]), bits(back(on_dev))) and bits(direct[:40]).any()
    assert (bits(direct[40:]) == SENTINEL).all()

    # mi355rt_bake_texels asking only for ncovered: out may be NULL
    uv = half_covered_charts(int(rt.triangle_count))
    n = C.c_uint32(SENTINEL)
    assert L.mi355rt_bake_texels(rt._h, uv.ctypes.data, AW, AH, 0, pkg.RAYS_HOST, None, C.byref(n)) == E_OK
    assert n.value == rt.bake_texels(uv, AW, AH, want=("owner",))["ncovered"] and 0 < n.value < nt

    assert rt.hbm_allocated_bytes() == held
    rt.close()


# ---- 4. the pass budget is one rule ---------------------------------------------------------------------------------------------------------------------
def test_pass_samples_changes_no_result(pkg, cams, scenes, monkeypatch):
    def everything(rt):
        rays = camera_rays(cams, rt, 10)[:2500]
        pts, nrm, ids = surface_points(rt, rays, 40)
        out = dict(trace=rt.trace_rays(rays, want=("rgb", "direct", "tuv", "prim")))
        out["trace_launches"] = rt.last_counts().trace_launches
        out["gather"] = rt.gather(pts, nrm, ids, spp=64, want=("n", "hits", "near", "sum", "sumsq", "direct"))
        out["gather_launches"] = rt.last_counts().trace_launches
        out["render_launches"] = rt.render(8).trace_launches
        out["film"] = dict(zip(("sum", "sumsq", "n"), rt.film.pixel_datas()))
        return out

    monkeypatch.setenv("MI355RT_PASS_SAMPLES", "1024")
    small = make(pkg, scenes, "4boxes")
    a = everything(small)
    small.close()
    monkeypatch.delenv("MI355RT_PASS_SAMPLES")
    whole = make(pkg, scenes, "4boxes")
    b = everything(whole)
    whole.close()
    for call in ("trace", "gather", "render"):                  # 2500 rays, 40 x 64 rays and 256 x 8 samples in passes of 1024: several, against one
        assert a[call + "_launches"] > b[call + "_launches"], call
    for call in ("trace", "gather", "film"):
        assert a[call].keys() == b[call].keys()
        for w in a[call]:
            assert np.array_equal(bits(a[call][w]), bits(b[call][w])), (call, w)
    assert bits(b["trace"]["rgb"]).any() and bits(b["gather"]["sum"]).any() and bits(b["film"]["sum"]).any()
