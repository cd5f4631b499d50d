"""Adaptive sampling on the device (include/mi355rt.h): the tile verdict equals its numpy statement on the film read
back; every round adds exactly batch_spp samples to exactly the owned pixels of the active tiles; the film is bit-exact against the
CPU oracle rendered batch by batch; inactive pixels cost no ray; limits, layouts, errors and the CLI."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ad(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.adaptive")


def make(pkg, scenes, name, w, h, **kw):
    return pkg.create_raytracer_from_arrays(scenes(name), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, **kw)


def full_cfg(**kw):
    c = dict(min_spp=8, max_spp=64, batch_spp=8, max_rounds=0, rel_error=0.05, abs_floor=0.02)
    c.update(kw)
    return c


def replay(ad, rt, cfg, owned=None):
    s, q, n = rt.film.pixel_datas()
    return ad.tile_mask(s, q, n, rt.width, rt.height, owned_rows=owned, **cfg)


def oracle_snapshots(oracle, scenes, name, w, h, seed, flags, batch, max_spp, pre=0):
    """the oracle's film after pre + k * batch samples per pixel, k = 0 .. (max_spp - pre) / batch"""
    orc = oracle.Oracle(scenes(name), w, h, seed=seed, flags=flags)
    if pre:
        orc.render(pre, nthreads=8)
    snaps = {pre: orc.film() + (orc.get_pixels(), orc.get_tonemapped_pixels())}
    k = pre
    while k + batch <= max_spp:
        orc.render(batch, nthreads=8)
        k += batch
        snaps[k] = orc.film() + (orc.get_pixels(), orc.get_tonemapped_pixels())
    return snaps


def assert_matches_snapshots(rt, snaps, rows=None):
    """every pixel (of `rows`) equals the snapshot for its own n: sums, squares, n, get_pixels and the packed pixel"""
    gs, gq, gn = rt.film.pixel_datas()
    gp = rt.film.get_pixels(); gt = rt.get_tonemapped_pixels()
    sel = np.ones(gn.size, bool)
    if rows is not None:
        sel = np.zeros((rt.height, rt.width), bool); sel[np.asarray(rows)] = True; sel = sel.reshape(-1)
    assert set(np.unique(gn[sel]).tolist()) <= set(snaps), (np.unique(gn[sel]), sorted(snaps))
    for k, (os_, oq, on, op, ot) in snaps.items():
        m = sel & (gn == k)
        if not m.any():
            continue
        assert np.array_equal(on[m], gn[m])
        assert np.array_equal(bits(gs[m]), bits(os_[m])), k
        assert np.array_equal(bits(gq[m]), bits(oq[m])), k
        if k:
            assert np.array_equal(bits(gp[m]), bits(op[m])), k
        assert np.array_equal(gt[m], ot[m]), k


# ---- 1. the verdict equals its numpy replay -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("ico2", 48, 40), ("thai2", 64, 48), ("ico3_tex", 100, 37)])
def test_tile_mask_equals_the_numpy_replay(pkg, scenes, ad, name, w, h):
    rt = make(pkg, scenes, name, w, h, seed=3)
    cfgs = [full_cfg(min_spp=2), full_cfg(min_spp=2, rel_error=0.3, abs_floor=0.05), full_cfg(min_spp=4, max_spp=12, batch_spp=3, rel_error=0.0),
            full_cfg(min_spp=2, rel_error=1.5, abs_floor=0.5), full_cfg(min_spp=2, max_spp=7, batch_spp=1)]

    def check():
        for cfg in cfgs:
            got = rt.adaptive_tile_mask(**cfg)
            assert np.array_equal(got, replay(ad, rt, cfg)), cfg
    check()                                           # empty film: n = 0 everywhere
    for k in (2, 3, 1):
        rt.render(k)
        check()
    rt.camera.move_rel(0.1, 0.05, -0.2); rt.camera.add_y_angle(0.05)
    rt.render(2)
    check()
    for _ in range(3):                                # 50-row calls leave a mixed n
        rt.trace_frame_additive()
    check()


# ---- 2. one round at a time ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [8, 3])
def test_rounds_change_exactly_the_predicted_pixels(pkg, scenes, ad, batch):
    name, w, h = "thai2", 64, 48
    rt = make(pkg, scenes, name, w, h, seed=5)
    cfg = full_cfg(min_spp=batch * 2, max_spp=batch * 8, batch_spp=batch, max_rounds=1, rel_error=0.05, abs_floor=0.02)
    tiles = ad.pixel_tiles(w, h).reshape(-1)
    rounds = 0
    while True:
        s0, q0, n0 = rt.film.pixel_datas()
        mask = replay(ad, rt, cfg).reshape(-1)
        st = rt.render_adaptive(**cfg)
        counts = rt.last_counts()
        s1, q1, n1 = rt.film.pixel_datas()
        on = mask[tiles] != 0
        assert st["tiles_active_first"] == int(mask.sum())
        if not mask.any():
            assert st["rounds"] == 0 and st["samples_added"] == 0 and counts.primary == 0
            assert np.array_equal(n0, n1) and np.array_equal(bits(s0), bits(s1))
            break
        assert st["rounds"] == 1
        assert np.array_equal(n1[on], n0[on] + batch)
        assert np.array_equal(n1[~on], n0[~on])
        assert np.array_equal(bits(s1[~on]), bits(s0[~on])) and np.array_equal(bits(q1[~on]), bits(q0[~on]))
        assert st["samples_added"] == counts.primary == int(n1.sum()) - int(n0.sum()) == int(on.sum()) * batch
        rounds += 1
        assert rounds < 20
    assert rounds >= 3


# ---- 3. bit-exact against the oracle rendered batch by batch ----------------------------------------------------------------------
@pytest.mark.parametrize("batch,max_spp", [(8, 24), (3, 12)])
def test_film_bit_exact_vs_oracle_snapshots(pkg, scenes, oracle, sem, batch, max_spp):
    name, w, h = "thai2", 48, 40
    rt = make(pkg, scenes, name, w, h, seed=2, flags=sem.gpu)
    st = rt.render_adaptive(**full_cfg(min_spp=batch, max_spp=max_spp, batch_spp=batch, rel_error=0.05, abs_floor=0.02))
    assert st["rounds"] >= 2 and st["tiles_active_last"] == 0
    _, _, gn = rt.film.pixel_datas()
    assert gn.min() < max_spp and gn.max() == max_spp       # something settled early, something ran to the cap
    assert_matches_snapshots(rt, oracle_snapshots(oracle, scenes, name, w, h, 2, sem.orc, batch, max_spp))


@pytest.mark.parametrize("variant", ["octree_walk", "no_raster", "no_cull_cache"])
def test_film_bit_exact_on_every_primary_path(pkg, scenes, oracle, monkeypatch, variant):
    name, w, h, batch, max_spp = "thai2", 40, 36, 3, 12
    flags = pkg.FLAG_OCTREE_SEMANTICS if variant == "octree_walk" else 0
    if variant == "no_raster":
        monkeypatch.setenv("MI355RT_NO_RASTER", "1")
    if variant == "no_cull_cache":
        monkeypatch.setenv("MI355RT_NO_CULL_CACHE", "1")
    rt = make(pkg, scenes, name, w, h, seed=4, flags=flags)
    st = rt.render_adaptive(**full_cfg(min_spp=3, max_spp=max_spp, batch_spp=batch))
    assert st["rounds"] >= 2
    assert_matches_snapshots(rt, oracle_snapshots(oracle, scenes, name, w, h, 4, 0, batch, max_spp))


# ---- 4. narrow images: every tile is a band of whole rows, so the oracle can render exactly the active bands ---------------------------
@pytest.mark.parametrize("name,batch", [("thai2", 4), ("ico2", 3)])
def test_counters_equal_the_oracle_on_the_active_bands(pkg, scenes, oracle, ad, sem, name, batch):
    w, h = 8, 44                                   # 6 bands, the last one 4 rows
    rt = make(pkg, scenes, name, w, h, seed=6, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=6, flags=sem.orc)
    cfg = full_cfg(min_spp=batch, max_spp=batch * 6, batch_spp=batch, max_rounds=1, rel_error=0.1, abs_floor=0.05)
    rounds = 0
    while True:
        mask = rt.adaptive_tile_mask(**cfg)[:, 0]
        st = rt.render_adaptive(**cfg)
        c = rt.last_counts()
        if not mask.any():
            assert st["rounds"] == 0
            break
        tot = dict(primary=0, bounce=0, shadow=0, primary_hits=0)
        for b in np.flatnonzero(mask):
            oc = orc.render(batch, nthreads=4, rows=(8 * b, min(8 * b + 8, h)))
            for k in tot:
                tot[k] += oc[k]
        assert (c.primary, c.bounce, c.shadow, c.primary_hits) == (tot["primary"], tot["bounce"], tot["shadow"], tot["primary_hits"])
        gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
        assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
        rounds += 1
    assert rounds >= 2


# ---- 5. limits --------------------------------------------------------------------------------------------------------------------
def test_min_equal_max_is_a_uniform_render(pkg, scenes):
    name, w, h, M, batch = "ico2", 40, 32, 12, 4
    a = make(pkg, scenes, name, w, h, seed=8); b = make(pkg, scenes, name, w, h, seed=8)
    st = a.render_adaptive(**full_cfg(min_spp=M, max_spp=M, batch_spp=batch, rel_error=0.0, abs_floor=0.0))
    ca = a.last_counts(); cb = b.render(M)
    assert st["rounds"] == M // batch and st["samples_added"] == w * h * M and st["tiles_active_last"] == 0
    assert (ca.primary, ca.bounce, ca.shadow, ca.primary_hits, ca.primary_culled) == (cb.primary, cb.bounce, cb.shadow, cb.primary_hits, cb.primary_culled)
    for x, y in zip(a.film.pixel_datas(), b.film.pixel_datas()):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))


def test_a_loose_target_stops_at_min_spp(pkg, scenes):
    rt = make(pkg, scenes, "thai2", 48, 40, seed=9)
    st = rt.render_adaptive(**full_cfg(min_spp=8, max_spp=64, batch_spp=4, rel_error=10.0, abs_floor=0.01))
    assert st["rounds"] == 2 and st["tiles_active_last"] == 0
    assert np.all(rt.film.pixel_datas()[2] == 8)


@pytest.mark.parametrize("name", ["thai2", "4boxes"])
def test_background_tiles_stop_early(pkg, scenes, name):
    w, h = 96, 64
    rt = make(pkg, scenes, name, w, h, seed=10)
    st = rt.render_adaptive(**full_cfg())
    n = rt.film.pixel_datas()[2]
    assert st["samples_added"] == int(n.sum()) < 64 * w * h
    assert n.min() == 8 and st["tiles"] == 12 * 8


# ---- 6. layouts ---------------------------------------------------------------------------------------------------------------------
def test_slices_do_not_change_the_film(pkg, scenes):
    cfg = full_cfg(min_spp=3, max_spp=15, batch_spp=3)
    films = []
    for sl in (1, 2):
        rt = make(pkg, scenes, "thai2", 64, 48, seed=11)
        rt.set_slices(sl)
        rt.render_adaptive(**cfg)
        films.append([np.asarray(x).view(np.uint32) for x in rt.film.pixel_datas()])
    for x, y in zip(*films):
        assert np.array_equal(x, y)


def test_striped_handle_adapts_its_own_rows(pkg, scenes, oracle, ad):
    name, w, h, batch, max_spp = "thai2", 48, 40, 4, 16
    rt = make(pkg, scenes, name, w, h, seed=12, stripe_rows=4, stripe_rank=1, stripe_world=2)
    owned = rt.owned_rows()
    cfg = full_cfg(min_spp=4, max_spp=max_spp, batch_spp=batch)
    assert np.array_equal(rt.adaptive_tile_mask(**cfg), replay(ad, rt, cfg, owned))
    st = rt.render_adaptive(**cfg)
    gs, gq, gn = rt.film.pixel_datas()
    other = np.ones(h, bool); other[owned] = False
    assert not gn.reshape(h, w)[other].any() and not gs.reshape(h, w, 3)[other].any()
    assert st["samples_added"] == int(gn.sum()) and st["tiles"] == 6 * 5
    snaps = oracle_snapshots(oracle, scenes, name, w, h, 12, 0, batch, max_spp)
    s_, q_, n_ = (x.reshape(h, w, -1) for x in rt.film.pixel_datas())
    for k, (os_, oq, on, _, _) in snaps.items():
        m = np.zeros((h, w), bool); m[owned] = True; m &= n_[..., 0] == k
        assert np.array_equal(bits(s_[m]), bits(os_.reshape(h, w, 3)[m])) and np.array_equal(bits(q_[m]), bits(oq.reshape(h, w, 3)[m]))


def test_adaptive_continues_the_sample_numbers(pkg, scenes, oracle):
    name, w, h = "ico3_tex", 40, 32
    rt = make(pkg, scenes, name, w, h, seed=13)
    rt.render(8)
    rt.render_adaptive(**full_cfg(min_spp=8, max_spp=32, batch_spp=8))
    assert_matches_snapshots(rt, oracle_snapshots(oracle, scenes, name, w, h, 13, 0, 8, 32, pre=8))


# ---- 7. errors, memory, guards ------------------------------------------------------------------------------------------------------
def test_invalid_configs_are_rejected_and_leave_the_film(pkg, scenes):
    rt = make(pkg, scenes, "ico2", 32, 24, seed=14)
    rt.render(2)
    before = [np.asarray(x).copy() for x in rt.film.pixel_datas()]
    bad = [("min_spp", dict(min_spp=1)), ("max_spp", dict(min_spp=8, max_spp=7)), ("batch_spp", dict(batch_spp=0)),
           ("rel_error", dict(rel_error=-0.1)), ("rel_error", dict(rel_error=float("nan"))), ("rel_error", dict(rel_error=float("inf"))),
           ("abs_floor", dict(abs_floor=-1.0)), ("abs_floor", dict(abs_floor=float("nan")))]
    for field, kw in bad:
        with pytest.raises(RuntimeError, match=field):
            rt.render_adaptive(**full_cfg(**kw))
        with pytest.raises(RuntimeError, match=field):
            rt.adaptive_tile_mask(**full_cfg(**kw))
    for x, y in zip(before, rt.film.pixel_datas()):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))


def test_device_groups_are_rejected(pkg, scenes):
    rt = make(pkg, scenes, "ico2", 32, 24, seed=15, device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    rt.render(2)
    before = rt.film.pixel_datas()[2].copy()
    with pytest.raises(RuntimeError, match="device group"):
        rt.render_adaptive(**full_cfg())
    with pytest.raises(RuntimeError, match="device group"):
        rt.adaptive_tile_mask(**full_cfg())
    assert np.array_equal(before, rt.film.pixel_datas()[2])


def test_memory_is_the_tile_buffers_and_guards_stay_clean(pkg, scenes, monkeypatch):
    monkeypatch.setenv("MI355RT_DEBUG_GUARD", "1")
    w, h = 100, 37
    rt = make(pkg, scenes, "thai2", w, h, seed=16)
    rt.render(8)
    hbm0 = rt.hbm_allocated_bytes()
    rt.render_adaptive(**full_cfg(min_spp=8, max_spp=40, batch_spp=8))
    assert rt.hbm_allocated_bytes() - hbm0 == 13 * 5 + 8
    rt.render_adaptive(**full_cfg(min_spp=8, max_spp=64, batch_spp=3))
    assert rt.debug_check_guards() == 0


# ---- 8. the CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_adaptive_writes_the_library_frame(pkg, scenes, tmp_path):
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    w, h = 48, 40
    out = tmp_path / "a.ppm"
    r = subprocess.run([exe, "-f", os.path.join(SCENES, "thai2.scene"), "--width", str(w), "--height", str(h), "--seed", "17",
                        "--adaptive", "0.1", "--abs-floor", "0.03", "--min-spp", "4", "--max-spp", "24", "--batch", "4", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "adaptive:" in r.stdout
    data = out.read_bytes()
    hdr = ("P6\n%d %d\n255\n" % (w, h)).encode()
    assert data.startswith(hdr)
    rgb = np.frombuffer(data[len(hdr):], np.uint8).reshape(-1, 3)
    rt = make(pkg, scenes, "thai2", w, h, seed=17)
    rt.render_adaptive(**full_cfg(min_spp=4, max_spp=24, batch_spp=4, rel_error=0.1, abs_floor=0.03))
    px = rt.get_tonemapped_pixels()
    want = np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8)
    assert np.array_equal(rgb, want)
