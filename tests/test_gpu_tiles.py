"""mi355rt_render_tiles and refine on the device (include/mi355rt.h, "RENDER TILES"): samples into the tiles of a caller's mask under the
pinhole, THIN and ORTHO, and the adaptive loop built on it.

No yardstick is the code under test: the CPU oracle (pinhole), a second handle that renders uniformly under the same lens (held to cameras.py and the oracle by
tests/test_gpu_lens.py), a striped handle whose rows are the mask's tile rows, mi355rt_render_adaptive on a twin handle, and adaptive.tile_mask in numpy.  Every
comparison is on the bits.  Shapes: 37 x 21 (tiles clipped at both edges; 256-sample chunks straddle tiles at 3 spp), 8 x 40 (a tile is a band of whole rows),
64 x 48 (a one-tile mask leaves most chunks wholly inactive)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_display import read_png

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
EXE = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
W, H, SEED = 37, 21, 5
T = 8
E_INVALID = -1
THIN = dict(model="thin", radius=0.1, focus=5.0)
ORTHO = dict(model="ortho", width_world=9.5)
PINHOLE = dict(model="pinhole")
LENSES = {"pinhole": PINHOLE, "thin": THIN, "ortho": ORTHO}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ad(pkg):
    return importlib.import_module("raytracer_rs_amd.adaptive")


def make(pkg, scenes, name, w=W, h=H, **kw):
    kw.setdefault("seed", SEED)
    rt = pkg.create_raytracer_from_arrays(scenes(name), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, **kw)
    rt._direct = bool(kw.get("flags", 0) & pkg.FLAG_DIRECT_FILM)
    return rt


@pytest.fixture(scope="module")
def handles(pkg, scenes):
    """handles shared by the tests of this module, keyed by (scene, tag, size, config); every test clears the film and sets the lens it needs"""
    made = {}

    def get(name, tag="a", w=W, h=H, **kw):
        key = (name, tag, w, h, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = make(pkg, scenes, name, w, h, **kw)
        rt = made[key]
        rt.set_lens("pinhole")
        rt.film.clear()
        return rt
    yield get
    for rt in made.values():
        rt.close()


def film_of(rt):
    """(sum bits, sumsq bits, n[, direct bits]) as [npix, ...] arrays"""
    s, q, n = rt.film.pixel_datas()
    out = (bits(s).reshape(-1, 3).copy(), bits(q).reshape(-1, 3).copy(), np.asarray(n).reshape(-1).copy())
    if rt._direct:
        out += (bits(rt.film.direct_sums()).reshape(-1, 3).copy(),)
    return out


def same_film(a, b, sel=None):
    return len(a) == len(b) and all(np.array_equal(x if sel is None else x[sel], y if sel is None else y[sel]) for x, y in zip(a, b))


def tiles_of(w, h):
    return (w + T - 1) // T, (h + T - 1) // T


def pixels_of(mask, w, h):
    """bool[npix]: the pixel lies in a selected tile"""
    y, x = np.mgrid[0:h, 0:w]
    return (np.asarray(mask).reshape(tiles_of(w, h)[::-1])[y // T, x // T] != 0).reshape(-1)


def checkerboard(w, h, phase=0):
    tx, ty = tiles_of(w, h)
    y, x = np.mgrid[0:ty, 0:tx]
    return ((x + y + phase) % 2 == 0).astype(np.uint8)


def tile_rows(w, h, r):
    tx, ty = tiles_of(w, h)
    m = np.zeros((ty, tx), np.uint8)
    m[r::2] = 1
    return m


COUNTERS = ("primary", "primary_hits", "bounce", "shadow", "bounce_skipped", "shadow_skipped")


def counters(c, names=COUNTERS):
    return tuple(int(getattr(c, k)) for k in names)


def oracle_snapshots(oracle, scene, w, h, seed, flags, counts):
    """the oracle's film (sums, squares, n, get_pixels, packed) after each of the sample counts in `counts` (ascending)"""
    orc = oracle.Oracle(scene, w, h, seed=seed, flags=flags)
    snaps, k = {}, 0
    for c in counts:
        if c > k:
            orc.render(c - k, nthreads=8)
            k = c
        snaps[c] = orc.film() + (orc.get_pixels(), orc.get_tonemapped_pixels())
    return snaps


def assert_matches_snapshots(rt, snaps, want_n):
    """every pixel equals the snapshot for its own n — which is want_n: sums, squares, n, get_pixels and the packed pixel"""
    gs, gq, gn = rt.film.pixel_datas()
    gp = rt.film.get_pixels(); gt = rt.get_tonemapped_pixels()
    assert np.array_equal(gn, want_n)
    for k, (os_, oq, on, op, ot) in snaps.items():
        m = gn == k
        assert np.array_equal(on[m], gn[m])
        assert np.array_equal(bits(gs)[m], bits(os_)[m]), k
        assert np.array_equal(bits(gq)[m], bits(oq)[m]), k
        if k:
            assert np.array_equal(bits(gp)[m], bits(op)[m]), k
        assert np.array_equal(gt[m], ot[m]), k


# ---- 1. the pinhole against the oracle -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ico2", "thai2"])
def test_pinhole_tiles_equal_the_oracle_per_pixel(pkg, scenes, oracle, handles, sem3, name):
    rt = handles(name, flags=sem3.gpu)
    rt.render(2)
    rt.get_tonemapped_pixels()                                          # every row is clean now: the packed pixels below are right only if render_tiles marks its rows changed
    mask = checkerboard(W, H)
    c = rt.render_tiles(mask, 3)
    on = pixels_of(mask, W, H)
    assert 0 < on.sum() < W * H and c.primary == 3 * int(on.sum())
    snaps = oracle_snapshots(oracle, scenes(name), W, H, SEED, sem3.orc, (2, 5))
    assert_matches_snapshots(rt, snaps, np.where(on, 5, 2).astype(np.uint32))


@pytest.mark.parametrize("name", ["ico2", "thai2"])
def test_pinhole_bands_equal_the_oracle_film_and_counters(pkg, scenes, oracle, handles, sem3, name):
    w, h = 8, 40                                   # 5 bands of 8 whole rows
    rt = handles(name, w=w, h=h, flags=sem3.gpu)
    mask = tile_rows(w, h, 0)
    c = rt.render_tiles(mask, 3)
    orc = oracle.Oracle(scenes(name), w, h, seed=SEED, flags=sem3.orc)
    tot = dict(primary=0, bounce=0, shadow=0, primary_hits=0)
    for b in np.flatnonzero(mask[:, 0]):
        oc = orc.render(3, nthreads=4, rows=(8 * b, 8 * b + 8))
        for k in tot:
            tot[k] += oc[k]
    assert counters(c, ("primary", "bounce", "shadow", "primary_hits")) == (tot["primary"], tot["bounce"], tot["shadow"], tot["primary_hits"])
    assert c.primary == 3 * 24 * w and c.primary_hits > 0
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))


# ---- 2. a lens against the uniform render under the same lens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["thai2", "ico2", "ico3_tex"])
@pytest.mark.parametrize("model", ["thin", "ortho"])
def test_lens_tiles_equal_the_uniform_lens_render_per_pixel(pkg, scenes, handles, sem3, model, name):
    flags = sem3.gpu | pkg.FLAG_DIRECT_FILM
    a, b = handles(name, flags=flags), handles(name, tag="uniform", flags=flags)
    for rt in (a, b):
        rt.set_lens(**LENSES[model])
        rt.render(2)
    snap2 = film_of(b)
    before = film_of(a)
    assert same_film(before, snap2)
    packed2 = a.get_tonemapped_pixels().copy()                          # every row of `a` is clean now
    assert np.array_equal(packed2, b.get_tonemapped_pixels())
    b.render(3)
    snap5 = film_of(b)
    packed5 = b.get_tonemapped_pixels()
    mask = checkerboard(W, H, 1)
    on = pixels_of(mask, W, H)
    c = a.render_tiles(mask, 3)
    got = film_of(a)
    assert len(got) == 4                                               # sums, squares, n and the direct film
    assert np.array_equal(got[2], np.where(on, 5, 2))
    assert same_film(got, snap5, on)                                    # selected pixels: the uniform render of 5 samples
    assert same_film(got, before, ~on)                                  # the others: bit-identical to before the call
    assert np.array_equal(a.get_tonemapped_pixels(), np.where(on, packed5, packed2))       # the touched rows were marked changed
    assert not np.array_equal(packed5[on], packed2[on])
    assert c.primary == 3 * int(on.sum()) and c.primary_culled == 0 and 0 < c.primary_hits < c.primary
    assert not same_film(snap2, snap5, on)


# ---- 3. counters under a lens against a striped handle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(W, H), (64, 48)])
@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("model", ["thin", "ortho"])
def test_lens_counters_equal_a_striped_handle(pkg, scenes, handles, model, r, w, h):
    flags = pkg.FLAG_COUNT_STEPS
    a = handles("thai2", w=w, h=h, flags=flags)
    st = handles("thai2", tag="stripe%d" % r, w=w, h=h, flags=flags, stripe_rows=8, stripe_world=2, stripe_rank=r)
    for rt in (a, st):
        rt.set_lens(**LENSES[model])
    mask = tile_rows(w, h, r)
    on = pixels_of(mask, w, h)
    owned = np.zeros(h, bool); owned[st.owned_rows()] = True
    assert np.array_equal(np.repeat(owned, w), on)
    cs = st.render(3)
    ca = a.render_tiles(mask, 3)
    read = a.debug_rays_read()
    assert same_film(film_of(a), film_of(st))                           # the owned rows, and zero elsewhere on both
    assert counters(ca) == counters(cs) and ca.primary == 3 * int(on.sum())
    assert ca.primary_culled == 0 and ca.primary_hits > 0 and ca.bounce > 0 and ca.shadow > 0
    # no ray was made for an inactive pixel: the trace launches took exactly the rays of the selected pixels from their queues
    assert read == ca.primary + (ca.bounce - ca.bounce_skipped) + (ca.shadow - ca.shadow_skipped), (read, ca.as_dict())


# ---- 4. degenerate masks ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["pinhole", "thin", "ortho"])
def test_full_and_empty_masks(pkg, scenes, handles, model):
    flags = pkg.FLAG_DIRECT_FILM
    a, b = handles("thai2", flags=flags), handles("thai2", tag="uniform", flags=flags)
    for rt in (a, b):
        rt.set_lens(**LENSES[model])
        rt.render(2)
    tx, ty = tiles_of(W, H)
    # all zero: nothing changes, nothing is counted
    before, row = film_of(a), a.current_row
    c0 = a.render_tiles(np.zeros((ty, tx), np.uint8), 3)
    assert same_film(film_of(a), before) and a.current_row == row
    assert counters(c0) == (0,) * 6 and c0.primary_culled == 0
    # full (flat, and values other than 1): the film and the counters of render(spp)
    cb = b.render(3)
    ca = a.render_tiles(np.full(ty * tx, 7, np.uint8), 3)
    assert same_film(film_of(a), film_of(b))
    assert counters(ca) == counters(cb) and ca.primary == 3 * W * H
    assert ca.primary_culled == cb.primary_culled
    if model != "pinhole":
        assert ca.primary_culled == 0


@pytest.mark.parametrize("model", ["pinhole", "thin", "ortho"])
def test_one_tile_mask_leaves_the_rest_alone(pkg, scenes, handles, model):
    w, h = 64, 48
    flags = pkg.FLAG_DIRECT_FILM
    a, b = handles("thai2", w=w, h=h, flags=flags), handles("thai2", tag="uniform", w=w, h=h, flags=flags)
    for rt in (a, b):
        rt.set_lens(**LENSES[model])
        rt.render(2)
    before = film_of(a)
    b.render(3)
    mask = np.zeros(tiles_of(w, h)[::-1], np.uint8)
    mask[3, 4] = 1                                                       # a tile on the statue
    on = pixels_of(mask, w, h)
    assert on.sum() == 64
    c = a.render_tiles(mask, 3)
    got = film_of(a)
    assert same_film(got, film_of(b), on) and same_film(got, before, ~on)
    assert c.primary == 3 * 64 and c.primary_hits > 0


# ---- 5. batching and layout do not matter ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["pinhole", "thin"])
def test_batching_and_layout_do_not_matter(pkg, scenes, handles, monkeypatch, model):
    lens = LENSES[model]
    mask = checkerboard(W, H)
    on = pixels_of(mask, W, H)

    def run(rt, close=True, m=mask):
        rt.set_lens(**lens)
        rt.render(2)
        rt.render_tiles(m, 3)
        f = film_of(rt)
        if close:
            rt.close()
        return f
    want = run(handles("thai2"), close=False)
    assert np.array_equal(want[2], np.where(on, 5, 2))
    # one sample per pass
    assert same_film(run(make(pkg, scenes, "thai2", samples_per_pass=1)), want)
    # small passes at 64 x 48: 1024 samples are 16 rows of one sample, so every sample takes three row blocks and a tile row of the mask is split between passes
    w2, h2 = 64, 48
    mask2 = checkerboard(w2, h2)
    want2 = run(handles("thai2", w=w2, h=h2), close=False, m=mask2)
    assert np.array_equal(want2[2], np.where(pixels_of(mask2, w2, h2), 5, 2))
    monkeypatch.setenv("MI355RT_PASS_SAMPLES", "1024")
    assert same_film(run(make(pkg, scenes, "thai2", w2, h2), m=mask2), want2)
    monkeypatch.delenv("MI355RT_PASS_SAMPLES")
    # stripes whose height is no multiple of the tile: each rank writes its rows of the selected tiles, together they give the film
    parts = []
    for rank in (0, 1):
        st = make(pkg, scenes, "thai2", stripe_rows=3, stripe_world=2, stripe_rank=rank)
        owned = np.zeros(H, bool); owned[st.owned_rows()] = True
        f = run(st)
        sel = np.repeat(owned, W)
        assert same_film(f, want, sel) and not any(x[~sel].any() for x in f)
        parts.append(sel)
    assert np.array_equal(parts[0], ~parts[1])
    # right after a queued frame
    rt = handles("thai2")
    rt.set_lens(**lens)
    assert rt.render(2, wait=False) is None
    c = rt.render_tiles(mask, 3)
    assert same_film(film_of(rt), want) and c.primary == 3 * int(on.sum())


def test_tiles_in_the_middle_of_a_drop_in_loop(pkg, scenes, handles):
    """pinhole: 50-row calls (one of them speculative) around a render_tiles call give what the same calls give with render_tiles moved to the end"""
    w, h = 64, 120
    a, b = handles("thai2", w=w, h=h), handles("thai2", tag="uniform", w=w, h=h)
    mask = checkerboard(w, h)
    a.trace_frame_additive(); a.trace_frame_additive()
    row = a.current_row
    a.render_tiles(mask, 3)
    assert a.current_row == row
    a.trace_frame_additive()
    # the yardstick: three 50-row calls, then uniform frames from which every pixel takes the snapshot of its own count
    for _ in range(3):
        b.trace_frame_additive()
    assert a.current_row == b.current_row
    base = film_of(b)
    b.render(3)
    plus3 = film_of(b)
    on = pixels_of(mask, w, h)
    got = film_of(a)
    # (rows 100..119 and 0..29 were traced once more by the third call AFTER the tiles; a sample is a function of (pixel, sample number, seed) and the film adds
    # them in number order, so it does not matter which call made which)
    assert np.array_equal(got[2], base[2] + np.where(on, 3, 0))
    assert same_film(got, base, ~on)
    assert same_film(got, plus3, on)


# ---- 6. host and device masks ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["pinhole", "thin"])
def test_device_mask_gives_the_host_mask_film(pkg, scenes, handles, model):
    import torch
    a, b = make(pkg, scenes, "ico2"), handles("ico2", tag="uniform")     # a: a fresh handle, which has no mask buffer yet
    for rt in (a, b):
        rt.set_lens(**LENSES[model])
        rt.render(3)                                                     # (as many samples as the call below adds: the pass buffers do not grow again)
    mask = checkerboard(W, H)
    tx, ty = tiles_of(W, H)
    hbm0 = a.hbm_allocated_bytes()
    ca = a.render_tiles(mask, 3)
    assert a.hbm_allocated_bytes() - hbm0 == tx * ty                     # the handle-owned copy of a host mask, allocated on first use
    buf = torch.full((tx * ty + 64,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", 0))
    buf[:tx * ty] = torch.from_numpy(mask.reshape(-1)).to(buf.device)
    torch.cuda.synchronize()
    hbm1 = b.hbm_allocated_bytes()
    cb = b.render_tiles(buf[:tx * ty].view(ty, tx), 3)
    assert b.hbm_allocated_bytes() == hbm1                                # read in place
    assert same_film(film_of(a), film_of(b)) and counters(ca) == counters(cb)
    back = buf.cpu().numpy()
    assert np.array_equal(back[:tx * ty], mask.reshape(-1)) and (back[tx * ty:] == 0xA5).all()
    with pytest.raises(ValueError, match="shape"):
        b.render_tiles(buf[:tx * ty - 1], 3)
    with pytest.raises(TypeError, match="uint8"):
        b.render_tiles(mask.astype(np.int32), 3)
    a.close()


# ---- 7. refine ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [8, 3])
def test_refine_is_render_adaptive_under_the_pinhole(pkg, scenes, handles, batch):
    """thai2 64 x 48, seed 21, rel_error 0.3: the CPU oracle replayed with adaptive.tile_mask gives 6 rounds and the sample counts 8 16 24 40 48 (batch 8) and
    6 9 18 (batch 3) among the pixels with hits"""
    w, h = 64, 48
    cfg = dict(min_spp=batch, max_spp=6 * batch, batch_spp=batch, max_rounds=0, rel_error=0.3, abs_floor=0.02)
    a, b = handles("thai2", w=w, h=h, seed=21), handles("thai2", tag="twin", w=w, h=h, seed=21)
    want = b.render_adaptive(**cfg)
    cb = b.last_counts()
    got = a.refine(**cfg)
    assert same_film(film_of(a), film_of(b))
    assert {k: got[k] for k in want} == want
    assert (got["primary"], got["bounce"], got["shadow"], got["primary_hits"]) == counters(cb, ("primary", "bounce", "shadow", "primary_hits"))
    s, _, n = film_of(a)
    assert got["rounds"] >= 2 and len(np.unique(n[s.any(axis=1)])) >= 2


def test_refine_under_a_thin_lens(pkg, scenes, handles, ad):
    """adaptive depth of field.  Observed on the device (thai2 64 x 48, seed 21, THIN (0.1, 5), batch 4, rel_error 0.3): 6 rounds, and the sample counts 8, 16, 20
    and 24 among the pixels with hits; the assertions rounds >= 2 and two distinct counts keep the pass from being vacuous"""
    w, h, batch = 64, 48, 4
    cfg = dict(min_spp=batch, max_spp=6 * batch, batch_spp=batch, max_rounds=0, rel_error=0.3, abs_floor=0.02)
    a, b = handles("thai2", w=w, h=h, seed=21), handles("thai2", tag="twin", w=w, h=h, seed=21)
    for rt in (a, b):
        rt.set_lens(**THIN)
    snaps = {0: film_of(b)}
    for k in range(1, 7):
        b.render(batch)
        snaps[k * batch] = film_of(b)
    # round by round: the verdict is adaptive.tile_mask on the film read back, and exactly its tiles get the batch
    rounds = 0
    while True:
        s, q, n = a.film.pixel_datas()
        replay = ad.tile_mask(s, q, n, w, h, **cfg)
        mask = a.adaptive_tile_mask(**cfg)
        assert np.array_equal(mask, replay)
        st = a.refine(**dict(cfg, max_rounds=1))
        assert st["tiles_active_first"] == int(replay.sum()) and st["rounds"] == (1 if replay.any() else 0)
        n1 = a.film.pixel_datas()[2]
        assert np.array_equal(n1, n + np.where(pixels_of(replay, w, h), batch, 0))
        if not replay.any():
            break
        rounds += 1
        assert rounds <= 6
    got = film_of(a)
    hit = got[0].any(axis=1)
    print("refine under THIN: %d rounds, sample counts among the pixels with hits %s" % (rounds, np.unique(got[2][hit]).tolist()))
    assert rounds >= 2 and len(np.unique(got[2][hit])) >= 2
    for k, snap in snaps.items():
        m = got[2] == k
        assert same_film(got, snap, m), k
    assert set(np.unique(got[2]).tolist()) <= set(snaps)
    # one call from an empty film does the same
    a.film.clear()
    st = a.refine(**cfg)
    assert st["rounds"] == rounds and st["tiles_active_last"] == 0 and st["samples_added"] == int(got[2].sum()) and same_film(film_of(a), got)
    # the guides are untouched: the denoised read-out serves this film under the lens, as it does on the twin given the same film
    s, q, n = a.film.pixel_datas()
    b.film.set(s, q, n)
    da, db = a.get_denoised_pixels(), b.get_denoised_pixels()
    assert np.array_equal(bits(da[0]), bits(db[0])) and np.array_equal(da[1], db[1])


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_change_nothing(pkg, scenes, handles):
    import ctypes as C
    rt = handles("ico2")
    rt.render(2)
    for _ in range(2):
        rt.trace_frame_additive()
    before, row, counts = film_of(rt), rt.current_row, rt.last_counts().as_dict()
    tx, ty = tiles_of(W, H)
    mask = np.ones(ty * tx + 1, np.uint8)
    addr = mask.ctypes.data
    call = pkg.lib().mi355rt_render_tiles
    cases = [("tile_mask", (None, ty * tx, 3, pkg.RAYS_HOST)), ("ntiles", (addr, ty * tx - 1, 3, pkg.RAYS_HOST)), ("ntiles", (addr, ty * tx + 1, 3, pkg.RAYS_HOST)),
             ("spp", (addr, ty * tx, 0, pkg.RAYS_HOST)), ("where", (addr, ty * tx, 3, 2))]
    for word, (m, nt, spp, where) in cases:
        rc = pkg.RayCounts()
        assert call(rt._h, m, nt, spp, where, C.byref(rc)) == E_INVALID, word
        err = pkg.lib().mi355rt_last_error(rt._h).decode()
        assert "mi355rt_render_tiles" in err and word in err, err
        assert same_film(film_of(rt), before) and rt.current_row == row and rt.last_counts().as_dict() == counts
    with pytest.raises(RuntimeError, match="spp"):
        rt.render_tiles(mask[:-1], 0)
    g = make(pkg, scenes, "ico2", device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    g.render(2)
    gn = g.film.pixel_datas()[2].copy()
    with pytest.raises(RuntimeError, match="device group"):
        g.render_tiles(mask[:-1], 3)
    assert np.array_equal(g.film.pixel_datas()[2], gn)
    g.close()


# ---- 9. guard tails -------------------------------------------------------------------------------------------------------------------------------------------------
GUARD_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
import importlib
pkg = ge.load_package()
sio = importlib.import_module("raytracer_rs_amd.scene_io")
scene = sio.load_scene_file(sys.argv[2])
for w, h in ((37, 21), (64, 48)):
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=5, flags=pkg.FLAG_DIRECT_FILM)
    tx, ty = (w + 7) // 8, (h + 7) // 8
    y, x = np.mgrid[0:ty, 0:tx]
    mask = ((x + y) % 2 == 0).astype(np.uint8)
    one = np.zeros((ty, tx), np.uint8); one[ty // 2, tx // 2] = 1
    for lens in (dict(model="pinhole"), dict(model="thin", radius=0.1, focus=5.0), dict(model="ortho", width_world=9.5)):
        rt.set_lens(**lens)
        rt.render_tiles(mask, 3)
        rt.render_tiles(one, 2)
        rt.render_tiles(np.ones((ty, tx), np.uint8), 1)
    bad = rt.debug_check_guards()
    print("guards", w, h, bad)
    if bad != 0:
        sys.exit(3)
    rt.close()
print("child ok")
"""


def test_guard_tails_stay_clean(tmp_path):
    script = tmp_path / "guard_child.py"
    script.write_text(GUARD_CHILD)
    env = dict(os.environ, MI355RT_DEBUG_GUARD="1")
    r = subprocess.run([sys.executable, str(script), ROOT, os.path.join(SCENES, "thai2.scene")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "child ok" in r.stdout and r.stdout.count("guards") == 2


# ---- 10. the CLI ------------------------------------------------------------------------------------------------------------------------------------------------------
def run_cli(args, w=48, h=40, seed=17):
    return subprocess.run([EXE, "-f", os.path.join(SCENES, "thai2.scene"), "--width", str(w), "--height", str(h), "--seed", str(seed)] + args,
                          capture_output=True, text=True, timeout=300)


def ppm_pixels(path, w, h):
    data = open(path, "rb").read()
    hdr = ("P6\n%d %d\n255\n" % (w, h)).encode()
    assert data.startswith(hdr)
    return np.frombuffer(data[len(hdr):], np.uint8).reshape(-1, 3)


def rgb_of(px):
    return np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8)


@pytest.mark.parametrize("model", ["pinhole", "thin"])
def test_cli_region_writes_the_library_frame(pkg, scenes, ad, tmp_path, model):
    w, h = 48, 40
    out = tmp_path / ("r.png" if model == "thin" else "r.ppm")         # both writers
    lens = ["--lens", "thin", "--lens-radius", "0.1", "--focus", "5"] if model == "thin" else []
    r = run_cli(["--region", "10,4,30,19", "--spp", "3", "--out", str(out)] + lens)
    assert r.returncode == 0, r.stderr
    rt = make(pkg, scenes, "thai2", w, h, seed=17)
    rt.set_lens(**LENSES[model])
    mask = ad.region_mask(w, h, 10, 4, 30, 19)
    assert mask.sum() == 3 * 3
    c = rt.render_tiles(mask, 3)
    assert "%d primary" % c.primary in r.stdout
    want = rgb_of(rt.get_tonemapped_pixels())
    if model == "thin":
        pw, ph, got = read_png(str(out))
        assert (pw, ph) == (w, h)
    else:
        got = ppm_pixels(out, w, h)
    assert want.any() and np.array_equal(got, want)
    rt.close()


def test_cli_refine_under_a_lens_and_the_exclusions(pkg, scenes, tmp_path):
    w, h = 48, 40
    out = tmp_path / "f.ppm"
    r = run_cli(["--refine", "0.05", "--lens", "thin", "--lens-radius", "0.1", "--focus", "5", "--abs-floor", "0.03", "--min-spp", "4", "--max-spp", "16", "--batch", "4",
                 "--out", str(out)])
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("adaptive:")]
    assert len(line) == 1
    rt = make(pkg, scenes, "thai2", w, h, seed=17)
    rt.set_lens(**THIN)
    st = rt.refine(min_spp=4, max_spp=16, batch_spp=4, rel_error=0.05, abs_floor=0.03)
    want = "adaptive: %u rounds, %u of %u tiles active at the first verdict, %u at the last, %u samples added (%.2f per owned pixel)" % (
        st["rounds"], st["tiles_active_first"], st["tiles"], st["tiles_active_last"], st["samples_added"], st["samples_added"] / (w * h))
    assert line[0].startswith(want), (line[0], want)
    assert st["rounds"] >= 2
    assert np.array_equal(ppm_pixels(out, w, h), rgb_of(rt.get_tonemapped_pixels()))
    rt.close()
    for args, names in [(["--region", "0,0,8,8", "--spp", "2", "--gpus", "2"], ("--region", "--gpus")),
                        (["--region", "0,0,8,8", "--spp", "2", "-i", "2"], ("--region", "-i")),
                        (["--region", "0,0,8,8", "--spp", "2", "--adaptive", "0.1"], ("--region", "--adaptive")),
                        (["--region", "0,0,8,8"], ("--region", "--spp")),
                        (["--region", "0,0,8,8", "--spp", "2", "--refine", "0.1"], ("--region", "--refine")),
                        (["--refine", "0.1", "--spp", "2"], ("--refine", "--spp")),
                        (["--refine", "0.1", "--gpus", "2"], ("--refine", "--gpus")),
                        (["--refine", "0.1", "-i", "2"], ("--refine", "-i")),
                        (["--refine", "0.1", "--adaptive", "0.1"], ("--refine", "--adaptive"))]:
        r = run_cli(args)
        assert r.returncode != 0 and all(n in r.stderr for n in names), (args, r.stderr)
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--refine" in r.stdout and "--region" in r.stdout
