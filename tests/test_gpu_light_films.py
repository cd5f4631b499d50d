"""Light films on the device (include/mi355rt.h, "LIGHT FILMS"): a handle created with FLAG_LIGHT_FILMS keeps one plane per light that
holds, per pixel, the f32 sum in sample order of its samples' colour with every other light black -- bit-equal to the film of a CPU oracle whose other
lights' colours are (0, 0, 0); the flag changes nothing else; every entry that adds samples adds to the planes for the same pixels and no others;
mi355rt_get_relit_pixels equals its numpy statement (raytracer_rs_amd.relight) bit for bit and, at weight 1, the film mean to rounding; what is refused."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID = -1
EXTRA_LIGHTS = np.array([[-3.0, 4.0, -2.0, 2.0, 5.0, 8.0], [6.0, -2.5, 3.0, 4.0, 1.0, 0.5], [1.5, 6.0, 2.5, 3.0, 3.0, 1.0], [-4.0, -3.0, 5.0, 0.5, 4.0, 2.0],
                         [2.0, 2.0, -6.0, 6.0, 0.5, 3.0], [-1.0, 7.0, 1.0, 1.0, 2.0, 7.0], [5.0, 5.0, 5.0, 2.5, 2.5, 2.5], [-6.0, 1.0, -1.0, 3.5, 0.25, 1.5]], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def with_lights(scenes, name, nlights, ntri=None):
    """the scene `name` with `nlights` lights: its own first, then EXTRA_LIGHTS (test_gpu_parity.py builds multi-light scenes the same way)"""
    sc = dict(scenes(name))
    if ntri is not None:
        sc["tri_verts"] = sc["tri_verts"][:ntri].copy(); sc["tri_geom"] = sc["tri_geom"][:ntri].copy()
    sc["lights"] = np.concatenate([sc["lights"][:1], EXTRA_LIGHTS])[:nlights].astype(np.float32).copy()
    return sc


def only_light(sc, li):
    """the scene with every light's colour but li's set to (0, 0, 0)"""
    one = dict(sc)
    one["lights"] = sc["lights"].copy()
    one["lights"][np.arange(len(one["lights"])) != li, 3:] = 0.0
    return one


def make(pkg, sc, w, h, flags=0, lights=True, **kw):
    return pkg.create_raytracer_from_arrays(sc, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, flags=flags | (pkg.FLAG_LIGHT_FILMS if lights else 0), **kw)


@pytest.fixture(scope="module")
def relight(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.relight")


# ---- 1. oracle parity, bit for bit -------------------------------------------------------------------------------------------------------
def check_against_oracles(pkg, oracle, sc, w, h, spps, gflags, oflags, seed=5, **tree):
    nl = len(sc["lights"])
    rt = make(pkg, sc, w, h, flags=gflags, seed=seed, **tree)
    assert rt.nlights == nl and rt.light_films.get().shape == (nl, w * h, 3) and not rt.light_films.get().any()      # zero at creation
    full = oracle.Oracle(sc, w, h, seed=seed, flags=oflags, **tree)
    ones = [oracle.Oracle(only_light(sc, li), w, h, seed=seed, flags=oflags, **tree) for li in range(nl)]
    for spp in spps:
        rt.render(spp)
        full.render(spp, nthreads=8)
        gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = full.film()
        assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
        L = rt.light_films.get()
        for li, o in enumerate(ones):
            o.render(spp, nthreads=8)
            want = o.film()[0]
            assert np.array_equal(bits(L[li]), bits(want)), (spp, li, int((bits(L[li]) != bits(want)).sum()))
    assert nl == 0 or L.any()
    return rt, L


@pytest.mark.parametrize("name,nl,rec,spread,spps", [("ico2", 3, 2, 1, (1, 3, 5)), ("4boxes", 4, 3, 1, (3,)), ("ico3_tex", 2, 1, 4, (7,))])
def test_light_films_equal_the_oracles_with_the_other_lights_black(pkg, scenes, oracle, sem3, name, nl, rec, spread, spps):
    """flat fold (ico2: the reference's tree; ico3_tex: five nodes) and node_radiance (4boxes: 16 nodes); spps accumulate, so film_n offsets are exercised"""
    check_against_oracles(pkg, oracle, with_lights(scenes, name, nl), 40, 24, spps, sem3.gpu, sem3.orc, recursions=rec, spread=spread)


def test_light_films_of_the_maximum_of_eight_lights(pkg, scenes, oracle, sem3):
    rt, L = check_against_oracles(pkg, oracle, with_lights(scenes, "4boxes", 8, ntri=48), 24, 16, (2,), sem3.gpu, sem3.orc)
    assert all(L[li].any() for li in range(8))


@pytest.mark.parametrize("spp", [33, 37, 100])
def test_light_films_in_the_four_and_eight_lane_groups(pkg, scenes, oracle, spp):
    """33 and 37 spp: four lanes per pixel, 100: eight; each leaves a tail turn in which some of a lane's U = 2 samples do not exist"""
    check_against_oracles(pkg, oracle, with_lights(scenes, "ico2", 2), 16, 8, (spp,), 0, 0)


# ---- 2. one light --------------------------------------------------------------------------------------------------------------------------
def test_one_light_film_is_the_film(pkg, scenes, sem):
    rt = make(pkg, scenes("thai2"), 48, 40, flags=sem.gpu, seed=3)
    assert rt.nlights == 1
    rt.render(3)
    s = rt.film.pixel_datas()[0]
    assert s.any() and np.array_equal(bits(rt.light_films.get()[0]), bits(s))


# ---- 3. the flag changes nothing else ---------------------------------------------------------------------------------------------------
COUNTERS = ("primary", "bounce", "shadow", "primary_hits", "primary_culled", "shadow_skipped")


@pytest.mark.parametrize("w,h", [(96, 70), (9, 7)])
def test_the_flag_changes_nothing_else(pkg, scenes, w, h):
    sc = with_lights(scenes, "ico2", 2)
    off = make(pkg, sc, w, h, flags=pkg.FLAG_DIRECT_FILM, lights=False, seed=8)
    on = make(pkg, sc, w, h, flags=pkg.FLAG_DIRECT_FILM, seed=8)
    assert on.hbm_allocated_bytes() - off.hbm_allocated_bytes() == 2 * w * h * 12
    ca, cb = off.render(3), on.render(3)
    assert [getattr(ca, k) for k in COUNTERS] == [getattr(cb, k) for k in COUNTERS]
    for a, b in zip(off.film.pixel_datas(), on.film.pixel_datas()):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    assert np.array_equal(bits(off.film.direct_sums()), bits(on.film.direct_sums()))
    assert np.array_equal(off.get_tonemapped_pixels(), on.get_tonemapped_pixels())
    assert on.light_films.get().any()


# ---- 4. every sample-adding entry ---------------------------------------------------------------------------------------------------------
W4, H4, K4, SEED4 = 24, 16, 8, 9
THIN = dict(model="thin", radius=0.1, focus=5.0)
_PREFIX = {}


def prefix(pkg, scenes, lens, name="ico2"):
    """P[k, li, p] = light film li of pixel p after its first k samples (P[0] = 0), from a handle that takes them one per call under `lens`; the film's
    sample keys are (p, film_n[p] + s), so a pixel with k samples holds P[k] however they arrived.  Computed once per lens and scene, shared, never modified."""
    if (lens, name) not in _PREFIX:
        rt = make(pkg, with_lights(scenes, name, 2), W4, H4, seed=SEED4)
        if lens == "thin":
            rt.set_lens(**THIN)
        P = np.zeros((K4 + 1, 2, W4 * H4, 3), np.float32)
        for k in range(K4):
            rt.render(1)
            P[k + 1] = rt.light_films.get()
        assert P[K4].any()
        P.setflags(write=False)
        _PREFIX[lens, name] = P
    return _PREFIX[lens, name]


def planes_for(P, n):
    n = np.asarray(n, np.int64)
    return np.stack([P[n, li, np.arange(n.size)] for li in range(P.shape[1])])


def checkerboard(rt):
    ty, tx = (rt.height + 7) // 8, (rt.width + 7) // 8
    mask = ((np.arange(ty)[:, None] + np.arange(tx)[None, :]) % 2).astype(np.uint8)
    pix = np.repeat(np.repeat(mask, 8, axis=0), 8, axis=1)[: rt.height, : rt.width].reshape(-1).astype(bool)
    return mask, pix


def test_render_tiles_adds_inside_the_mask_and_keeps_the_bits_outside(pkg, scenes):
    P = prefix(pkg, scenes, "pinhole")
    rt = make(pkg, with_lights(scenes, "ico2", 2), W4, H4, seed=SEED4)
    mask, inside = checkerboard(rt)
    assert inside.any() and not inside.all()
    pre = np.zeros((2, W4 * H4, 3), np.uint32)
    pre[:] = 0x80000000                                            # -0.0: the first sample's addition turns it into what a zero plane holds
    pre[:, ~inside & (np.arange(W4 * H4) % 2 == 1)] = 0x7FC12345    # a NaN with a payload
    rt.light_films.set(pre.view(np.float32))
    assert np.array_equal(bits(rt.light_films.get()), pre)
    rt.render_tiles(mask, 3)
    n = rt.film.pixel_datas()[2]
    assert np.array_equal(n, np.where(inside, 3, 0))
    L = rt.light_films.get()
    assert np.array_equal(bits(L)[:, ~inside], pre[:, ~inside])
    assert np.array_equal(bits(L)[:, inside], bits(planes_for(P, n))[:, inside])
    rt.render_tiles(1 - mask, 2)                                   # the other tiles, onto the NaNs and the -0.0
    L2 = rt.light_films.get()
    assert np.array_equal(bits(L2)[:, inside], bits(L)[:, inside])
    was_zero = ~inside & (np.arange(W4 * H4) % 2 == 0)
    assert np.array_equal(bits(L2)[:, was_zero], bits(P[2])[:, was_zero]) and np.isnan(L2[:, ~inside & ~was_zero]).all()


def test_render_adaptive_adds_to_the_light_films_of_the_active_tiles(pkg, scenes):
    """thai2: some of the six tiles settle after the first batch (the parameters of test_gpu_direct_film.py's adaptive case), so a settled tile keeps its sums"""
    P = prefix(pkg, scenes, "pinhole", "thai2")
    rt = make(pkg, with_lights(scenes, "thai2", 2), W4, H4, seed=SEED4)
    st = rt.render_adaptive(min_spp=3, max_spp=K4, batch_spp=3, max_rounds=2, rel_error=0.3, abs_floor=0.05)
    n = rt.film.pixel_datas()[2]
    print("adaptive: rounds %d, n %s" % (st["rounds"], np.unique(n).tolist()))
    assert st["rounds"] == 2 and len(np.unique(n)) > 1 and n.max() <= K4
    assert np.array_equal(bits(rt.light_films.get()), bits(planes_for(P, n)))


def test_render_rays_with_the_pinhole_rays_is_render(pkg, scenes):
    import importlib
    cams = importlib.import_module("raytracer_rs_amd.cameras")
    P = prefix(pkg, scenes, "pinhole")
    rt = make(pkg, with_lights(scenes, "ico2", 2), W4, H4, seed=SEED4)
    rt.render(2)
    rays = cams.pinhole(rt.camera.matrices(), W4, H4, 3, SEED4, film_n=rt.film.pixel_datas()[2])
    rt.render_rays(rays, 3)
    assert np.array_equal(bits(rt.light_films.get()), bits(P[5]))


def test_a_thin_lens_render_adds_to_the_light_films(pkg, scenes):
    P = prefix(pkg, scenes, "thin")
    assert not np.array_equal(bits(P[3]), bits(prefix(pkg, scenes, "pinhole")[3]))
    rt = make(pkg, with_lights(scenes, "ico2", 2), W4, H4, seed=SEED4)
    rt.set_lens(**THIN)
    rt.render(3)
    assert np.array_equal(bits(rt.light_films.get()), bits(P[3]))
    rt.render(2, wait=False)                                       # mi355rt_render_async: the read-out settles the queued frame
    assert np.array_equal(bits(rt.light_films.get()), bits(P[5]))


def test_a_striped_handle_writes_its_rows_and_the_ranks_add_up(pkg, scenes):
    P = prefix(pkg, scenes, "pinhole")
    sc = with_lights(scenes, "ico2", 2)
    whole = make(pkg, sc, W4, H4, seed=SEED4)
    rows = np.arange(W4 * H4) // W4
    for rank in range(2):
        st = make(pkg, sc, W4, H4, seed=SEED4, stripe_rows=4, stripe_rank=rank, stripe_world=2)
        own = (rows // 4) % 2 == rank
        poison = np.full((2, W4 * H4, 3), 7.0, np.float32)
        st.light_films.set(poison)                                 # only the owned rows are written
        got = st.light_films.get()
        assert (got[:, own] == 7.0).all() and not got[:, ~own].any()
        st.film.clear()                                            # ... and cleared
        assert not st.light_films.get().any()
        st.render(3)
        L = st.light_films.get()
        assert not L[:, ~own].any() and np.array_equal(bits(L)[:, own], bits(P[3])[:, own])
        whole.light_films.add(L)
    assert np.array_equal(bits(whole.light_films.get()), bits(P[3]))


# ---- 5. relit against its statement ------------------------------------------------------------------------------------------------------
def hand_made(w, h, nl, seed):
    """planes and counts no render produces: n == 0 pixels, NaN, +-inf, denormals, -0.0 and negative values among ordinary ones"""
    rng = np.random.default_rng(seed)
    npix = w * h
    L = rng.uniform(0.0, 40.0, (nl, npix, 3)).astype(np.float32)
    n = rng.integers(1, 9, npix).astype(np.uint32)
    special = np.array([np.nan, np.inf, -np.inf, 1e-42, -1e-42, -0.0, 0.0, -3.5, 3e38], np.float32)
    for k in range(min(npix, 3 * len(special))):
        L[k % nl, (k * 5) % npix, k % 3] = special[k % len(special)]
    n[::7] = 0
    L[0, ::14] = 0.0                                               # n == 0 over a zero plane and over a non-zero one
    return L, n


WEIGHTS = {"one": lambda nl: np.ones(nl, np.float32), "zero": lambda nl: np.zeros(nl, np.float32), "negative": lambda nl: -np.arange(1, nl + 1, dtype=np.float32) * F(0.75),
           "per_channel": lambda nl: (np.arange(nl * 3, dtype=np.float32).reshape(nl, 3) * F(0.37) - F(0.5))}
DISPLAYS = [dict()] + [dict(curve=c, transfer=t, exposure=1.7, white=2.5) for c in range(4) for t in range(2)] + [dict(auto_exposure=1, curve=1, transfer=1, key=0.2, low=0.05, high=0.95)]


def assert_relit_is_the_statement(pkg, relight, rt, L, n):
    table = pkg.display_srgb_thresholds()
    for wname, wf in WEIGHTS.items():
        wts = wf(L.shape[0])
        for cfg in DISPLAYS:
            rgb, packed, used = rt.get_relit_pixels(wts, rgb=True, **cfg)
            wrgb, wpacked, wused = relight.relit_pixels(L, n, wts, thresholds=table, **cfg)
            nan = np.isnan(wrgb)
            assert np.array_equal(np.isnan(rgb), nan) and np.array_equal(bits(rgb)[~nan], bits(wrgb)[~nan]), (wname, cfg)
            assert np.array_equal(packed, wpacked), (wname, cfg)
            assert bits(np.float32(used)) == bits(np.float32(wused)), (wname, cfg, used, wused)


@pytest.mark.parametrize("w,h", [(24, 16), (1, 1)])
def test_relit_equals_its_statement_on_hand_made_planes(pkg, scenes, relight, w, h):
    """rgb bit for bit where it is a number (a NaN is a NaN: which payload an operation on two NaNs keeps is not part of the statement), packed integer for integer"""
    rt = make(pkg, with_lights(scenes, "ico2", 3), w, h)
    L, n = hand_made(w, h, 3, 11)
    if w * h == 1:
        n[:] = 2
    zero = np.zeros((w * h, 3), np.float32)
    rt.film.set(zero, zero, n)
    assert not rt.light_films.get().any()                          # film.set leaves the planes alone
    rt.light_films.set(L)
    assert np.array_equal(bits(rt.light_films.get()), bits(L))
    assert_relit_is_the_statement(pkg, relight, rt, L, n)
    if w * h == 1:
        rt.film.set(zero, zero, np.zeros(1, np.uint32))            # n == 0
        assert_relit_is_the_statement(pkg, relight, rt, L, np.zeros(1, np.uint32))


def test_relit_equals_its_statement_on_rendered_planes(pkg, scenes, relight):
    rt = make(pkg, with_lights(scenes, "ico2", 3), 24, 16, seed=2)
    rt.render(3)
    L, n = rt.light_films.get(), rt.film.pixel_datas()[2]
    before = [bits(x).copy() for x in rt.film.pixel_datas()[:2]]
    assert_relit_is_the_statement(pkg, relight, rt, L, n)
    assert np.array_equal(bits(rt.light_films.get()), bits(L))     # the call only reads
    assert all(np.array_equal(bits(a), b) for a, b in zip(rt.film.pixel_datas()[:2], before))


# ---- 6. relit at weight 1 against the film mean ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nl,rec,spread,nodes,spp", [("ico2", 3, 2, 1, 5, 5), ("4boxes", 4, 3, 1, 16, 3), ("ico3_tex", 2, 1, 4, 5, 7)])
def test_relit_at_weight_one_is_the_film_mean_to_rounding(pkg, scenes, name, nl, rec, spread, nodes, spp):
    """Every term is non-negative, so nothing cancels: one rounding per addition or multiplication on either path bounds the difference by
    (n + nl * nodes + 3 * nl + 2) * 2^-23 * mean per channel, and it is zero where the mean is zero."""
    rt = make(pkg, with_lights(scenes, name, nl), 40, 24, seed=5, recursions=rec, spread=spread)
    rt.render(spp)
    mean = rt.film.get_pixels().astype(np.float64)
    rgb = rt.get_relit_pixels(np.ones(nl, np.float32), rgb=True)[0].astype(np.float64)
    assert np.isfinite(rgb).all() and (mean >= 0).all() and mean.any()
    bound = (spp + nl * nodes + 3 * nl + 2) * 2.0 ** -23 * mean
    err = np.abs(rgb - mean)
    print("relit - mean: largest share of the bound %.3f" % float((err[mean > 0] / bound[mean > 0]).max()))
    assert (err <= bound).all()
    assert not rgb[mean == 0].any()


# ---- 7. errors and guards ----------------------------------------------------------------------------------------------------------------
def last_error(pkg, rt):
    return (pkg.lib().mi355rt_last_error(rt._h) or b"").decode()


def test_invalid_calls_are_refused_and_write_nothing(pkg, scenes):
    lib = pkg.lib()
    sc = with_lights(scenes, "ico2", 2)
    w, h = 24, 16
    npix = w * h
    rt = make(pkg, sc, w, h)
    plain = make(pkg, sc, w, h, lights=False)
    rt.render(1)
    L0 = rt.light_films.get()
    buf = np.full((2, npix, 3), 5.0, np.float32)
    wts = np.ones(6, np.float32)
    rgb = np.full((npix, 3), 5.0, np.float32); packed = np.full(npix, 5, np.uint32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def refused(handle, code, word):
        assert code == E_INVALID and word in last_error(pkg, handle), (code, word, last_error(pkg, handle))
        assert (buf == 5.0).all() and (rgb == 5.0).all() and (packed == 5).all()
        assert np.array_equal(bits(rt.light_films.get()), bits(L0))

    for fn in (lib.mi355rt_light_films_get, lib.mi355rt_light_films_set, lib.mi355rt_light_films_add):
        refused(plain, fn(plain._h, fp(buf), 2, npix), "MI355RT_FLAG_LIGHT_FILMS")
        refused(rt, fn(rt._h, fp(buf), 3, npix), "nlights")
        refused(rt, fn(rt._h, fp(buf), 2, npix - 1), "npix")
        refused(rt, fn(rt._h, None, 2, npix), "light_rgb")
    relit = lib.mi355rt_get_relit_pixels
    refused(plain, relit(plain._h, fp(wts), 6, None, fp(rgb), up(packed), npix, None), "MI355RT_FLAG_LIGHT_FILMS")
    refused(rt, relit(rt._h, fp(wts), 5, None, fp(rgb), up(packed), npix, None), "nweights")
    refused(rt, relit(rt._h, None, 6, None, fp(rgb), up(packed), npix, None), "weights3")
    refused(rt, relit(rt._h, fp(wts), 6, None, fp(rgb), up(packed), npix + 1, None), "npix")
    refused(rt, relit(rt._h, fp(wts), 6, None, None, None, npix, None), "both NULL")
    for field, value, word in [("source", 1, "source"), ("source", 3, "source"), ("curve", 4, "curve"), ("transfer", 2, "transfer"), ("auto_exposure", 2, "auto_exposure"),
                               ("exposure", 0.0, "exposure"), ("white", float("nan"), "white"), ("key", -1.0, "key")]:
        c = pkg.display_config(**{field: value})
        refused(rt, relit(rt._h, fp(wts), 6, C.byref(c), fp(rgb), up(packed), npix, None), word)
    # either output alone is fine
    assert relit(rt._h, fp(wts), 6, None, fp(rgb), None, npix, None) == 0 and relit(rt._h, fp(wts), 6, None, None, up(packed), npix, None) == 0
    assert np.array_equal(packed, rt.get_relit_pixels(np.ones(2, np.float32))[0])


def test_create_guards(pkg, scenes):
    sc9 = dict(with_lights(scenes, "4boxes", 8, ntri=48))
    sc9["lights"] = np.concatenate([sc9["lights"], sc9["lights"][:1] + F(0.5)]).astype(np.float32)
    assert len(sc9["lights"]) == 9
    with pytest.raises(RuntimeError, match="MI355RT_FLAG_LIGHT_FILMS"):
        make(pkg, sc9, 24, 16)
    assert make(pkg, sc9, 24, 16, lights=False).nlights == 9        # accepted without the flag
    with pytest.raises(RuntimeError, match="MI355RT_FLAG_LIGHT_FILMS"):
        make(pkg, with_lights(scenes, "ico2", 2), 24, 16, flags=pkg.FLAG_GROUP_SHARES_DEVICE, device_count=2)
    none = make(pkg, with_lights(scenes, "4boxes", 0, ntri=48), 24, 16)          # no light: no planes
    none.render(1)
    assert none.light_films.get().shape == (0, 24 * 16, 3)
    rgb, packed, _ = none.get_relit_pixels(np.zeros((0, 3), np.float32), rgb=True)
    assert not rgb.any() and not np.signbit(rgb).any()


def test_drop_in_frames_flags_clear_and_film_set(pkg, scenes):
    sc = with_lights(scenes, "ico2", 2)
    rt = make(pkg, sc, 24, 16, seed=4)
    rt.render(2)
    film = [np.asarray(x).copy() for x in rt.film.pixel_datas()]
    L = rt.light_films.get()
    assert pkg.lib().mi355rt_trace_frame_additive(rt._h) == 0 and "MI355RT_FLAG_LIGHT_FILMS" in last_error(pkg, rt)
    assert all(np.array_equal(np.asarray(a).view(np.uint32), b.view(np.uint32)) for a, b in zip(rt.film.pixel_datas(), film))
    assert np.array_equal(bits(rt.light_films.get()), bits(L))
    with pytest.raises(RuntimeError, match="create-time"):
        rt.set_flags(0)
    rt.set_flags(pkg.FLAG_LIGHT_FILMS | pkg.FLAG_FIX_ROW_INDEX)    # the bit passed unchanged
    plain = make(pkg, sc, 24, 16, lights=False)
    with pytest.raises(RuntimeError, match="create-time"):
        plain.set_flags(pkg.FLAG_LIGHT_FILMS)
    rt.film.set(film[0] * F(2), film[1], film[2])
    assert np.array_equal(bits(rt.light_films.get()), bits(L))     # film.set leaves the planes alone
    rt.film.clear()
    assert not rt.light_films.get().any() and not bits(rt.light_films.get()).any()


def test_memory_is_counted_and_steady(pkg, scenes):
    """Allocated on first use and kept (include/mi355rt.h): 16 bytes per pixel and the weights with the first get_relit_pixels; the display section's
    histogram and sRGB table with the first display config.  Everything else is the same before and after."""
    sc = with_lights(scenes, "ico2", 3)
    w, h = 24, 16
    off, rt = make(pkg, sc, w, h, lights=False), make(pkg, sc, w, h)
    base = rt.hbm_allocated_bytes()
    assert base - off.hbm_allocated_bytes() == 3 * w * h * 12
    L = rt.light_films.get(); rt.light_films.set(L); rt.light_films.add(L)
    assert rt.hbm_allocated_bytes() == base
    rt.get_relit_pixels(np.ones(3, np.float32))
    first = rt.hbm_allocated_bytes()
    assert first - base == w * h * 16 + 8 * 12
    rt.get_relit_pixels(np.ones(3, np.float32), rgb=True)
    assert rt.hbm_allocated_bytes() == first
    rt.get_relit_pixels(np.ones(3, np.float32), transfer=1, auto_exposure=1)
    second = rt.hbm_allocated_bytes()
    assert second - first == 1040 + 1024
    rt.get_relit_pixels(np.ones(3, np.float32), transfer=1, auto_exposure=1); rt.light_films.get(); rt.light_films.add(L)
    assert rt.hbm_allocated_bytes() == second


# ---- 8. the CLI ----------------------------------------------------------------------------------------------------------------------------
def scene_file_with_lights(src, dst, lights):
    """a copy of the scene file src (raytracer_rs_amd/scene_io.py has the layout) whose light records are `lights` (float32[n, 6])"""
    import struct
    data = open(src, "rb").read()
    ntri, nmat, nlight, ntex, ncam = struct.unpack_from("<5I", data, 8)
    off = 28 + ntri * 40 + nmat * 20
    lights = np.ascontiguousarray(lights, np.float32)
    with open(dst, "wb") as f:
        f.write(data[:8] + struct.pack("<5I", ntri, nmat, len(lights), ntex, ncam) + data[28:off] + lights.tobytes() + data[off + nlight * 24:])


def read_png_rgb(path):
    """uint8[npix, 3] of an 8-bit RGB PNG whose scanlines all use filter 0 (what the CLI writes)"""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        ln, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + ln]
        if kind == b"IHDR":
            size = struct.unpack(">II", body[:8]); assert body[8:] == bytes([8, 2, 0, 0, 0])
        elif kind == b"IDAT":
            idat += body
        pos += 12 + ln
    w, h = size
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(-1, 3)


def rgb_of(px):
    return np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8)


def test_cli_light_film_options(pkg, scenes, scene_io, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "raytracer-rs_amd", "bin", "raytracer")
    w, h = 40, 24
    path = str(tmp_path / "three_lights.scene")
    scene_file_with_lights(os.path.join(root, "tests", "golden", "scenes", "4boxes.scene"), path, with_lights(scenes, "4boxes", 3)["lights"])
    sc = scene_io.load_scene_file(path)
    assert len(sc["lights"]) == 3
    base = [exe, "-f", path, "--width", str(w), "--height", str(h), "--seed", "17", "--spp", "4"]
    run = lambda extra: subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
    r = run(["--light-films", "--relight", "1,0.25,0", "--srgb", "--out", str(tmp_path / "relit.png"), "--out-lights", str(tmp_path / "light")])
    assert r.returncode == 0, r.stderr
    assert "light films: 3 lights\n" in r.stdout and "display: exposure 1\n" in r.stdout
    rt = make(pkg, sc, w, h, seed=17)
    rt.render(4)
    want = rt.get_relit_pixels([1.0, 0.25, 0.0], transfer=pkg.TRANSFER_SRGB)[0]
    assert np.array_equal(read_png_rgb(tmp_path / "relit.png"), rgb_of(want))
    for li in range(3):
        one = rt.get_relit_pixels(np.eye(3, dtype=np.float32)[li], transfer=pkg.TRANSFER_SRGB)[0]
        assert np.array_equal(read_png_rgb(tmp_path / ("light%d.png" % li)), rgb_of(one))
    assert not np.array_equal(want, rt.get_display_pixels(transfer=pkg.TRANSFER_SRGB)[0])
    # the flag alone, and no option at all: the bytes the CLI always wrote
    for extra in (["--light-films"], []):
        r = run(extra + ["--out", str(tmp_path / "plain.png")])
        assert r.returncode == 0, r.stderr
        assert np.array_equal(read_png_rgb(tmp_path / "plain.png"), rgb_of(rt.get_tonemapped_pixels()))
    r = run(["--light-films", "--relight", "1,2", "--out", str(tmp_path / "bad.png")])
    assert r.returncode == 1 and "3 lights" in r.stderr
