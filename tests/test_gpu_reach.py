"""Which nodes of a sample's radiance tree were reached, and what the resolve kernels make of the others.  The light terms of a slot are zero-filled by the
primary round and overwritten by whoever shades a node; every reader (resolve_kernel, resolve_rays_kernel, the fused kernel's resolve phase, debug_sample)
folds the whole tree, so an unreached node must read back as +0.0 and nothing an earlier pass left in the buffers may show.  The pass buffers of a handle
are reused by every frame: these tests render several DIFFERENT frames on one handle first and then compare one more frame, bit for bit, with the CPU oracle
and with a handle that never rendered anything else.  The second half walks resolve_kernel's sample loop — several samples per lane and turn, all their loads
in flight before the in-order exchange — over every samples-per-pixel count at which it takes another shape."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 4
# (seed, samples per pixel, camera step) of the warm-up frames: the largest pass first, so that the later ones reuse its buffers instead of growing new ones
WARM = ((11, 6, ("move", 0.2, 0.0, 0.0)), (12, 5, ("yaw", 0.15)), (13, 3, ("pitch", -0.1)), (14, 2, ("move", 0.0, -0.1, 0.2)))
LAST = (21, ("yaw", -0.05))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def step(cam_owner, move, is_oracle):
    kind, args = move[0], move[1:]
    if is_oracle:
        {"move": cam_owner.camera_move_rel, "yaw": cam_owner.camera_add_y_angle, "pitch": cam_owner.camera_add_x_angle}[kind](*args)
    else:
        {"move": cam_owner.camera.move_rel, "yaw": cam_owner.camera.add_y_angle, "pitch": cam_owner.camera.add_x_angle}[kind](*args)


def scene_with_lights(scenes, name, nlights):
    """the file's light, then (3 lights) one BEHIND the object as the camera sees it — many hits face away from it and fail mod.rs:218 — and one to the side;
    built like test_several_lights_on_multi_leaf_octrees builds its scene"""
    sc = dict(scenes(name))
    if nlights == 1:
        return sc
    base = sc["lights"][0].copy()
    v = sc["tri_verts"].reshape(-1, 3)
    centre = (v.min(0) + v.max(0)) * np.float32(0.5)
    eye = np.asarray(sc["camera_matrix"], np.float32).reshape(4, 4)[3, :3]
    behind = np.concatenate([2.0 * centre - eye, [2.0, 5.0, 8.0]]).astype(np.float32)
    side = np.array([6.0, -2.5, 3.0, 4.0, 1.0, 0.5], np.float32)
    sc["lights"] = np.stack([base, behind, side])[:nlights].astype(np.float32)
    return sc


def used_handle(pkg, sc, w, h, flags, rec, spread, **kw):
    """a handle whose pass buffers hold the trees of four other frames, left at the camera and seed of the frame under test with a clear film"""
    rt = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=WARM[0][0], recursions=rec, spread=spread, flags=flags, **kw)
    for seed, spp, move in WARM:
        rt.set_seed(seed); step(rt, move, False)
        rt.film.clear()
        rt.render(spp)
    rt.set_seed(LAST[0]); step(rt, LAST[1], False)
    rt.film.clear()
    return rt


def fresh_handle(pkg, sc, w, h, flags, rec, spread, **kw):
    rt = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=LAST[0], recursions=rec, spread=spread, flags=flags, **kw)
    for _, _, move in WARM:
        step(rt, move, False)
    step(rt, LAST[1], False)
    return rt


def fresh_oracle(oracle, sc, w, h, flags, rec, spread):
    orc = oracle.Oracle(sc, w, h, seed=LAST[0], recursions=rec, spread=spread, flags=flags)
    for _, _, move in WARM:
        step(orc, move, True)
    step(orc, LAST[1], True)
    return orc


def same_film(rt, other):
    gs, gq, gn = rt.film.pixel_datas()
    os_, oq, on = other.film() if hasattr(other, "film") and callable(other.film) else other.film.pixel_datas()
    return np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))


TREES = [(2, 1), (3, 1), (2, 2)]          # 5, 16 and 13 nodes per sample: the first is folded flat by the resolve kernels, the others by the tree walk


# ---- 1. stale buffers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlights", [1, 3])
@pytest.mark.parametrize("rec,spread", TREES)
@pytest.mark.parametrize("name", ["ico2", "4boxes"])
def test_a_fifth_frame_on_a_used_handle_equals_the_oracle_and_a_fresh_handle(pkg, scenes, oracle, sem3, name, rec, spread, nlights):
    sc = scene_with_lights(scenes, name, nlights)
    rt = used_handle(pkg, sc, W, H, sem3.gpu, rec, spread)
    c = rt.render(SPP)
    orc = fresh_oracle(oracle, sc, W, H, sem3.orc, rec, spread)
    oc = orc.render(SPP, nthreads=8)
    assert (c.primary, c.bounce, c.shadow, c.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"])
    # reached and unreached child nodes: some reflection rays were proved free, some level-1 rays hit (their nodes made level-2 rays), and fewer
    # rays were made than a tree with every node reached has
    k0, k1 = spread * rec, spread * (rec - 1)
    full = k0 * (1 + k1 * (1 + (spread * (rec - 2) if rec > 2 else 0)))
    print("\n[reach %s rec %d spread %d lights %d %s] primary hits %d, bounce %d (skipped %d), every node reached would be %d"
          % (name, rec, spread, nlights, sem3, c.primary_hits, c.bounce, c.bounce_skipped, full * c.primary_hits))
    assert c.bounce_skipped > 0
    assert k0 * c.primary_hits < c.bounce < full * c.primary_hits
    assert same_film(rt, orc)
    assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())
    new = fresh_handle(pkg, sc, W, H, sem3.gpu, rec, spread)
    new.render(SPP)
    assert same_film(rt, new)
    rt.close(); new.close(); orc.close()


# ---- 2. per-node terms after reuse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec,spread", TREES)
@pytest.mark.parametrize("name", ["ico2", "4boxes"])
def test_per_node_terms_after_reuse(pkg, scenes, oracle, sem3, name, rec, spread):
    """debug_sample reads the terms back on the host: an unreached node reads 0.0, not what an earlier frame left in its planes"""
    sc = scene_with_lights(scenes, name, 3)
    rt = used_handle(pkg, sc, W, H, sem3.gpu, rec, spread)
    orc = fresh_oracle(oracle, sc, W, H, sem3.orc, rec, spread)
    rng = np.random.default_rng(31)
    first = np.cumsum([0, 1, spread * rec, spread * rec * spread * (rec - 1)])        # first node of levels 0, 1, 2 (and the end of level 2)
    reached = np.zeros(3, np.int64); unreached = np.zeros(3, np.int64)
    for pixel in rng.integers(0, W * H, 100):
        oc, ol, oh = orc.sample_debug(int(pixel), 2)
        gc, gl = rt.debug_sample(int(pixel), 2)
        assert np.array_equal(bits(gl), bits(ol)), (pixel, gl, ol)
        assert np.array_equal(bits(gc), bits(oc)), (pixel, gc, oc)
        assert not bits(gl)[oh == 0].any()                                            # +0.0, bit for bit
        for lv in range(3):
            reached[lv] += int(oh[first[lv]:first[lv + 1]].sum()); unreached[lv] += int((oh[first[lv]:first[lv + 1]] == 0).sum())
    assert reached.min() > 0 and unreached.min() > 0, (reached, unreached)
    rt.close(); orc.close()


# ---- 3. every reader ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec,spread", [(2, 1), (2, 2)])
def test_fused_50_row_frames_after_reuse(pkg, scenes, oracle, sem3, rec, spread):
    """trace_frame_additive(): the fused kernel's own primary round, secondary shade and resolve phase (64 x 50: a call is the whole frame)"""
    sc = scene_with_lights(scenes, "ico2", 3)
    rt = used_handle(pkg, sc, 64, 50, sem3.gpu, rec, spread)
    orc = fresh_oracle(oracle, sc, 64, 50, sem3.orc, rec, spread)
    for _ in range(2):
        assert rt.trace_frame_additive() == orc.trace_frame_additive() == 50 * 64
    assert same_film(rt, orc)
    c = rt.last_counts()
    assert c.bounce_skipped > 0 and c.bounce > spread * rec * c.primary_hits
    rt.close(); orc.close()


def test_ray_fed_passes_after_reuse(pkg, scenes, oracle, sem3):
    """trace_rays (resolve_rays_kernel) and render_rays (resolve_kernel behind a ray-fed primary round) on a used handle: the oracle's own primary rays,
    with their keys, give the oracle's colours and root light sums; as a film they give the oracle's film"""
    sc = scene_with_lights(scenes, "ico2", 3)
    w, h, sno = 37, 21, 3
    rt = used_handle(pkg, sc, w, h, sem3.gpu, 2, 1)
    orc = fresh_oracle(oracle, sc, w, h, sem3.orc, 2, 1)
    n = w * h
    keys = np.ascontiguousarray(np.stack([np.arange(n, dtype=np.uint32), np.full(n, sno, np.uint32)], axis=1))
    other = np.array([orc.primary_ray(p, sno + 1) for p in range(n)], np.float32)
    rt.trace_rays(other, keys, want=("rgb", "direct"))                                  # other trees in the slots the next call uses
    rays = np.array([orc.primary_ray(p, sno) for p in range(n)], np.float32)
    dbg = [orc.sample_debug(p, sno) for p in range(n)]
    got = rt.trace_rays(rays, keys, want=("rgb", "direct"))
    assert np.array_equal(bits(got["rgb"]), bits(np.array([d[0] for d in dbg], np.float32)))
    assert np.array_equal(bits(got["direct"]), bits(np.array([d[1][0] for d in dbg], np.float32)))
    hit = np.array([d[2][0] for d in dbg], bool)
    assert 0 < hit.sum() < n
    film_rays = np.concatenate([np.array([orc.primary_ray(p, s) for p in range(n)], np.float32) for s in range(3)])
    rt.render_rays(film_rays, 3)
    orc.render(3, nthreads=8)
    assert same_film(rt, orc)
    rt.close(); orc.close()


def test_direct_film_after_reuse(pkg, scenes, oracle, sem3):
    """MI355RT_FLAG_DIRECT_FILM: the DIRECT instantiations of the resolve kernels; the direct film against a fresh handle's and against the oracle's root terms"""
    sc = scene_with_lights(scenes, "ico2", 3)
    w, h = 37, 21
    rt = used_handle(pkg, sc, w, h, sem3.gpu | pkg.FLAG_DIRECT_FILM, 2, 1)
    orc = fresh_oracle(oracle, sc, w, h, sem3.orc, 2, 1)
    rt.render(SPP); orc.render(SPP, nthreads=8)
    assert same_film(rt, orc)
    new = fresh_handle(pkg, sc, w, h, sem3.gpu | pkg.FLAG_DIRECT_FILM, 2, 1)
    new.render(SPP)
    assert same_film(rt, new)
    d = rt.film.direct_sums()
    assert np.array_equal(bits(d), bits(new.film.direct_sums()))
    want = np.zeros((w * h, 3), np.float32)
    for s in range(SPP):
        want = want + np.array([orc.sample_debug(p, s)[1][0] for p in range(w * h)], np.float32)
    assert np.array_equal(bits(d), bits(want)) and d.any()
    rt.close(); new.close(); orc.close()


def test_masked_render_after_reuse(pkg, scenes, oracle, sem3):
    """an adaptive-style pass with inactive tiles (render_tiles, a checkerboard): active pixels equal the oracle's, inactive ones are not written at all"""
    sc = scene_with_lights(scenes, "ico2", 3)
    rt = used_handle(pkg, sc, W, H, sem3.gpu, 2, 1)
    orc = fresh_oracle(oracle, sc, W, H, sem3.orc, 2, 1)
    ty, tx = np.mgrid[0:H // 8, 0:W // 8]
    mask = ((tx + ty) % 2 == 0).astype(np.uint8)
    py, px = np.mgrid[0:H, 0:W]
    on = (mask[py // 8, px // 8] != 0).reshape(-1)
    marker = np.full((W * H, 3), -7.5, np.float32)                                       # what an unwritten pixel must still hold afterwards
    rt.film.set(np.where(on[:, None], np.float32(0.0), marker), np.where(on[:, None], np.float32(0.0), marker), np.zeros(W * H, np.uint32))
    c = rt.render_tiles(mask, 3)
    assert c.primary == 3 * int(on.sum())
    orc.render(3, nthreads=8)
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on_ = orc.film()
    assert np.array_equal(gn, np.where(on, 3, 0))
    assert np.array_equal(bits(gs)[on], bits(os_)[on]) and np.array_equal(bits(gq)[on], bits(oq)[on])
    assert np.array_equal(bits(gs)[~on], bits(marker)[~on]) and np.array_equal(bits(gq)[~on], bits(marker)[~on])
    rt.close(); orc.close()


# ---- 4. resolve shapes ---------------------------------------------------------------------------------------------------------------------
_SHAPES = {}


@pytest.fixture(scope="module")
def shape_handles(pkg, scenes, oracle):
    """one handle and one oracle per image size, shared by the sample counts: every case clears both films first"""
    def get(w, h):
        if (w, h) not in _SHAPES:
            _SHAPES[(w, h)] = (pkg.create_raytracer_from_arrays(scenes("ico2"), 70, w, h, seed=9), oracle.Oracle(scenes("ico2"), w, h, seed=9))
        rt, orc = _SHAPES[(w, h)]
        rt.film.clear(); orc.film_clear()
        return rt, orc
    yield get
    for rt, orc in _SHAPES.values():
        rt.close(); orc.close()
    _SHAPES.clear()


@pytest.mark.parametrize("spp", [1, 3, 4, 5, 31, 32, 33, 64, 96, 97, 130])
@pytest.mark.parametrize("w,h", [(40, 24), (37, 5)])
def test_resolve_shapes(shape_handles, w, h, spp):
    """both sides of every lanes-per-pixel boundary of launch_resolve and of every samples-per-turn count, with remainders; the second render adds to the
    film of the first, so the order of the additions shows"""
    rt, orc = shape_handles(w, h)
    for _ in range(2):
        c = rt.render(spp); oc = orc.render(spp, nthreads=8)
        assert (c.primary, c.bounce, c.shadow) == (oc["primary"], oc["bounce"], oc["shadow"])
    assert same_film(rt, orc)
    assert np.all(rt.film.pixel_datas()[2] == 2 * spp)


@pytest.mark.parametrize("spp", [3, 33, 97])
@pytest.mark.parametrize("rec,spread", [(0, 1), (1, 3), (1, 4), (2, 2), (3, 1)])
def test_resolve_shapes_of_other_trees(pkg, scenes, oracle, rec, spread, spp):
    """the same loop over the other ways a tree is folded: one node, one level of 3 and of 4 children (folded flat, like the reference's own tree), and the
    13- and 16-node trees that are walked node by node for the samples of a turn together"""
    w, h = 37, 5
    rt = pkg.create_raytracer_from_arrays(scenes("ico2"), 70, w, h, seed=9, recursions=rec, spread=spread)
    orc = oracle.Oracle(scenes("ico2"), w, h, seed=9, recursions=rec, spread=spread)
    for _ in range(2):
        c = rt.render(spp); oc = orc.render(spp, nthreads=8)
        assert (c.primary, c.bounce, c.shadow) == (oc["primary"], oc["bounce"], oc["shadow"])
    assert same_film(rt, orc)
    rt.close(); orc.close()


# ---- 5. signed zero -------------------------------------------------------------------------------------------------------------------------
def test_a_film_of_negative_zeros_takes_one_black_sample(pkg, scenes, oracle):
    """a pixel whose samples all miss skips resolve_kernel's sample loop: one addition of +0.0 instead of one per sample.  -0.0 + 0.0 is +0.0: put -0.0 in
    through the film-set entry, render one sample of a view in which most pixels miss, and the all-miss pixels hold the bits of +0.0 and n = 1"""
    w, h = 96, 64
    rt = pkg.create_raytracer_from_arrays(scenes("ico2"), 70, w, h, seed=4)
    orc = oracle.Oracle(scenes("ico2"), w, h, seed=4)
    rt.camera.add_y_angle(0.35); orc.camera_add_y_angle(0.35)
    neg = np.full((w * h, 3), -0.0, np.float32)
    assert np.all(bits(neg) == 0x80000000)
    rt.film.set(neg, neg, np.zeros(w * h, np.uint32)); orc.film_set(neg, neg, np.zeros(w * h, np.uint32))
    c = rt.render(1); oc = orc.render(1, nthreads=4)
    assert c.primary_hits == oc["primary_hits"] and 0 < c.primary_hits < w * h // 2
    gs, gq, gn = rt.film.pixel_datas()
    assert same_film(rt, orc) and np.all(gn == 1)
    black = ~bits(gs).any(axis=1)
    assert black.sum() >= w * h - c.primary_hits                                        # every pixel whose sample missed holds +0.0, bit for bit
    assert not (bits(gs) == 0x80000000).any() and not (bits(gq) == 0x80000000).any()
    rt.close(); orc.close()
