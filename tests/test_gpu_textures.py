"""The texture path on the device (fetch_texel in csrc/kernels.hip, the texel pool upload in csrc/renderer.cpp, the marshalling of
create_raytracer_from_arrays) on hand-made scenes with nine textures of different shapes -- 1x1, one row, one column, wider than tall, taller
than wide, 4099 wide -- whose material index, texture id and position in the texel pool all differ:

(a) rays with chosen barycentrics on unit "cards" come back with the radiance of exactly the texel that texture.rs:21-27 names: the statement
    of those lines below (`texel_index`) is written from the reference's text, not from the kernel or from oracle.c;
(b) the albedo guide of a pinhole view equals that statement bit for bit;
(c) whole frames with two bounces (reflection rays land on textured triangles) are bit-equal to the CPU oracle: film, direct film,
    render_rays, one light and two.  oracle.c's get_texel is a transcription of the kernel's lines, clamp included, so (c) alone could not
    see an error the two share: (a) and (b), which rest on the independent statement, are what make (c) meaningful;
(d) the scene container: textures stored as bytes and as floats load to the arrays they were written from, in C++ and in scene_io;
(e) what create refuses; (f) 25 random cases of tools/parity_fuzz.py with random textures on random materials."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MISS = 0xFFFFFFFF
USIZE_MAX = 2 ** 64 - 1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the independent statement of texture.rs:21-27 -------------------------------------------------------------------------------------------
def as_usize(x):
    """Rust's `f32 as usize`: truncation toward zero; NaN and negatives give 0, values past the type's range its maximum"""
    x = float(x)
    if not x > 0.0:
        return 0
    return USIZE_MAX if x >= 2.0 ** 64 else int(x)


def texel_index(width, height, u, v):
    """`x = (u * width as f32) as usize; y = (v * height as f32) as usize; &data[y * width + x]`: the index, in Python integers, and whether
    the reference would panic there.  u == 1 is column `width`: the first texel of the next row, not the last of this one.  Only an index
    past the last texel is clamped to it (the project's documented divergence)."""
    x = as_usize(F(u) * F(width))
    y = as_usize(F(v) * F(height))
    i = y * width + x
    return (i, False) if i < width * height else (width * height - 1, True)


def texels_of(texture, u, v):
    """float32[n, 3]: the texel of each (u, v), and bool[n]: the clamp was taken"""
    h, w = texture.shape[:2]
    flat = np.asarray(texture, F).reshape(-1, 3)
    idx = [texel_index(w, h, a, b) for a, b in zip(u, v)]
    return flat[[i for i, _ in idx]], np.array([c for _, c in idx], bool)


# ---- nine textures, fifteen materials ------------------------------------------------------------------------------------------------------------
TEX_SHAPES = [(1, 1), (2, 1), (1, 2), (3, 5), (5, 3), (7, 2), (640, 1), (4099, 3), (16, 16)]          # (width, height): texture id = pool order
# material -> texture id (None: a coloured material).  Reversed against the pool, coloured ones in between, texture 3 used by two materials.
MAT_TEX = [None, 8, 7, None, 6, 5, None, 4, 3, None, 2, 1, None, 0, 3]
MAT_OF_TEX = {t: m for m, t in enumerate(MAT_TEX[:-1]) if t is not None}
SHARED_MAT = 14


def probe_textures():
    """texels (r, 0.5, 0): r = k / 16384 with every k of the scene different, in scrambled order, so that a texel names itself"""
    total = sum(w * h for w, h in TEX_SHAPES)
    assert total < 16384
    r = ((np.random.default_rng(5).permutation(total) + 1).astype(F) / F(16384.0)).astype(F)
    out, first = [], 0
    for w, h in TEX_SHAPES:
        t = np.zeros((h, w, 3), F)
        t[:, :, 0] = r[first:first + w * h].reshape(h, w); t[:, :, 1] = 0.5
        out.append(t); first += w * h
    return out


def random_textures(seed, as_bytes):
    rng = np.random.default_rng(seed)
    if as_bytes:
        return [(rng.integers(0, 256, (h, w, 3)).astype(F) / F(256.0)).astype(F) for w, h in TEX_SHAPES]
    return [rng.random((h, w, 3), dtype=F) * F(1.5) for w, h in TEX_SHAPES]


def materials():
    n = len(MAT_TEX)
    kind = np.array([0 if t is None else 1 for t in MAT_TEX], np.uint32)
    rgb = np.array([[0.9, 0.05 * m, 1.0 - 0.05 * m] for m in range(n)], F)                    # of a textured material: a decoy, never read
    tex = np.array([(m * 5) % len(TEX_SHAPES) if t is None else t for m, t in enumerate(MAT_TEX)], np.uint32)    # of a coloured one: a decoy too
    return kind, rgb, tex


def camera_at(x, y, z):
    m = np.eye(4, dtype=F).reshape(-1)
    m[12:15] = (x, y, z)                                     # looks along +z, +x to the right, +y up (camera.rs:80-90)
    return m


def scene_of(tris, geom, textures, lights, camera, fov):
    kind, rgb, tex = materials()
    return dict(tri_verts=np.asarray(tris, F).reshape(-1, 9), tri_geom=np.asarray(geom, np.uint32), mat_kind=kind, mat_rgb=rgb, mat_tex=tex,
                lights=np.asarray(lights, F).reshape(-1, 6), textures=textures, camera_matrix=camera, camera_fov=F(fov))


# ---- (a) the cards ----------------------------------------------------------------------------------------------------------------------------------
def card_materials(first):
    """card k's material: every texture on a card of its own, texture `first` on card 0, where u = a holds for every float a (elsewhere a is
    what is left after 4k was added in f32, a multiple of 2^-21 or coarser); the last card shares texture 3 through the second material"""
    return [MAT_OF_TEX[t] for t in [first] + [t for t in (3, 4, 5, 7, 0, 1, 2, 6, 8) if t != first]] + [SHARED_MAT]


def cards_scene(first):
    mats = card_materials(first)
    tris = [[4 * k, 0, 0, 4 * k + 1, 0, 0, 4 * k, 1, 0] for k in range(len(mats))]
    tris.append([0, 0, -1, 1, 0, -1, 0, 1, -1])                                           # off the plane: the scene's bounds have volume
    return scene_of(tris, mats + [0], probe_textures(), [[-60.0, 0.5, 1.0, 1.0, 1.0, 1.0]], camera_at(18.0, 0.5, 30.0), 40.0)


def coordinates(n, rng):
    """k / n as f32 computes it, its two neighbours, 0, the last float below 1, and 1; every k up to n = 64, beyond that the ends, the middle
    and 40 random k"""
    ks = np.arange(n + 1) if n <= 64 else np.unique(np.concatenate([[0, 1, 2, 3, n // 2, n - 3, n - 2, n - 1, n], rng.integers(0, n + 1, 40)]))
    c = (ks.astype(F) / F(n)).astype(F)
    c = np.concatenate([c, np.nextafter(c, F(-1)), np.nextafter(c, F(2)), np.array([0.0, 1.0 - 2.0 ** -24, 1.0], F)]).astype(F)
    return np.unique(c[(c >= 0) & (c <= 1)])


def centres(w, h):
    """(u, v) of the centre of every texel, row by row"""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return ((x.reshape(-1) + 0.5) / w).astype(F), ((y.reshape(-1) + 0.5) / h).astype(F)


def card_rays(scene):
    """(rays6, card, u, v): per card the products of its texture's coordinates along both edges and 400 random pairs of them, 200 random
    points and the centre of every texel (of the textures up to 256 texels), of which those inside the triangle (fl(u + v) <= 1) stay.  u is
    what is left of the coordinate after 4k was added in f32."""
    rng = np.random.default_rng(17)
    rays, card, us, vs = [], [], [], []
    for k, m in enumerate(scene["tri_geom"][:-1]):
        th, tw = scene["textures"][MAT_TEX[m]].shape[:2]
        cu, cv = coordinates(tw, rng), coordinates(th, rng)
        mid_x, mid_y = centres(tw, th) if tw * th <= 256 else (np.zeros(0, F), np.zeros(0, F))
        u = np.concatenate([cu, np.zeros(cv.size, F), rng.choice(cu, 400), rng.random(200, dtype=F), mid_x])
        v = np.concatenate([np.zeros(cu.size, F), cv, rng.choice(cv, 400), rng.random(200, dtype=F), mid_y])
        ox = (F(4 * k) + u).astype(F)
        u = (ox - F(4 * k)).astype(F)                                                       # exact: ox lies in [4k, 4k + 1]
        keep = (u + v).astype(F) <= F(1.0)
        u, v, ox = u[keep], v[keep], ox[keep]
        r = np.zeros((u.size, 6), F)
        r[:, 0] = ox; r[:, 1] = v; r[:, 2] = 1.0; r[:, 5] = -1.0
        rays.append(r); card.append(np.full(u.size, k)); us.append(u); vs.append(v)
    return np.concatenate(rays), np.concatenate(card), np.concatenate(us), np.concatenate(vs)


def check_the_sweep(scene, card, tuv, prim, u, v):
    """the conditions on the input of (a), on what the tracer returned"""
    assert np.array_equal(prim, card.astype(np.uint32))                                      # every ray hits its card
    assert np.array_equal(bits(tuv[:, 0]), bits(np.ones(len(card), F)))                    # every product of Moller-Trumbore is with 0 or 1:
    assert np.array_equal(bits(tuv[:, 1]), bits(u)) and np.array_equal(bits(tuv[:, 2]), bits(v))      # t = 1, u = a, v = b, exactly
    assert (tuv[:, 1] == 1.0).any() and (tuv[:, 2] == 1.0).any()
    widths = np.array([scene["textures"][MAT_TEX[scene["tri_geom"][k]]].shape[1] for k in card], F)
    fx = (tuv[:, 1] * widths).astype(F)
    above = (np.nextafter(tuv[:, 1], F(2)) * widths).astype(F)
    on_edge = (fx == np.floor(fx)) & (fx > 0) & (fx < widths)
    below_edge = (above == np.floor(above)) & (np.floor(fx) == above - 1)
    assert on_edge.sum() >= 50 and below_edge.sum() >= 50                                    # u * W an integer, and one ulp below such a point
    assert (on_edge & (card == 0)).sum() >= 2 and (below_edge & (card == 0)).any()           # ... on card 0 too, whose width is no power of two


@pytest.mark.parametrize("lbvh,first", [(False, 3), (True, 7), (False, 4), (True, 5)], ids=["host_bvh-3x5", "device_lbvh-4099x3", "host_bvh-5x3", "device_lbvh-7x2"])
def test_chosen_barycentrics_reach_the_texel_they_should(pkg, oracle, sem3, lbvh, first):
    """With one white light 60 units away in the cards' plane, n . l <= 1 / 60 < 2^-5, so the specular term pow32(-(n . l)) < 2^-160 rounds
    to exactly 0 in f32 and the radiance of a hit is (fl(r * ndl), fl(0.5 * ndl), 0) for the texel (r, 0.5, 0): blue == 0 proves the specular
    term gone, green gives ndl exactly, and red then names the texel -- compared with the one texture.rs:21-27 names for the returned (u, v)
    and the texture id of the material of the returned triangle."""
    scene = cards_scene(first)
    rays, card, u, v = card_rays(scene)
    orc = oracle.Oracle(scene, 8, 8, recursions=0, flags=sem3.orc)
    otuv, oprim = orc.intersect(rays, brute=bool(sem3.orc & oracle.FLAG_BRUTE_FORCE))
    check_the_sweep(scene, card, otuv, oprim, u, v)                                          # on the CPU first
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, 8, 8, recursions=0, flags=sem3.gpu | (pkg.FLAG_DEVICE_LBVH if lbvh else 0))
    assert rt.bvh_build_info()["on_device"] == lbvh
    out = rt.trace_rays(rays, want=("rgb", "tuv", "prim"))
    rgb, tuv, prim = out["rgb"], out["tuv"], out["prim"]
    check_the_sweep(scene, card, tuv, prim, u, v)
    assert not rgb[:, 2].any()                                                               # blue == 0: no specular term
    assert (rgb[:, 1] > 0).all()
    ndl = (F(2.0) * rgb[:, 1]).astype(F)
    assert (ndl <= F(1.0 / 60.0)).all() and (ndl >= F(1.0 / 100.0)).all()
    tex_id = np.array([MAT_TEX[int(scene["tri_geom"][p])] for p in prim])
    assert np.array_equal(scene["mat_tex"][scene["tri_geom"][prim]], tex_id)
    r_pred, clamped = np.zeros(len(prim), F), np.zeros(len(prim), bool)
    for t in range(len(TEX_SHAPES)):
        sel = tex_id == t
        assert sel.any()
        texel, clamped[sel] = texels_of(scene["textures"][t], tuv[sel, 1], tuv[sel, 2])
        assert np.array_equal(texel[:, 1:], np.tile(F([0.5, 0.0]), (int(sel.sum()), 1)))
        r_pred[sel] = texel[:, 0]
    for t in (0, 1, 6):                                                                      # 1x1, 2x1, 640x1: u = 1 is past the last texel
        assert (clamped & (tex_id == t) & (tuv[:, 1] == 1.0)).any(), t
    want = (r_pred * ndl).astype(F)
    wrong = np.flatnonzero(bits(rgb[:, 0]) != bits(want))
    assert wrong.size == 0, "%d of %d rays; the first: card %d u %r v %r red %r, expected %r" % (
        wrong.size, len(prim), card[wrong[0]], tuv[wrong[0], 1], tuv[wrong[0], 2], rgb[wrong[0], 0], want[wrong[0]])
    # every texel whose centre lies in the triangle was named by some ray (of the textures up to 256 texels: the sweep holds their centres).
    # Which texels those are is read off the array by row and column here, not through texel_index.
    for t, (w, h) in enumerate(TEX_SHAPES):
        if w * h <= 256:
            inside = {scene["textures"][t][y, x, 0] for y in range(h) for x in range(w) if (x + 0.5) / w + (y + 0.5) / h <= 0.99}
            assert len(inside) >= w * h // 3 and inside <= set(r_pred[tex_id == t]), t
    assert {int(m) for m in scene["tri_geom"][prim][tex_id == 3]} == {MAT_OF_TEX[3], SHARED_MAT}
    rt.close(); orc.close()


# ---- the gallery: nine tilted textured cards in front of the camera, a textured wall behind it ---------------------------------------------------
def gallery_scene(textures, two_lights=False):
    rng = np.random.default_rng(23)
    tris, geom = [], []
    for k, t in enumerate((3, 4, 5, 7, 0, 1, 2, 6, 8)):
        cx, cy = 1.5 * (k % 3 - 1), 1.5 * (k // 3 - 1)
        ax, ay = rng.uniform(-0.35, 0.35, 2)
        rot = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]]) @ np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        p00, p10, p01, p11 = (np.array([cx, cy, 0.0]) + rot @ np.array([sx * 0.7, sy * 0.7, 0.0]) for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1)))
        tris += [np.concatenate([p00, p01, p10]), np.concatenate([p11, p10, p01])]          # wound to face the camera (-z)
        geom += [MAT_OF_TEX[t]] * 2
    q = [np.array([x, y, -6.0]) for x, y in ((-15, -15), (15, -15), (-15, 15), (15, 15))]             # behind the camera, facing the cards (+z): where their
    tris += [np.concatenate([q[0], q[1], q[2]]), np.concatenate([q[3], q[2], q[1]])]          # reflection rays land
    geom += [SHARED_MAT] * 2
    b = [np.array([x, y, 2.0]) for x, y in ((-4, -4), (4, -4), (-4, 4), (4, 4))]              # a coloured backdrop seen between the cards
    tris += [np.concatenate([b[0], b[2], b[1]]), np.concatenate([b[3], b[1], b[2]])]
    geom += [3] * 2
    tris.append(np.array([-0.3, -0.3, -1.0, -0.3, 0.3, -1.0, 0.3, -0.3, -1.0]))              # a small coloured triangle in front
    geom.append(0)
    lights = [[0.8, 1.2, -3.0, 0.9, 0.8, 0.7]] + ([[-2.0, -1.0, -2.5, 0.3, 0.5, 0.9]] if two_lights else [])
    return scene_of(tris, geom, textures, lights, camera_at(0.0, 0.0, -4.0), 60.0)


@pytest.fixture(scope="module")
def gallery():
    cache = {}

    def get(two_lights=False, as_bytes=False):
        key = (two_lights, as_bytes)
        if key not in cache:
            cache[key] = gallery_scene(random_textures(31, as_bytes), two_lights)
        return cache[key]
    return get


def albedo_by_the_statement(scene, tuv, prim):
    alb = np.zeros((len(prim), 3), F)
    hit = np.flatnonzero(prim != MISS)
    mat = np.asarray(scene["tri_geom"])[prim[hit]]
    alb[hit] = scene["mat_rgb"][mat]
    for m in np.unique(mat):
        if scene["mat_kind"][m] == 1:
            sel = hit[mat == m]
            alb[sel] = texels_of(scene["textures"][int(scene["mat_tex"][m])], tuv[sel, 1], tuv[sel, 2])[0]
    return alb, hit, mat


# ---- (b) the albedo guide ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix_row", [False, True], ids=["reference_rows", "fixed_rows"])
def test_albedo_guide_equals_the_statement(pkg, oracle, gallery, sem3, fix_row):
    w, h = 64, 48
    scene = gallery()
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, flags=sem3.gpu | (pkg.FLAG_FIX_ROW_INDEX if fix_row else 0))
    orc = oracle.Oracle(scene, w, h, flags=sem3.orc)
    p = np.arange(w * h)
    rays = np.stack([orc.get_ray(int(a), int(b), 0.5, 0.5) for a, b in zip(p % w, p // w if fix_row else p // h)])      # the pixel-centre rays
    tuv, prim = rt.intersect_rays(rays)
    g = rt.guides()
    assert np.array_equal(g["prim"], prim)
    want, hit, mat = albedo_by_the_statement(scene, tuv, prim)
    textured = scene["mat_kind"][mat] == 1
    assert textured.sum() > 0.3 * w * h, "only %d of %d pixels on textured triangles" % (textured.sum(), w * h)
    seen = {int(t) for t in scene["mat_tex"][mat[textured]]}
    assert seen == set(range(len(TEX_SHAPES))), seen                                         # every texture is seen ...
    assert (~textured).any()                                                                 # coloured triangles are seen too
    assert np.array_equal(bits(g["albedo"]), bits(want))
    assert len(np.unique(bits(want[hit][textured]), axis=0)) > 100                            # ... and many different texels of them
    rt.close(); orc.close()


# ---- (c) whole frames ------------------------------------------------------------------------------------------------------------------------------
def film_bits(rt):
    s, q, n = rt.film.pixel_datas()
    return bits(s).copy(), bits(q).copy(), n.copy(), rt.get_tonemapped_pixels().copy()


@pytest.mark.parametrize("two_lights", [False, True], ids=["one_light", "two_lights"])
def test_frames_of_the_gallery_equal_the_oracle(pkg, oracle, gallery, sem3, two_lights):
    """Two bounces: the cards' reflection rays land on the textured wall behind the camera and the wall's on the cards, so every level of the
    radiance tree fetches texels.  The oracle's get_texel shares the kernel's transcription of the clamp (see the module's docstring): this
    test says that the frame is assembled from the fetch as the reference assembles it; that the fetch is right is (a) and (b)."""
    import importlib
    cams = importlib.import_module("raytracer_rs_amd.cameras")
    w, h, spp, seed = 40, 30, 3, 9
    scene = gallery(two_lights)
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, recursions=2, seed=seed, flags=sem3.gpu | pkg.FLAG_DIRECT_FILM)
    orc = oracle.Oracle(scene, w, h, recursions=2, seed=seed, flags=sem3.orc)
    rays = cams.pinhole(rt.camera.matrices(), w, h, spp, seed)
    c = rt.render(spp)
    oc = orc.render(spp, nthreads=8)
    assert (c.primary, c.bounce, c.shadow, c.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"])
    assert c.bounce > 2 * c.primary_hits                                                     # the bounce levels are there
    gs, gq, gn, packed = film_bits(rt)
    os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(gs, bits(os_)) and np.array_equal(gq, bits(oq))
    assert np.array_equal(packed, orc.get_tonemapped_pixels())
    # the direct film: the root light term of every sample, added in sample order
    direct = np.zeros((w * h, 3), F)
    reached_textured = 0
    for s in range(spp):
        for p in range(w * h):
            _, node_l, node_hit = orc.sample_debug(p, s)
            direct[p] = direct[p] + node_l[0]
            reached_textured += int(node_hit[1:].any())
    assert reached_textured > 0.3 * spp * w * h                                              # samples with bounce hits: on the wall, a card or the backdrop
    assert np.array_equal(bits(rt.film.direct_sums()), bits(direct))
    # the same frame from the camera's own rays
    rt.film.clear()
    rt.render_rays(rays, spp)
    s2, q2, n2, packed2 = film_bits(rt)
    assert np.array_equal(n2, gn) and np.array_equal(s2, gs) and np.array_equal(q2, gq) and np.array_equal(packed2, packed)
    assert np.array_equal(bits(rt.film.direct_sums()), bits(direct))
    rt.close(); orc.close()


# ---- (d) the scene container -----------------------------------------------------------------------------------------------------------------------
def write_scene_file(path, sc, as_bytes):
    """the M355SCN1 layout as scene_io.load_scene_file documents it by reading it"""
    with open(path, "wb") as f:
        f.write(b"M355SCN1" + struct.pack("<5I", len(sc["tri_geom"]), len(sc["mat_kind"]), len(sc["lights"]), len(sc["textures"]), 1))
        f.write(np.ascontiguousarray(sc["tri_verts"], F).tobytes() + np.ascontiguousarray(sc["tri_geom"], np.uint32).tobytes())
        for k, rgb, t in zip(sc["mat_kind"], sc["mat_rgb"], sc["mat_tex"]):
            f.write(struct.pack("<I3fI", int(k), *[float(x) for x in rgb], int(t)))
        f.write(np.ascontiguousarray(sc["lights"], F).tobytes())
        f.write(np.ascontiguousarray(sc["camera_matrix"], F).tobytes() + struct.pack("<f", float(sc["camera_fov"])))
        for t in sc["textures"]:
            h, w = t.shape[:2]
            f.write(struct.pack("<3I", w, h, 1 if as_bytes else 0))
            if as_bytes:
                q = np.asarray(t, F) * F(256.0)
                assert np.array_equal(q, np.floor(q)) and q.min() >= 0 and q.max() <= 255
                f.write(q.astype(np.uint8).tobytes())
            else:
                f.write(np.ascontiguousarray(t, F).tobytes())


@pytest.mark.parametrize("form", ["floats", "bytes", "byte_values_as_floats"])
def test_scene_files_with_textures_load_to_what_was_written(pkg, scene_io, gallery, tmp_path, form):
    scene = gallery(as_bytes=form != "floats")
    if form == "floats":                                                                     # the float form holds values no byte gives
        assert all((t * F(256.0) != np.floor(t * F(256.0))).any() for t in scene["textures"])
    path = str(tmp_path / "gallery.scene")
    write_scene_file(path, scene, as_bytes=form == "bytes")
    back = scene_io.load_scene_file(path)
    for key in ("tri_verts", "tri_geom", "mat_kind", "mat_rgb", "mat_tex", "lights", "camera_matrix"):
        assert back[key].dtype == scene[key].dtype and np.array_equal(back[key].view(np.uint32), scene[key].view(np.uint32)), key
    assert back["camera_fov"] == scene["camera_fov"] and len(back["textures"]) == len(scene["textures"])
    for a, b in zip(back["textures"], scene["textures"]):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b))
    w, h = 40, 30
    results = []
    for make in (lambda: pkg.create_raytracer_from_scene_file(path, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=3),
                 lambda: pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=3)):
        rt = make()
        g = rt.guides()
        rt.render(2)
        results.append([bits(g["depth"]), bits(g["normal"]), bits(g["albedo"]), g["prim"]] + list(film_bits(rt)))
        rt.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert results[0][2].any() and results[0][4].any()


# ---- (e) refusals at create ------------------------------------------------------------------------------------------------------------------------
def create_from_desc(pkg, sd):
    cfg = pkg.default_config(8, 8)
    handle = C.c_void_p()
    code = pkg.lib().mi355rt_create(C.byref(sd), C.byref(cfg), C.byref(handle))
    return code, handle.value, (pkg.lib().mi355rt_last_error(None) or b"").decode()


def test_create_refuses_textures_it_cannot_use(pkg, gallery):
    """each a RuntimeError naming the cause, and no handle is left"""
    scene = dict(gallery())
    # a textured material whose tex_id is the number of textures
    bad = dict(scene); bad["mat_tex"] = scene["mat_tex"].copy(); bad["mat_tex"][MAT_OF_TEX[0]] = len(TEX_SHAPES)
    with pytest.raises(RuntimeError, match="material texture id out of range"):
        pkg.create_raytracer_from_arrays(bad, pkg.DEFAULT_TRIANGLES_PER_LEAF, 8, 8)
    sd, keep = pkg.scene_desc(bad)
    code, handle, text = create_from_desc(pkg, sd)
    assert code != 0 and handle is None and "material texture id out of range" in text
    # ... which a coloured material may carry: its tex_id is not read
    fine = dict(scene); fine["mat_tex"] = scene["mat_tex"].copy(); fine["mat_tex"][0] = 1000
    pkg.create_raytracer_from_arrays(fine, pkg.DEFAULT_TRIANGLES_PER_LEAF, 8, 8).close()
    # a texture of width 0
    bad = dict(scene); bad["textures"] = list(scene["textures"]); bad["textures"][4] = np.zeros((3, 0, 3), F)
    with pytest.raises(RuntimeError, match="empty texture: texture 4 has width 0"):
        pkg.create_raytracer_from_arrays(bad, pkg.DEFAULT_TRIANGLES_PER_LEAF, 8, 8)
    sd, keep = pkg.scene_desc(scene)
    sd.textures[2].width = 0
    code, handle, text = create_from_desc(pkg, sd)
    assert code != 0 and handle is None and "empty texture: texture 2" in text
    # a texture whose array is shorter than width * height * 3.  The C struct carries no length, so the library cannot see this: the
    # marshalling refuses an array that is not (height, width, 3), and the entry point a texture without an array
    bad = dict(scene); bad["textures"] = list(scene["textures"]); bad["textures"][3] = scene["textures"][3][:, :, :2]
    with pytest.raises(RuntimeError, match=r"texture size mismatch: texture 3 has shape \(5, 3, 2\)"):
        pkg.create_raytracer_from_arrays(bad, pkg.DEFAULT_TRIANGLES_PER_LEAF, 8, 8)
    bad["textures"][3] = scene["textures"][3].reshape(-1)[:44]
    with pytest.raises(RuntimeError, match="texture size mismatch: texture 3"):
        pkg.create_raytracer_from_arrays(bad, pkg.DEFAULT_TRIANGLES_PER_LEAF, 8, 8)
    sd, keep = pkg.scene_desc(scene)
    sd.textures[7].rgb = None
    code, handle, text = create_from_desc(pkg, sd)
    assert code != 0 and handle is None and "empty texture: texture 7" in text
    # the untouched description is fine
    sd, keep = pkg.scene_desc(scene)
    code, handle, text = create_from_desc(pkg, sd)
    assert code == 0 and handle is not None
    pkg.lib().mi355rt_destroy(C.c_void_p(handle))


# ---- (f) fuzz ----------------------------------------------------------------------------------------------------------------------------------------
def test_randomised_cases_with_random_textures(pkg, scenes, oracle, monkeypatch):
    """tools/parity_fuzz.py with FUZZ_TEX + FUZZ_SOUP, 25 cases of a fixed seed: one to four random float textures (1..9 x 1..9, now and then 640
    wide) on random materials, the soup's included -- films, pixels and counters bit-equal to the oracle"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("parity_fuzz", os.path.join(ROOT, "tools", "parity_fuzz.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    for m in ("FUZZ_WILD", "FUZZ_SPP", "FUZZ_SOUP", "FUZZ_BUILD", "FUZZ_TEX"):
        monkeypatch.delenv(m, raising=False)
    monkeypatch.setenv("FUZZ_TEX", "1"); monkeypatch.setenv("FUZZ_SOUP", "1")
    rng = np.random.default_rng(77)
    textured = 0
    for _ in range(25):
        textured += int("+tex" in fuzz.one_case(pkg, oracle, scenes, rng, verbose=False))
    assert textured >= 10
