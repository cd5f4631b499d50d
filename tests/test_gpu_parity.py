"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same
seeded inputs.  Bit-exact for everything the render path computes: hit records, per-node light
terms, film sums, tonemapped pixels.  Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(pkg, scenes, name, w, h, **kw):
    tpl = kw.pop("triangles_per_leaf", pkg.DEFAULT_TRIANGLES_PER_LEAF)
    return pkg.create_raytracer_from_arrays(scenes(name), tpl, w, h, **kw)


def test_device_arithmetic_is_ieee(pkg, scenes, oracle):
    """a/b and sqrt on the device are correctly rounded (what numpy float32 gives), denormals
    included; a^32 equals the oracle's double-squaring evaluation of powf(x, 32.0)."""
    rt = make(pkg, scenes, "4boxes", 16, 16)
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.uniform(-4, 4, 200000), rng.uniform(0, 1e-38, 1000), [0.0, 1.0, -1.0, 1e30, 3e38, 1e-45]]).astype(np.float32)
    b = np.concatenate([rng.uniform(-3, 3, 200000), rng.uniform(1e-39, 1e-37, 1000), [1.0, 3.0, 7.0, 1e-30, 3.0, 2.0]]).astype(np.float32)
    q, r, p = rt.debug_numerics(a, b)
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(q), bits(a / b))
        ok = a >= 0
        assert np.array_equal(bits(r[ok]), bits(np.sqrt(a[ok])))
        expect = (a.astype(np.float64) ** 32).astype(np.float32)
    assert np.array_equal(bits(p), bits(expect))
    for i in range(0, 2000, 40):
        assert bits(np.float32(oracle.pow32(a[i])))[()] == bits(p[i:i + 1])[0]


@pytest.mark.parametrize("name", ["4boxes", "ico2", "thai2"])
def test_sample_table_matches_oracle(pkg, scenes, oracle, name):
    rt = make(pkg, scenes, name, 32, 32, seed=5)
    orc = oracle.Oracle(scenes(name), 32, 32, seed=5)
    assert np.array_equal(bits(rt.sample_table()), bits(orc.sample_table()))


@pytest.mark.parametrize("name,n", [("4boxes", 60000), ("ico2", 60000), ("thai2", 12000)])
def test_closest_hit_matches_brute_force_oracle(pkg, scenes, oracle, sem, name, n):
    """Intersector seam in both semantics (default: the reference's OctTreeIntersector; opt-out: NoAccelerationIntersector), bit-exact
    t/u/v and identical triangle, on primary rays, rays from surface points and random rays."""
    w, h = 320, 200
    rt = make(pkg, scenes, name, w, h, seed=3, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=3, flags=sem.orc)
    rng = np.random.default_rng(11)
    prim_rays = np.stack([orc.primary_ray(int(p), 0) for p in rng.integers(0, w * h, n // 3)])
    tuv, prim = orc.intersect(prim_rays, brute=bool(sem.orc & oracle.FLAG_BRUTE_FORCE))
    hitm = prim != 0xFFFFFFFF
    pts = prim_rays[hitm, :3] + tuv[hitm, :1] * prim_rays[hitm, 3:]
    dirs = rng.normal(size=(pts.shape[0], 3)).astype(np.float32)
    sec = np.concatenate([pts + 1e-5 * dirs, dirs], axis=1).astype(np.float32)
    sc = scenes(name)
    lo, hi = sc["tri_verts"].reshape(-1, 3).min(0), sc["tri_verts"].reshape(-1, 3).max(0)
    org = rng.uniform(lo - 2, hi + 2, (n // 3, 3)); tgt = rng.uniform(lo, hi, (n // 3, 3))
    rnd = np.concatenate([org, tgt - org], axis=1).astype(np.float32)
    rays = np.concatenate([prim_rays, sec, rnd]).astype(np.float32)
    o_tuv, o_prim = orc.intersect(rays, brute=bool(sem.orc & oracle.FLAG_BRUTE_FORCE))
    g_tuv, g_prim = rt.intersect_rays(rays)
    assert (o_prim != 0xFFFFFFFF).sum() > n // 10
    assert np.array_equal(g_prim, o_prim)
    m = o_prim != 0xFFFFFFFF
    assert np.array_equal(bits(g_tuv[m]), bits(o_tuv[m]))


def test_axis_parallel_and_degenerate_rays(pkg, scenes, oracle, sem):
    """zero direction components (1/0 = inf in the slab test), rays starting on surfaces."""
    name = "4boxes"
    rt = make(pkg, scenes, name, 64, 64, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), 64, 64, flags=sem.orc)
    rays = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            for k in range(200):
                o = np.array([2.0, 0.2, 2.0], np.float32) + np.float32(k * 0.013)
                d = np.zeros(3, np.float32); d[ax] = sgn
                o[ax] -= sgn * 9.0
                rays.append(np.concatenate([o, d]))
    rays.append(np.array([0, 0, 0, 0, 0, 0], np.float32))        # null direction: never hits
    rays.append(np.array([1.0, 1.0, 1.0, 0, -1, 0], np.float32))  # starts on a box face
    rays = np.stack(rays).astype(np.float32)
    o_tuv, o_prim = orc.intersect(rays, brute=bool(sem.orc & oracle.FLAG_BRUTE_FORCE))
    g_tuv, g_prim = rt.intersect_rays(rays)
    assert np.array_equal(g_prim, o_prim)
    m = o_prim != 0xFFFFFFFF
    assert m.sum() > 100
    assert np.array_equal(bits(g_tuv[m]), bits(o_tuv[m]))


@pytest.mark.parametrize("name", ["4boxes", "ico2", "thai2"])
def test_per_node_light_terms_match_oracle(pkg, scenes, oracle, sem, name):
    """stage-level parity: shade() term of every node of the radiance tree + the sample colour."""
    w, h = 96, 96
    rt = make(pkg, scenes, name, w, h, seed=9, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=9, flags=sem.orc)
    rng = np.random.default_rng(2)
    checked = 0
    for pixel in rng.integers(0, w * h, 150):
        oc, ol, oh = orc.sample_debug(int(pixel), 3)
        gc, gl = rt.debug_sample(int(pixel), 3)
        assert np.array_equal(bits(gl), bits(ol)), (pixel, gl, ol)
        assert np.array_equal(bits(gc), bits(oc)), (pixel, gc, oc)
        checked += int(oh[0])
    assert checked > 10


@pytest.mark.parametrize("name,w,h,spp", [("4boxes", 64, 64, 4), ("ico2", 64, 64, 4), ("thai2", 64, 64, 4), ("ico2", 96, 40, 3)])
def test_film_bit_exact_vs_brute_force_oracle(pkg, scenes, oracle, sem, name, w, h, spp):
    """whole path: seeded render, film sums / squares / counts and packed pixels identical."""
    rt = make(pkg, scenes, name, w, h, seed=1, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=1, flags=sem.orc)
    counts = rt.render(spp)
    oc = orc.render(spp, nthreads=8)
    assert (counts.primary, counts.bounce, counts.shadow, counts.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"])
    gs, gq, gn = rt.film.pixel_datas()
    os_, oq, on = orc.film()
    assert np.array_equal(gn, on)
    assert np.array_equal(bits(gs), bits(os_))
    assert np.array_equal(bits(gq), bits(oq))
    assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())
    assert np.array_equal(bits(rt.film.get_pixels()), bits(orc.get_pixels()))


def test_trace_frame_additive_matches_oracle(pkg, scenes, oracle, sem):
    """the reference's own entry: 50 rows x 1 sample per call, row cursor wraps, unsampled rows
    read back white (NaN -> 255), film.clear() restarts the accumulation but not the cursor."""
    name, w, h = "ico2", 64, 120
    rt = make(pkg, scenes, name, w, h, seed=4, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=4, flags=sem.orc)
    for call in range(4):
        assert rt.trace_frame_additive() == orc.trace_frame_additive() == 50 * w
        assert rt.current_row == orc.current_row
        g = rt.get_tonemapped_pixels(); o = orc.get_tonemapped_pixels()
        assert np.array_equal(g, o)
        if call == 0:
            assert np.all(g[50 * w:] == 0xFFFFFFFF)          # rows not sampled yet: white
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and gn.max() == 2 and gn.min() == 1
    assert np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
    rt.film.clear(); orc.film_clear()
    assert rt.trace_frame_additive() == orc.trace_frame_additive()
    assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())


def test_small_height_row_wrap(pkg, scenes, oracle, sem):
    """height < 50: one call wraps the row cursor and samples rows more than once."""
    name, w, h = "4boxes", 40, 16
    rt = make(pkg, scenes, name, w, h, seed=2, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=2, flags=sem.orc)
    assert rt.trace_frame_additive() == orc.trace_frame_additive()
    gs, _, gn = rt.film.pixel_datas(); os_, _, on = orc.film()
    assert np.array_equal(gn, on) and gn.max() == 4
    assert np.array_equal(bits(gs), bits(os_))


def test_camera_moves_match_oracle(pkg, scenes, oracle, sem):
    name, w, h = "ico2", 48, 48
    rt = make(pkg, scenes, name, w, h, seed=6, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=6, flags=sem.orc)
    rt.camera.move_rel(0.1, 0.0, 0.0); orc.camera_move_rel(0.1, 0.0, 0.0)
    rt.camera.add_y_angle(0.01); orc.camera_add_y_angle(0.01)
    rt.camera.add_x_angle(-0.02); orc.camera_add_x_angle(-0.02)
    rt.camera.move_rel(0.0, -0.1, 0.1); orc.camera_move_rel(0.0, -0.1, 0.1)
    for a, b in zip(rt.camera.matrices(), orc.camera_matrices()):
        assert np.array_equal(bits(a), bits(b))
    rt.film.clear(); orc.film_clear()
    rt.render(2); orc.render(2, nthreads=8)
    assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(orc.film()[0]))


def test_fix_row_index_flag(pkg, scenes, oracle, sem):
    name, w, h = "ico2", 80, 48
    rt = make(pkg, scenes, name, w, h, seed=8, flags=pkg.FLAG_FIX_ROW_INDEX | sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=8, flags=sem.orc | oracle.FLAG_FIX_ROW_INDEX)
    rt.render(2); orc.render(2, nthreads=8)
    assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(orc.film()[0]))


def test_textured_scene_matches_oracle(pkg, scenes, oracle, sem):
    """ico3_tex: Diffuse::TextureId -> nearest texel at the hit's barycentric (u, v)."""
    name, w, h = "ico3_tex", 64, 64
    rt = make(pkg, scenes, name, w, h, seed=1, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=1, flags=sem.orc)
    rt.render(3); orc.render(3, nthreads=8)
    assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(orc.film()[0]))


@pytest.mark.parametrize("rec,spread", [(0, 1), (1, 2), (3, 1), (2, 2)])
def test_other_recursion_settings(pkg, scenes, oracle, sem, rec, spread):
    name, w, h = "ico2", 40, 40
    rt = make(pkg, scenes, name, w, h, seed=1, recursions=rec, spread=spread, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), w, h, seed=1, recursions=rec, spread=spread, flags=sem.orc)
    c = rt.render(2); oc = orc.render(2, nthreads=8)
    assert (c.bounce, c.shadow) == (oc["bounce"], oc["shadow"])
    assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(orc.film()[0]))


def test_shadow_predicate(pkg, scenes, oracle, sem):
    """occluded_rays == `closest hit has 0.01 < t < 1.0` (mod.rs:226-229) on the oracle's closest hit."""
    name = "thai2"
    rt = make(pkg, scenes, name, 64, 64, flags=sem.gpu)
    orc = oracle.Oracle(scenes(name), 64, 64, flags=sem.orc)
    sc = scenes(name)
    rng = np.random.default_rng(5)
    lo, hi = sc["tri_verts"].reshape(-1, 3).min(0), sc["tri_verts"].reshape(-1, 3).max(0)
    org = rng.uniform(lo, hi, (6000, 3)); light = sc["lights"][0, :3]
    rays = np.concatenate([org, light - org], axis=1).astype(np.float32)
    tuv, prim = orc.intersect(rays, brute=bool(sem.orc & oracle.FLAG_BRUTE_FORCE))
    expect = (prim != 0xFFFFFFFF) & (tuv[:, 0] > np.float32(0.01)) & (tuv[:, 0] < np.float32(1.0))
    got = rt.occluded_rays(rays)
    assert expect.sum() > 100 and (~expect).sum() > 100
    assert np.array_equal(got.astype(bool), expect)


def test_stripes_partition_the_frame(pkg, scenes, oracle):
    """N stripe handles (the per-GPU decomposition) produce exactly the single-handle film."""
    name, w, h, spp = "ico2", 64, 50, 2
    full = make(pkg, scenes, name, w, h, seed=3)
    full.render(spp)
    fs, _, fn = full.film.pixel_datas()
    acc = np.zeros_like(fs); cnt = np.zeros_like(fn)
    for rank in range(3):
        part = make(pkg, scenes, name, w, h, seed=3, stripe_rows=4, stripe_rank=rank, stripe_world=3)
        part.render(spp)
        ps, _, pn = part.film.pixel_datas()
        rows = part.owned_rows()
        assert np.all((rows // 4) % 3 == rank)
        acc += ps; cnt += pn
    assert np.array_equal(cnt, fn)
    assert np.array_equal(bits(acc), bits(fs))


@pytest.mark.parametrize("slices", [1, 2, 3, 8])
def test_concurrent_frame_slices_do_not_change_the_film(pkg, scenes, oracle, sem, slices):
    """render() splits its rows into concurrent slices (own stream + pass buffers each): the film, the ray
    counts and repeated (accumulating) frames are identical to the oracle for every slice count, also when
    the slices need several passes each and when they are combined with multi-GPU stripes."""
    name, w, h, spp = "ico2", 72, 52, 3
    orc = oracle.Oracle(scenes(name), w, h, seed=5, flags=sem.orc)
    rt = make(pkg, scenes, name, w, h, seed=5, samples_per_pass=2, flags=sem.gpu)       # 2 passes per slice and frame
    rt.set_slices(slices)
    assert rt.get_slices() == slices
    for frame in range(2):
        counts = rt.render(spp)
        oc = orc.render(spp, nthreads=8)
        assert (counts.primary, counts.bounce, counts.shadow, counts.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"])
        gs, gq, gn = rt.film.pixel_datas()
        os_, oq, on = orc.film()
        assert np.array_equal(gn, on)
        assert np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
    # stripes x slices: rank 1 of 2 owns every other block of 4 rows, split again into slices
    part = make(pkg, scenes, name, w, h, seed=5, stripe_rows=4, stripe_rank=1, stripe_world=2, flags=sem.gpu)
    part.set_slices(slices)
    part.render(spp); part.render(spp)
    ps, _, pn = part.film.pixel_datas()
    rows = part.owned_rows()
    assert np.array_equal(pn.reshape(h, w)[rows], on.reshape(h, w)[rows]) and pn.sum() == len(rows) * w * 2 * spp
    assert np.array_equal(bits(ps).reshape(h, w, 3)[rows], bits(os_).reshape(h, w, 3)[rows])
    with pytest.raises(Exception):
        rt.set_slices(9)


# ---- committed golden fixtures (tests/golden/make_golden.py) --------------------------------------------
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", ["4boxes", "ico2", "thai2", "ico3_tex"])
def test_gpu_matches_golden_fixtures(pkg, scenes, name):
    """committed oracle outputs: brute-force arrays <-> MI355RT_FLAG_TRUE_CLOSEST_HIT (the octree arrays are checked by
    test_reference_default_semantics_match_golden_fixtures below)"""
    g = np.load(os.path.join(GOLDEN, "render_%s.npz" % name))
    rt = make(pkg, scenes, name, 64, 64, seed=1, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    c = rt.render(4)
    s, q, n = rt.film.pixel_datas()
    assert np.array_equal(bits(s), bits(g["brute_sum"])) and np.array_equal(bits(q), bits(g["brute_sumsq"]))
    assert np.array_equal(n, g["brute_n"]) and np.array_equal(rt.get_tonemapped_pixels(), g["brute_ldr"])
    assert [c.primary, c.bounce, c.shadow, c.primary_hits] == [int(x) for x in g["brute_counts"]]
    tuv, prim = rt.intersect_rays(g["rays"])
    assert np.array_equal(prim, g["brute_prim"])
    m = prim != 0xFFFFFFFF
    assert np.array_equal(bits(tuv[m]), bits(g["brute_tuv"][m]))


# ---- BASELINE.json sizes: size-independent properties -----------------------------------------------------
def test_full_size_frame_properties(pkg, scenes):
    """thai2 1920x1080: determinism, pass-size invariance (the film does not depend on how samples are
    batched into wavefront passes), exact sample counts, ray-count identities, stripe union."""
    w, h, spp = 1920, 1080, 6
    rt = make(pkg, scenes, "thai2", w, h, seed=1)
    c1 = rt.render(spp)
    s1, q1, n1 = rt.film.pixel_datas()
    assert np.all(n1 == spp)
    assert c1.primary == w * h * spp
    assert c1.bounce <= 2 * c1.primary_hits + c1.bounce // 2 + 1 and c1.bounce >= 2 * c1.primary_hits   # 2 children per primary hit, <= 1 each after
    assert c1.shadow <= c1.primary_hits + c1.bounce
    assert 0.2 < c1.primary_hits / c1.primary < 0.32                       # 0.26 at 1080p
    assert np.isfinite(s1).all()
    rt.film.clear()
    rt.render(spp)
    assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(s1))         # run-to-run bit-identical
    small = make(pkg, scenes, "thai2", w, h, seed=1, samples_per_pass=1)    # 6 passes of 1 spp instead of one of 6
    c2 = small.render(spp)
    assert (c2.bounce, c2.shadow, c2.primary_hits) == (c1.bounce, c1.shadow, c1.primary_hits)
    s2, q2, _ = small.film.pixel_datas()
    assert np.array_equal(bits(s2), bits(s1)) and np.array_equal(bits(q2), bits(q1))
    inc = make(pkg, scenes, "thai2", w, h, seed=1)                          # progressive: 2 + 4 spp == 6 spp
    inc.render(2); inc.render(4)
    assert np.array_equal(bits(inc.film.pixel_datas()[0]), bits(s1))
    ldr = rt.get_tonemapped_pixels()
    assert np.all(ldr >> 24 == 255) and 0.2 < (ldr != 0xFF000000).mean() < 0.4
    parts = np.zeros_like(s1); rows_seen = 0
    for rank in range(2):
        p = make(pkg, scenes, "thai2", w, h, seed=1, stripe_rows=8, stripe_rank=rank, stripe_world=2)
        p.render(spp)
        parts += p.film.pixel_datas()[0]; rows_seen += p.owned_rows().size
    assert rows_seen == h and np.array_equal(bits(parts), bits(s1))


def test_full_size_matches_oracle_on_sampled_rows(pkg, scenes, oracle, sem):
    """1080p frame (with the reference's idx / height row mapping active): rows picked across the image
    are bit-identical to the oracle rendering just those rows."""
    w, h, spp = 1920, 1080, 2
    rt = make(pkg, scenes, "thai2", w, h, seed=1, flags=sem.gpu)
    rt.render(spp)
    s, _, _ = rt.film.pixel_datas()
    orc = oracle.Oracle(scenes("thai2"), w, h, seed=1, flags=sem.orc)
    for r0 in (100, 539, 900):
        orc.render(spp, nthreads=16, rows=(r0, r0 + 1))
    os_, _, on = orc.film()
    m = on > 0
    assert m.sum() == 3 * w
    assert np.array_equal(bits(s[m]), bits(os_[m]))


# ---- reference-exact octree intersector (MI355RT_FLAG_OCTREE_SEMANTICS) ------------------------------------
@pytest.mark.parametrize("flag", ["default", "octree_walk"])
@pytest.mark.parametrize("name", ["4boxes", "ico2", "thai2", "ico3_tex"])
def test_reference_default_semantics_match_golden_fixtures(pkg, scenes, oracle, name, flag):
    """The reference's default intersector (OctTreeIntersector) on the device, two ways: the shipped default (BVH + octree
    confirm step) and the direct walk of the reference's octree (MI355RT_FLAG_OCTREE_SEMANTICS).  Hit records, film and
    pixels are bit-identical to the oracle in its default (octree) mode — including 4boxes, where the leaf-cube rule
    drops hits the true closest-hit search keeps."""
    g = np.load(os.path.join(GOLDEN, "render_%s.npz" % name))
    rt = make(pkg, scenes, name, 64, 64, seed=1, flags=pkg.FLAG_OCTREE_SEMANTICS if flag == "octree_walk" else 0)
    st = rt.octree_stats()
    assert [st["nodes"], st["inner"], st["leaves"], st["empty"], st["depth"], st["tri_refs"]] == [int(x) for x in g["octree_stats"]]
    tuv, prim = rt.intersect_rays(g["rays"])
    assert np.array_equal(prim, g["octree_prim"])
    m = prim != 0xFFFFFFFF
    assert np.array_equal(bits(tuv[m]), bits(g["octree_tuv"][m]))
    c = rt.render(4)
    s, q, n = rt.film.pixel_datas()
    assert [c.primary, c.bounce, c.shadow, c.primary_hits] == [int(x) for x in g["octree_counts"]]
    assert np.array_equal(bits(s), bits(g["octree_sum"])) and np.array_equal(bits(q), bits(g["octree_sumsq"]))
    assert np.array_equal(rt.get_tonemapped_pixels(), g["octree_ldr"])


def test_octree_mode_other_leaf_sizes_and_frames(pkg, scenes, oracle):
    """--max_triangles (tris per leaf) reaches the octree build; 50-row frames work in this mode too."""
    name, w, h = "ico2", 72, 60
    for tpl, flags in ((5, 0), (20, pkg.FLAG_OCTREE_SEMANTICS), (100, 0), (1, 0)):
        rt = make(pkg, scenes, name, w, h, seed=2, flags=flags, triangles_per_leaf=tpl)
        orc = oracle.Oracle(scenes(name), w, h, tris_per_leaf=tpl, seed=2)
        so = orc.octree_stats(); sg = rt.octree_stats()
        assert (sg["nodes"], sg["leaves"], sg["depth"], sg["tri_refs"]) == (so["nodes"], so["leaves"], so["depth"], so["tri_refs"])
        for _ in range(2):
            assert rt.trace_frame_additive() == orc.trace_frame_additive()
        assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(orc.film()[0]))
        assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())


def _image_delta(a, b):
    """(fraction of differing pixels, max per-channel u8 error, PSNR in dB over the RGB channels) of two 0xAARRGGBB frames"""
    ca = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], axis=1).astype(np.int32)
    cb = np.stack([(b >> 16) & 255, (b >> 8) & 255, b & 255], axis=1).astype(np.int32)
    diff = ca - cb
    mse = float((diff.astype(np.float64) ** 2).mean())
    psnr = float("inf") if mse == 0.0 else 10.0 * np.log10(255.0 ** 2 / mse)
    return float((a != b).mean()), int(np.abs(diff).max()), psnr


# measured on MI355X, 1920x1080 (profiles/r02_notes.md): what MI355RT_FLAG_TRUE_CLOSEST_HIT changes against the default
TOLERANCE_1080P = {          # name: (spp, max differing-pixel fraction, max u8 channel error, min PSNR dB)
    "ico2": (64, 0.0, 0, 99.0),              # BASELINE config 2 at its full 64 spp; measured: identical frames
    "4boxes": (256, 0.07, 60, 38.0),       # BASELINE config 3 at its full 256 spp, measured 0.0618 / 29 / 41.0 dB: box faces lie ON the root cube's bounds, the octree drops those hits
    "thai2": (64, 0.0, 0, 99.0),             # BASELINE config 4 (the headline) at its full 64 spp; measured: identical frames
}


@pytest.mark.parametrize("name", ["ico2", "4boxes", "thai2"])
def test_1080p_semantics_exactness_and_stated_tolerance(pkg, scenes, name):
    """BASELINE configs 2-4 at their full sizes (1920x1080, 64 / 256 / 64 spp).  (1) EXACTNESS of the shipped default: the BVH + octree confirm
    step and the direct walk of the reference's octree give bit-identical films and ray counters on full frames.
    (2) STATED TOLERANCE of the opt-out: what MI355RT_FLAG_TRUE_CLOSEST_HIT (NoAccelerationIntersector semantics) changes
    in the tonemapped frame — differing-pixel fraction, max per-channel u8 error, PSNR — within the bounds above."""
    w, h = 1920, 1080
    spp, max_frac, max_err, min_psnr = TOLERANCE_1080P[name]
    dflt = make(pkg, scenes, name, w, h, seed=1)
    cd = dflt.render(spp)
    sd, qd, nd = dflt.film.pixel_datas()
    ldr_d = dflt.get_tonemapped_pixels()
    del dflt                                                        # one handle's pass buffers at a time
    walk = make(pkg, scenes, name, w, h, seed=1, flags=pkg.FLAG_OCTREE_SEMANTICS)
    cw = walk.render(spp)
    assert (cd.primary, cd.bounce, cd.shadow, cd.primary_hits) == (cw.primary, cw.bounce, cw.shadow, cw.primary_hits)
    sw, qw, nw = walk.film.pixel_datas()
    assert np.array_equal(nd, nw) and np.array_equal(bits(sd), bits(sw)) and np.array_equal(bits(qd), bits(qw))
    assert np.array_equal(ldr_d, walk.get_tonemapped_pixels())
    del walk
    closest = make(pkg, scenes, name, w, h, seed=1, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    cc = closest.render(spp)
    frac, err, psnr = _image_delta(ldr_d, closest.get_tonemapped_pixels())
    print("\n[tolerance %s 1920x1080x%d] true-closest vs reference-default: differing pixels %.6f, max u8 channel error %d, PSNR %.2f dB; "
          "primary hits %d vs %d" % (name, spp, frac, err, psnr, cc.primary_hits, cd.primary_hits))
    assert frac <= max_frac and err <= max_err and psnr >= min_psnr
    assert cc.primary_hits >= cd.primary_hits                      # the octree only ever drops hits of primary rays' closest triangles


# ---- degenerate inputs ---------------------------------------------------------------------------------------
def _tiny_scene(scenes, ntri=None, nlights=None):
    sc = dict(scenes("4boxes"))
    if ntri is not None:
        sc["tri_verts"] = sc["tri_verts"][:ntri].copy(); sc["tri_geom"] = sc["tri_geom"][:ntri].copy()
    if nlights is not None:
        sc["lights"] = np.concatenate([sc["lights"]] * max(nlights, 1))[:nlights].copy()
        if nlights > 1:
            sc["lights"][1, :3] = [-3.0, 4.0, -2.0]; sc["lights"][1, 3:] = [2.0, 5.0, 8.0]
    return sc


@pytest.mark.parametrize("ntri,nlights", [(0, 1), (1, 1), (48, 0), (48, 2), (5, 3)])
def test_empty_single_triangle_and_multi_light_scenes(pkg, oracle, scenes, sem, ntri, nlights):
    """no triangles (every ray misses: black film), one triangle (the BVH is a single leaf), no light
    (every light term black), several lights (accum_color adds them in light order, mod.rs:214-256)."""
    sc = _tiny_scene(scenes, ntri, nlights)
    w, h = 48, 40
    rt = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=3, flags=sem.gpu)
    orc = oracle.Oracle(sc, w, h, seed=3, flags=sem.orc)
    c = rt.render(3); oc = orc.render(3, nthreads=4)
    assert (c.primary, c.bounce, c.shadow, c.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"])
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
    assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())
    if ntri == 0:
        assert c.primary_hits == 0 and not gs.any()
    if nlights == 0:
        assert c.shadow == 0 and not gs.any() and c.bounce > 0
    # the same through the direct octree walk
    rto = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=3, flags=pkg.FLAG_OCTREE_SEMANTICS)
    orco = oracle.Oracle(sc, w, h, seed=3)
    rto.render(2); orco.render(2, nthreads=4)
    assert np.array_equal(bits(rto.film.pixel_datas()[0]), bits(orco.film()[0]))


@pytest.mark.parametrize("name,nlights,rec", [("ico2", 2, 2), ("ico3_tex", 3, 1), ("thai2", 2, 2)])
def test_several_lights_on_multi_leaf_octrees(pkg, oracle, scenes, sem3, name, nlights, rec):
    """Several lights where the octree has many leaves, i.e. through the confirm kernel (the 48-triangle scenes above settle
    the octree inside the trace kernel): a shadow record holds only the hit point and the index of its light term, its ray is
    rebuilt from the light that index belongs to (term = 3 * ((node * nlights + light) * slots + slot)), and slot_L has one plane
    per (node, light).  Whole frames, 50-row frames (the fused kernel) and per-node terms against the oracle, bit for bit."""
    sc = dict(scenes(name))
    base = sc["lights"][0].copy()
    extra = np.array([[-3.0, 4.0, -2.0, 2.0, 5.0, 8.0], [6.0, -2.5, 3.0, 4.0, 1.0, 0.5]], np.float32)
    sc["lights"] = np.concatenate([base[None, :], extra[: nlights - 1]]).astype(np.float32)
    w, h = 96, 70
    rt = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=11, recursions=rec, flags=sem3.gpu)
    orc = oracle.Oracle(sc, w, h, seed=11, recursions=rec, flags=sem3.orc)
    c = rt.render(3); oc = orc.render(3, nthreads=4)
    assert (c.primary, c.bounce, c.shadow, c.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"])
    assert c.shadow > c.primary_hits                       # more than one shadow ray per shading point somewhere
    for _ in range(3):
        assert rt.trace_frame_additive() == orc.trace_frame_additive()
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
    assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())
    hit = 0
    for pixel in range(w * 10 + 5, w * h, 397):
        gc, gl = rt.debug_sample(pixel, 7); ocol, ol, ohit = orc.sample_debug(pixel, 7)
        assert np.array_equal(bits(gc), bits(ocol)) and np.array_equal(bits(gl), bits(ol)), pixel
        hit += int(ohit[0])
    assert hit > 0


def test_tiny_and_odd_image_sizes(pkg, oracle, scenes, sem):
    """1x1, 1xN, Nx1 and sizes that are not multiples of the chunk / stripe / wave sizes."""
    for w, h in ((1, 1), (1, 37), (37, 1), (257, 3), (33, 65)):
        rt = make(pkg, scenes, "ico2", w, h, seed=5, flags=sem.gpu)
        orc = oracle.Oracle(scenes("ico2"), w, h, seed=5, flags=sem.orc)
        rt.render(5); orc.render(5, nthreads=4)
        assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(orc.film()[0])), (w, h)
        assert rt.trace_frame_additive() == orc.trace_frame_additive() == 50 * w
        assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(orc.film()[0])), (w, h)


def test_images_of_fewer_pixels_than_a_chunk_with_the_object_at_the_edge(pkg, oracle, scenes, sem):
    """An image of fewer than 256 pixels: a chunk of primary samples runs past the end of the pixel order and wraps into the next sample index —
    possibly past its own first pixel, so that "last pixel >= first pixel" does not mean "a run of pixels".  The chunk culling once took such a chunk
    for the run between its first and last pixel and culled it when the object sat elsewhere in the image (found by the randomised soak with wild
    camera moves: the object at the right edge of a 24 x 8 image).  Cameras turned so that the object crosses every edge, several sample counts."""
    for w, h in ((24, 8), (15, 9), (12, 12), (31, 5)):
        for yaw, pitch in ((0.0, 0.0), (0.35, 0.0), (-0.35, 0.0), (0.5, 0.1), (-0.5, -0.1), (0.0, 0.3), (0.0, -0.3)):
            rt = make(pkg, scenes, "ico2", w, h, seed=9, flags=sem.gpu)
            orc = oracle.Oracle(scenes("ico2"), w, h, seed=9, flags=sem.orc)
            rt.camera.add_y_angle(yaw); orc.camera_add_y_angle(yaw); rt.camera.add_x_angle(pitch); orc.camera_add_x_angle(pitch)
            for spp in (1, 3, 33):
                c = rt.render(spp); oc = orc.render(spp, nthreads=4)
                assert (c.primary, c.bounce, c.shadow, c.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"]), (w, h, yaw, pitch, spp)
            for a, b in zip(rt.film.pixel_datas(), orc.film()):
                assert np.array_equal(bits(a) if a.dtype != np.uint32 else a, bits(b) if b.dtype != np.uint32 else b), (w, h, yaw, pitch)


def test_4k_frame_tiled_over_8_stripes_matches_oracle_on_sampled_rows(pkg, scenes, oracle, sem):
    """BASELINE config 5 in small: thai2 3840x2160 dealt to 8 ranks in stripes of 8 rows; two of the ranks
    are rendered (2 spp) and rows picked from their stripes are bit-identical to the oracle rendering just
    those rows; rows of other ranks stay untouched."""
    w, h, spp = 3840, 2160, 2
    orc = oracle.Oracle(scenes("thai2"), w, h, seed=1, flags=sem.orc)
    for rank, rows in ((3, (24, 1051)), (6, (1584, 2096))):
        rt = make(pkg, scenes, "thai2", w, h, seed=1, stripe_rows=8, stripe_rank=rank, stripe_world=8, flags=sem.gpu)
        c = rt.render(spp)
        owned = rt.owned_rows()
        assert owned.size == (272 if rank < 6 else 264) and np.all((owned // 8) % 8 == rank)    # 270 blocks of 8 rows over 8 ranks
        assert c.primary == owned.size * w * spp
        s_, _, n = rt.film.pixel_datas()
        n = n.reshape(h, w)
        assert np.all(n[owned] == spp) and n.sum() == owned.size * w * spp
        for r0 in rows:
            assert (r0 // 8) % 8 == rank
            orc.render(spp, nthreads=16, rows=(r0, r0 + 1))
            os_, _, _ = orc.film()
            assert np.array_equal(bits(s_).reshape(h, w, 3)[r0], bits(os_).reshape(h, w, 3)[r0])


def test_c5_one_rank_share_at_full_size(pkg, scenes, oracle):
    """BASELINE config 5 AT ITS SIZE, as far as one GPU goes: thai2 3840x2160 x 256 spp dealt to 8 ranks in the 2-row stripes
    bench.py deals; rank 5's share (270 rows, 265 M primary samples, ~550 M rays) is rendered twice.  Every owned pixel holds 256
    samples and no other pixel any; the ray counters obey the recursion's identities (RECURSIONS = 2 / SUB_SPREAD = 1: a level-0
    hit emits 2 reflection rays, a level-1 hit 1, every shaded hit at most one shadow ray); the two runs agree bit for bit; and
    three owned rows — one per third of the image — equal the oracle rendering just those rows at 256 spp."""
    w, h, spp, rank, world, sr = 3840, 2160, 256, 5, 8, 2
    rt = make(pkg, scenes, "thai2", w, h, seed=1, stripe_rows=sr, stripe_rank=rank, stripe_world=world)
    c = rt.render(spp)
    owned = rt.owned_rows()
    assert owned.size == 270 and np.all((owned // sr) % world == rank)
    assert c.primary == owned.size * w * spp == 265420800
    assert 0 < c.primary_hits <= c.primary - c.primary_culled
    assert 2 * c.primary_hits <= c.bounce <= 4 * c.primary_hits            # 2 per level-0 hit + 1 per level-1 hit (at most one per level-1 ray)
    assert 0 < c.shadow <= c.primary_hits + c.bounce                       # at most one per shaded hit of any level
    s1, q1, n1 = rt.film.pixel_datas()
    n = n1.reshape(h, w)
    assert np.all(n[owned] == spp) and int(n.sum(dtype=np.int64)) == owned.size * w * spp
    assert rt.hbm_allocated_bytes() < 80 * 2**30
    rt.film.clear()
    c2 = rt.render(spp)
    assert (c2.primary, c2.bounce, c2.shadow, c2.primary_hits, c2.primary_culled) == (c.primary, c.bounce, c.shadow, c.primary_hits, c.primary_culled)
    s2, q2, n2 = rt.film.pixel_datas()
    assert np.array_equal(n1, n2) and np.array_equal(bits(s1), bits(s2)) and np.array_equal(bits(q1), bits(q2))     # run to run
    del s2, q2, n2
    orc = oracle.Oracle(scenes("thai2"), w, h, seed=1)
    for r0 in (owned[20], owned[135], owned[250]):
        orc.render(spp, nthreads=16, rows=(int(r0), int(r0) + 1))
        os_, oq, on = orc.film()
        assert np.all(on.reshape(h, w)[r0] == spp)
        assert np.array_equal(bits(s1).reshape(h, w, 3)[r0], bits(os_).reshape(h, w, 3)[r0]), r0
        assert np.array_equal(bits(q1).reshape(h, w, 3)[r0], bits(oq).reshape(h, w, 3)[r0]), r0


@pytest.mark.parametrize("name", ["thai2", "ico2"])
def test_chunk_culling_stages_never_change_a_frame(pkg, scenes, monkeypatch, name):
    """The two stages of the primary-chunk culling (rectangles of the top BVH boxes; the coverage mask of the triangles' screen rectangles) only
    ever skip samples that miss: frames with both stages, with the first only (MI355RT_NO_CULL_MASK) and with none (MI355RT_NO_CULL) are
    bit-identical, the mask skips at least what the rectangles skip, and all of that still holds after the camera moved (the mask is rebuilt)
    and in a 50-row frame of the drop-in entry."""
    w, h, spp = 960, 540, 4
    films, culled = {}, {}
    for mode, env in (("mask", {}), ("rects", {"MI355RT_NO_CULL_MASK": "1"}), ("none", {"MI355RT_NO_CULL": "1"}), ("uncached", {"MI355RT_NO_CULL_CACHE": "1"})):
        for k in ("MI355RT_NO_CULL_MASK", "MI355RT_NO_CULL", "MI355RT_NO_CULL_CACHE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rt = make(pkg, scenes, name, w, h, seed=2)
        out = []
        c0 = rt.render(spp)
        out.append(rt.film.pixel_datas())
        rt.camera.move_rel(0.1, -0.1, 0.3); rt.camera.add_y_angle(0.07); rt.camera.add_x_angle(-0.03)
        rt.film.clear()
        c1 = rt.render(spp)
        out.append(rt.film.pixel_datas())
        rt.trace_frame_additive()
        out.append(rt.film.pixel_datas())
        c2 = rt.last_counts()
        films[mode] = out
        culled[mode] = (c0.primary_culled, c1.primary_culled, c2.primary_culled)
        assert (c0.primary, c1.primary) == (w * h * spp, w * h * spp)
        del rt
    assert culled["uncached"] == culled["mask"]               # the verdicts cached per pixel block are the verdicts every launch used to compute
    for mode in ("rects", "none", "uncached"):
        for a, b in zip(films["mask"], films[mode]):
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), mode
    assert culled["none"] == (0, 0, 0)
    for i in range(3):
        assert culled["mask"][i] >= culled["rects"][i]
    if name == "thai2":
        assert culled["mask"][0] > culled["rects"][0] > 0 and culled["mask"][1] > culled["rects"][1]


@pytest.mark.parametrize("name,light", [("thai2", None), ("thai2", (0.0, 0.0, 6.0)), ("thai2", (-1.5, -2.0, 3.0)), ("ico2", None), ("ico2", (0.05, 0.02, 0.01)),
                                        ("4boxes", None), ("4boxes", (1.0, 0.4, 1.0)), ("ico3_tex", (30.0, 40.0, -25.0))])
def test_light_depth_maps_never_change_a_frame(pkg, scenes, oracle, sem3, monkeypatch, name, light):
    """Shadow rays that the depth cube map around their light proves free are never made (shadow_skipped).  With the file's light, with lights
    in the middle of the geometry (the ray's 1 % tail behind the light matters there), inside a mesh, and far outside: film, pixels and every
    counter equal the run without maps (MI355RT_NO_LIGHT_MAP) bit for bit in all three intersector semantics, a second, re-coloured light
    included; and the default semantics equal the oracle."""
    sc = dict(scenes(name))
    if light is not None:
        sc["lights"] = sc["lights"].copy(); sc["lights"][0, :3] = light
    second = sc["lights"][0].copy(); second[:3] = second[:3][::-1] * np.float32(0.7); second[3:] = [0.5, 2.0, 1.0]
    sc["lights"] = np.concatenate([sc["lights"][:1], second[None, :]]).astype(np.float32)
    w, h, spp = 160, 120, 3
    runs = {}
    for mode in ("maps", "none"):
        monkeypatch.delenv("MI355RT_NO_LIGHT_MAP", raising=False)
        if mode == "none":
            monkeypatch.setenv("MI355RT_NO_LIGHT_MAP", "1")
        rt = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=4, flags=sem3.gpu)
        c = rt.render(spp)
        rt.camera.move_rel(0.2, 0.1, -0.3); rt.camera.add_y_angle(-0.05)
        for _ in range(3):
            rt.trace_frame_additive()
        c2 = rt.last_counts()
        runs[mode] = (rt.film.pixel_datas(), rt.get_tonemapped_pixels(), (c.primary, c.bounce, c.shadow, c.primary_hits), (c2.bounce, c2.shadow), c.shadow_skipped + c2.shadow_skipped)
        del rt
    (fa, pa, ca, c2a, skipped), (fb, pb, cb, c2b, none_skipped) = runs["maps"], runs["none"]
    assert ca == cb and c2a == c2b and none_skipped == 0
    assert np.array_equal(pa, pb)
    for x, y in zip(fa, fb):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert 0 <= skipped <= ca[2] + c2a[1]
    if light is None or name == "ico3_tex":
        assert skipped > 0                                     # an outside light: most lit points are proved free
    if sem3.orc is not None and name != "thai2":
        orc = oracle.Oracle(sc, w, h, seed=4, flags=sem3.orc)
        oc = orc.render(spp, nthreads=8)
        assert ca == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"])


@pytest.mark.parametrize("name,w,h,stripe", [("thai2", 960, 544, None), ("thai2", 640, 360, (2, 1, 3)), ("ico2", 512, 256, None), ("4boxes", 320, 240, (4, 0, 2)),
                                              ("ico3_tex", 256, 256, None), ("thai2", 322, 250, None)])
def test_primary_rays_through_the_tile_bins_equal_the_tree_walk(pkg, scenes, sem, monkeypatch, name, w, h, stripe):
    """The primary rays' closest hits come from the screen-space triangle bins (raster_kernel) when the pass layout allows it, from the BVH walk
    otherwise (MI355RT_NO_RASTER; odd widths / heights like 322 x 250 whose tiles would straddle row groups).  Both give the same film, pixels and
    counters — whole images and row stripes, both shipped semantics, with and without the row-index quirk, before and after camera moves (the bins
    are rebuilt) and with several passes per frame."""
    kw = {}
    if stripe is not None:
        kw = dict(stripe_rows=stripe[0], stripe_rank=stripe[1], stripe_world=stripe[2])
    runs = {}
    for mode in ("bins", "walk"):
        monkeypatch.delenv("MI355RT_NO_RASTER", raising=False)
        if mode == "walk":
            monkeypatch.setenv("MI355RT_NO_RASTER", "1")
        rt = make(pkg, scenes, name, w, h, seed=6, flags=sem.gpu, samples_per_pass=2, **kw)
        out = []
        rt.set_flags(sem.gpu | pkg.FLAG_COUNT_STEPS)
        nodes = rt.render(2).nodes_visited                      # instrumented: the bins take the primary rays' node visits away
        rt.set_flags(sem.gpu); rt.film.clear()
        c = rt.render(5)                                        # 3 passes (2 + 2 + 1 samples per pixel)
        out.append((rt.film.pixel_datas(), (c.primary, c.bounce, c.shadow, c.primary_hits, c.primary_culled)))
        rt.camera.move_rel(-0.3, 0.2, 0.5); rt.camera.add_x_angle(0.04); rt.camera.add_y_angle(0.11)
        rt.film.clear()
        c = rt.render(2)
        out.append((rt.film.pixel_datas(), (c.primary, c.bounce, c.shadow, c.primary_hits, c.primary_culled)))
        rt.set_flags(sem.gpu | pkg.FLAG_FIX_ROW_INDEX)
        c = rt.render(2)
        out.append((rt.film.pixel_datas(), (c.primary, c.bounce, c.shadow, c.primary_hits, c.primary_culled)))
        out.append(rt.get_tonemapped_pixels())
        out.append(nodes)
        runs[mode] = out
        del rt
    if (name, w) == ("thai2", 960):
        assert runs["bins"][4] < runs["walk"][4]               # the bins were in use
    elif w % 4 or h % 8:
        assert runs["bins"][4] == runs["walk"][4]              # tiles would straddle row groups: both runs walked the tree
    else:
        assert runs["bins"][4] <= runs["walk"][4]
    for a, b in zip(runs["bins"][:3], runs["walk"][:3]):
        assert a[1] == b[1]
        for x, y in zip(a[0], b[0]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(runs["bins"][3], runs["walk"][3])
    assert runs["bins"][0][1][3] > 0                            # something was hit


def _random_scene(scenes, ntri, seed):
    """ntri small random triangles in a slab in front of the 4boxes camera (materials / light from 4boxes)."""
    rng = np.random.default_rng(seed)
    sc = dict(scenes("4boxes"))
    lo, hi = sc["tri_verts"].reshape(-1, 3).min(0), sc["tri_verts"].reshape(-1, 3).max(0)
    centre = rng.uniform(lo, hi, size=(ntri, 1, 3))
    # strongly non-uniform: half of the triangles crowd into 2 % of the volume, so the SAH tree gets deep
    crowd = rng.random(ntri) < 0.5
    centre[crowd] = lo + (hi - lo) * (0.49 + 0.02 * rng.random((int(crowd.sum()), 1, 3)))
    size = np.where(crowd, 0.002, 0.05)[:, None, None] * (hi - lo).max()
    sc["tri_verts"] = (centre + rng.uniform(-1.0, 1.0, size=(ntri, 3, 3)) * size).astype(np.float32).reshape(ntri, 9)
    sc["tri_geom"] = rng.integers(0, len(sc["mat_kind"]), size=ntri).astype(np.uint32)
    return sc


def test_large_random_scene_deep_tree(pkg, scenes, oracle, sem):
    """120 000 random triangles, half of them crowded into a tiny volume: a deep, unbalanced BVH (more stack
    rows than 8 blocks per CU leave room for).  Closest hits of random rays and a small rendered frame are
    bit-identical to the brute-force oracle."""
    sc = _random_scene(scenes, 120000, 7)
    w, h, spp = 40, 24, 2
    rt = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=11, flags=sem.gpu)
    st = rt.accel_stats()
    assert st["max_depth"] > 18 and st["max_leaf"] <= 4 and st["leaves"] >= 30000
    rng = np.random.default_rng(3)
    n = 6000
    lo, hi = sc["tri_verts"].reshape(-1, 3).min(0), sc["tri_verts"].reshape(-1, 3).max(0)
    rays = np.empty((n, 6), np.float32)
    rays[:, :3] = rng.uniform(lo - 1.0, hi + 1.0, size=(n, 3))
    tgt = rng.uniform(lo, hi, size=(n, 3)); tgt[::2] = lo + (hi - lo) * (0.49 + 0.02 * rng.random((n // 2, 3)))
    rays[:, 3:] = tgt - rays[:, :3]
    tuv, prim = rt.intersect_rays(rays)
    otuv, oprim = oracle.Oracle(sc, w, h, seed=11, flags=sem.orc).intersect(rays, brute=bool(sem.orc & oracle.FLAG_BRUTE_FORCE), nthreads=16)
    assert np.array_equal(prim, oprim) and (prim != 0xFFFFFFFF).mean() > 0.3
    hit = prim != 0xFFFFFFFF
    assert np.array_equal(bits(tuv[hit]), bits(otuv[hit]))
    orc = oracle.Oracle(sc, w, h, seed=11, flags=sem.orc)
    c = rt.render(spp); oc = orc.render(spp, nthreads=16)
    assert (c.primary, c.bounce, c.shadow, c.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"])
    assert c.primary_hits > 0
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))


def test_headless_cli_renders_the_library_frame(pkg, scenes, tmp_path):
    """bin/raytracer (the reference's `raytracer` binary without the window): same flags, the
    `fps: ... primary rays/s: ...` lines, and the PPM it writes holds exactly the pixels the library returns
    for the same seed — both in the reference's 50-row progressive mode and with --spp."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "raytracer-rs_amd", "bin", "raytracer")
    scene = os.path.join(GOLDEN, "scenes", "ico2.scene")
    w, h = 96, 70
    for extra, frames in ((["-i", "2"], None), (["--spp", "3"], 3), (["--spp", "3", "--device-lbvh"], 3)):     # the device-built BVH: same picture
        out = str(tmp_path / "o.ppm")
        r = subprocess.run([exe, "-f", scene, "--width", str(w), "--height", str(h), "--seed", "4", "--out", out] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "number of triangles: 608" in r.stdout and "max triangles per leaf: 70" in r.stdout
        assert len(re.findall(r"fps: [0-9.]+ +primary rays/s: ", r.stdout)) >= (2 if frames is None else 1)
        assert "mean fps" in r.stdout or "mean" in r.stdout
        rt = make(pkg, scenes, "ico2", w, h, seed=4)
        if frames is None:
            rt.trace_frame_additive(); rt.trace_frame_additive()
        else:
            rt.render(frames)
        ldr = rt.get_tonemapped_pixels()
        data = open(out, "rb").read()
        header = ("P6\n%d %d\n255\n" % (w, h)).encode()
        assert data.startswith(header) and len(data) == len(header) + 3 * w * h
        rgb = np.frombuffer(data[len(header):], np.uint8).reshape(-1, 3).astype(np.uint32)
        assert np.array_equal((rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2], ldr & 0xFFFFFF)
    bad = subprocess.run([exe, "-f", str(tmp_path / "missing.dae")], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and bad.stderr.startswith("Error: ")


@pytest.mark.parametrize("name,spp", [("ico2", 64), ("4boxes", 256), ("thai2", 64)])
def test_baseline_configs_at_full_size(pkg, scenes, name, spp):
    """BASELINE configs 2-4 at their full sizes (1920x1080, 64 / 256 / 64 spp), through properties that do
    not need the oracle: every pixel holds spp samples, the ray counters obey the radiance tree (2 reflection
    rays per primary hit, one per hit after that; at most one shadow ray per shading point and light), the
    frame is bit-identical run to run, for another slice count, and when it is split into two progressive
    halves; variance estimates are finite and the packed pixels are opaque."""
    w, h = 1920, 1080
    rt = make(pkg, scenes, name, w, h, seed=1)
    c = rt.render(spp)
    s1, q1, n1 = rt.film.pixel_datas()
    assert np.all(n1 == spp) and c.primary == w * h * spp
    lvl1 = 2 * c.primary_hits
    assert lvl1 <= c.bounce <= lvl1 + lvl1                         # level-2 rays: one per level-1 hit
    assert c.shadow <= (c.primary_hits + c.bounce) * len(scenes(name)["lights"])
    assert np.isfinite(s1).all() and np.isfinite(q1).all() and (s1 >= 0).all()
    var = rt.film.get_estimated_variances()
    assert np.isfinite(var).all() and (var >= -1e-3).all()
    ldr = rt.get_tonemapped_pixels()
    assert np.all(ldr >> 24 == 255)
    other = make(pkg, scenes, name, w, h, seed=1)
    other.set_slices(1 if rt.get_slices() != 1 else 2)
    other.render(spp // 2); other.render(spp - spp // 2)
    s2, q2, n2 = other.film.pixel_datas()
    assert np.array_equal(n2, n1) and np.array_equal(bits(s2), bits(s1)) and np.array_equal(bits(q2), bits(q1))
    rt.film.clear(); c2 = rt.render(spp)
    assert (c2.bounce, c2.shadow, c2.primary_hits) == (c.bounce, c.shadow, c.primary_hits)
    assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(s1))


def test_build_times_are_reported(pkg, scenes):
    """mi355rt_accel_stats reports the host build times inside mi355rt_create: the binned-SAH BVH and the reference's
    octree (SAT).  The API never rebuilds (the scene is fixed at create; camera moves only clear the film), so these are
    one-off costs: DESIGN.md section 8 quotes the numbers this test prints."""
    for name, sc in (("thai2", scenes("thai2")), ("random 120 000 triangles", _random_scene(scenes, 120000, 7))):
        rt = pkg.create_raytracer_from_arrays(sc, 70, 64, 64, seed=1)
        st = rt.accel_stats(); oc = rt.octree_stats()
        print("\n[build %s] BVH %.1f ms (%d nodes, depth %d), octree %.1f ms (%d nodes, depth %d, %d triangle references)" % (
            name, st["bvh_build_ms"], st["nodes"], st["max_depth"], st["octree_build_ms"], oc["nodes"], oc["depth"], oc["tri_refs"]))
        assert 0.0 < st["bvh_build_ms"] < 5000.0 and 0.0 < st["octree_build_ms"] < 60000.0
        fast = pkg.create_raytracer_from_arrays(sc, 70, 64, 64, seed=1, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
        assert fast.accel_stats()["octree_build_ms"] == 0.0 and fast.octree_stats()["nodes"] == 0


def _adversarial_rays(sc, rng, n):
    """Rays aimed at the places where the octree semantics are NOT the true closest hit and where the confirm step leaves
    its fast path: origins and hit points ON the octree's grid planes (root bounds, mid planes of the first four levels),
    axis-parallel and in-plane directions (inf / NaN in the inverse direction), rays through cube corners and along cube
    edges, rays starting on triangle vertices, plus ordinary random rays."""
    v = sc["tri_verts"].reshape(-1, 3).astype(np.float32)
    lo, hi = v.min(0), v.max(0)
    grid = [np.unique(np.concatenate([np.linspace(lo[a], hi[a], 2 ** k + 1, dtype=np.float32) for k in range(5)])) for a in range(3)]
    def on_grid(m):
        p = rng.uniform(lo, hi, (m, 3)).astype(np.float32)
        for a in range(3):
            sel = rng.random(m) < 0.6
            p[sel, a] = rng.choice(grid[a], int(sel.sum()))
        return p
    parts = []
    m = n // 6
    o = on_grid(m); t = on_grid(m); parts.append(np.concatenate([o, t - o], 1))                       # grid point -> grid point
    o = on_grid(m); d = np.zeros((m, 3), np.float32); ax = rng.integers(0, 3, m); d[np.arange(m), ax] = rng.choice([-1.0, 1.0], m); parts.append(np.concatenate([o - 20 * d * (rng.random((m, 1)) < 0.5), d], 1))   # axis-parallel
    o = on_grid(m); d = rng.normal(size=(m, 3)).astype(np.float32); d[np.arange(m), rng.integers(0, 3, m)] = 0.0; parts.append(np.concatenate([o, d], 1))   # in-plane
    tv = v[rng.integers(0, len(v), m)]; o = rng.uniform(lo - 3, hi + 3, (m, 3)).astype(np.float32); parts.append(np.concatenate([o, tv - o], 1))          # through triangle vertices
    tv = v[rng.integers(0, len(v), m)]; d = rng.normal(size=(m, 3)).astype(np.float32); parts.append(np.concatenate([tv, d], 1))                           # starting on vertices
    o = rng.uniform(lo - 3, hi + 3, (n - 5 * m, 3)).astype(np.float32); t = rng.uniform(lo, hi, (n - 5 * m, 3)).astype(np.float32); parts.append(np.concatenate([o, t - o], 1))
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.parametrize("name,tpl", [("4boxes", 70), ("4boxes", 5), ("ico2", 70), ("ico2", 1), ("thai2", 70), ("thai2", 8)])
def test_confirm_step_equals_direct_octree_walk_on_adversarial_rays(pkg, scenes, name, tpl):
    """The shipped default (BVH + octree confirm step) against the direct walk of the reference's octree, on the device, for
    300 000 rays built to sit on the octree's grid planes, corners and edges and on triangle vertices: identical hit records
    (triangle, t, u, v bit for bit) and identical shadow predicates.  (Both against the oracle: the parametrised seam tests.)"""
    sc = scenes(name)
    rng = np.random.default_rng(12345 + tpl)
    rays = _adversarial_rays(sc, rng, 300000)
    a = make(pkg, scenes, name, 32, 32, triangles_per_leaf=tpl)
    b = make(pkg, scenes, name, 32, 32, triangles_per_leaf=tpl, flags=pkg.FLAG_OCTREE_SEMANTICS)
    ta, pa = a.intersect_rays(rays); tb, pb = b.intersect_rays(rays)
    assert np.array_equal(pa, pb), "hit triangles differ for %d rays" % int((pa != pb).sum())
    m = pa != 0xFFFFFFFF
    assert m.sum() > 20000 and np.array_equal(bits(ta[m]), bits(tb[m]))
    assert np.array_equal(a.occluded_rays(rays), b.occluded_rays(rays))
    # and the true closest hit differs from both somewhere (otherwise this test would not exercise the semantics)
    c = make(pkg, scenes, name, 32, 32, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    _, pc = c.intersect_rays(rays)
    print("\n[adversarial %s, %d per leaf] rays whose octree answer is not the true closest hit: %d of %d" % (name, tpl, int((pc != pa).sum()), len(rays)))
    assert (pc != pa).sum() > 0


def test_randomised_configurations_match_oracle(pkg, scenes, oracle):
    """24 random configurations — scene, image size, seed, camera pose, samples, recursion / spread, octree leaf size,
    semantics, stripes, row-index fix, whole frames mixed with 50-row frames — each compared with the oracle bit for bit
    (film sums, sums of squares, counts, packed pixels).  A fixed generator seed keeps the test reproducible."""
    rng = np.random.default_rng(int(os.environ.get("MI355RT_TEST_RANDOM_SEED", "20261004")))
    names = ["4boxes", "ico2", "ico3_tex", "thai2"]
    for case in range(int(os.environ.get("MI355RT_TEST_RANDOM_CASES", "24"))):      # soak runs: more cases, other seeds
        name = names[int(rng.integers(0, 4))]
        w, h = int(rng.integers(17, 140)), int(rng.integers(9, 110))
        seed = int(rng.integers(1, 1 << 30))
        rec, spread = [(2, 1), (2, 1), (1, 1), (0, 1), (1, 2), (3, 1)][int(rng.integers(0, 6))]
        tpl = int(rng.choice([1, 3, 10, 70, 200]))
        closest = bool(rng.integers(0, 3) == 0)
        fix = bool(rng.integers(0, 2))
        world = int(rng.choice([1, 1, 2, 3])); rank = int(rng.integers(0, world)); srows = int(rng.choice([1, 4, 8]))
        lbvh = bool(rng.integers(0, 4) == 0)
        gflags = (pkg.FLAG_TRUE_CLOSEST_HIT if closest else 0) | (pkg.FLAG_FIX_ROW_INDEX if fix else 0) | (pkg.FLAG_DEVICE_LBVH if lbvh else 0)
        oflags = (oracle.FLAG_BRUTE_FORCE if closest else 0) | (oracle.FLAG_FIX_ROW_INDEX if fix else 0)
        rt = pkg.create_raytracer_from_arrays(scenes(name), tpl, w, h, seed=seed, recursions=rec, spread=spread, flags=gflags,
                                              stripe_rows=srows, stripe_rank=rank, stripe_world=world)
        orc = oracle.Oracle(scenes(name), w, h, tris_per_leaf=tpl, recursions=rec, spread=spread, seed=seed, flags=oflags)
        for _ in range(int(rng.integers(0, 4))):
            mv = rng.uniform(-0.3, 0.3, 3).astype(np.float32); ax, ay = np.float32(rng.uniform(-0.1, 0.1)), np.float32(rng.uniform(-0.1, 0.1))
            rt.camera.move_rel(float(mv[0]), float(mv[1]), float(mv[2])); orc.camera_move_rel(float(mv[0]), float(mv[1]), float(mv[2]))
            rt.camera.add_x_angle(float(ax)); orc.camera_add_x_angle(float(ax))
            rt.camera.add_y_angle(float(ay)); orc.camera_add_y_angle(float(ay))
        rows = rt.owned_rows()
        desc = (case, name, w, h, seed, rec, spread, tpl, closest, fix, world, rank, srows, lbvh)
        for step in range(int(rng.integers(1, 4))):
            if world == 1 and rng.integers(0, 2) == 0:
                assert rt.trace_frame_additive() == orc.trace_frame_additive(), desc      # the oracle has no stripes: frames only on whole handles
            else:
                spp = int(rng.integers(1, 4))
                rt.render(spp)
                for r0 in rows:                                                          # the oracle renders exactly the owned rows
                    orc.render(spp, nthreads=1, rows=(int(r0), int(r0) + 1))
        gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
        m = np.zeros(h, bool); m[rows] = True; m = np.repeat(m, w)
        assert np.array_equal(gn[m], on[m]), desc
        assert np.array_equal(bits(gs[m]), bits(os_[m])) and np.array_equal(bits(gq[m]), bits(oq[m])), desc
        assert np.array_equal(rt.get_tonemapped_pixels()[m], orc.get_tonemapped_pixels()[m]), desc


# ---- device LBVH (MI355RT_FLAG_DEVICE_LBVH): a different tree, the same results ---------------------------------
@pytest.mark.parametrize("name", ["ico2", "ico3_tex", "thai2"])
def test_device_lbvh_gives_the_same_results(pkg, scenes, oracle, sem, name):
    """The BVH built on the device (Morton order, Karras hierarchy, refit: csrc/lbvh.hip) instead of the host's SAH build:
    closest hits against the brute-force oracle on 40 000 rays, whole frames + 50-row frames against the oracle bit for bit
    in both semantics, and the builder reports that it ran on the device."""
    sc = scenes(name)
    w, h = 80, 64
    rt = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=5, flags=sem.gpu | pkg.FLAG_DEVICE_LBVH)
    info = rt.bvh_build_info(); st = rt.accel_stats()
    assert info["on_device"] and info["device_ms"] > 0.0 and st["max_depth"] <= 31 and st["max_leaf"] == 1
    print("\n[%s] device LBVH: %d nodes, %d leaves, depth %d, device %.3f ms, wall %.3f ms" % (name, st["nodes"], st["leaves"], st["max_depth"], info["device_ms"], st["bvh_build_ms"]))
    host = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=5, flags=sem.gpu)
    assert not host.bvh_build_info()["on_device"]
    rng = np.random.default_rng(3)
    v = np.asarray(sc["tri_verts"], np.float32).reshape(-1, 3); lo, hi = v.min(0), v.max(0)
    org = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (40000, 3)); tgt = rng.uniform(lo, hi, (40000, 3))
    rays = np.concatenate([org, tgt - org], axis=1).astype(np.float32)
    g_tuv, g_prim = rt.intersect_rays(rays); h_tuv, h_prim = host.intersect_rays(rays)
    assert np.array_equal(g_prim, h_prim) and np.array_equal(bits(g_tuv[g_prim != 0xFFFFFFFF]), bits(h_tuv[h_prim != 0xFFFFFFFF]))
    orc = oracle.Oracle(sc, w, h, seed=5, flags=sem.orc)
    c = rt.render(3); oc = orc.render(3, nthreads=4)
    assert (c.primary, c.bounce, c.shadow, c.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"])
    for _ in range(2):
        assert rt.trace_frame_additive() == orc.trace_frame_additive()
    gs, gq, gn = rt.film.pixel_datas(); os_, oq, on = orc.film()
    assert np.array_equal(gn, on) and np.array_equal(bits(gs), bits(os_)) and np.array_equal(bits(gq), bits(oq))
    assert np.array_equal(rt.get_tonemapped_pixels(), orc.get_tonemapped_pixels())


def test_device_lbvh_falls_back_on_one_leaf_scenes_and_builds_large_ones(pkg, scenes, oracle):
    """A 3-triangle scene fits one leaf: the host build serves it (create succeeds, the flag is a request).  4boxes (48 triangles)
    and the 120 000-triangle random scene are built on the device; closest hits and a frame equal the host tree's."""
    sc = dict(scenes("4boxes")); sc["tri_verts"] = sc["tri_verts"][:3].copy(); sc["tri_geom"] = sc["tri_geom"][:3].copy()
    rt = pkg.create_raytracer_from_arrays(sc, 70, 32, 32, seed=1, flags=pkg.FLAG_DEVICE_LBVH)
    assert not rt.bvh_build_info()["on_device"]
    orc = oracle.Oracle(sc, 32, 32, seed=1)
    rt.render(2); orc.render(2, nthreads=2)
    assert np.array_equal(bits(rt.film.pixel_datas()[0]), bits(orc.film()[0]))
    rt4 = pkg.create_raytracer_from_arrays(scenes("4boxes"), 70, 32, 32, seed=1, flags=pkg.FLAG_DEVICE_LBVH)
    assert rt4.bvh_build_info()["on_device"]
    # 120 000 small triangles spread evenly: built on the device.  The crowded scene of test_large_random_scene_deep_tree gives a
    # Morton-order tree deeper than the traversal stack (31 levels): the host build serves it, results as ever.  (Which way the crowded scene goes is
    # not asserted here; the limit itself is pinned from both sides in tests/test_gpu_lbvh_statement.py: height 31 on the device, height 32 refused.)
    rng = np.random.default_rng(7)
    big = dict(scenes("4boxes"))
    lo, hi = big["tri_verts"].reshape(-1, 3).min(0), big["tri_verts"].reshape(-1, 3).max(0)
    centre = rng.uniform(lo, hi, size=(120000, 1, 3))
    big["tri_verts"] = (centre + rng.uniform(-1.0, 1.0, size=(120000, 3, 3)) * 0.01 * (hi - lo).max()).astype(np.float32).reshape(120000, 9)
    big["tri_geom"] = rng.integers(0, len(big["mat_kind"]), size=120000).astype(np.uint32)
    for label, sc_big, expect_device in (("even", big, True), ("crowded", _random_scene(scenes, 120000, 7), None)):
        dev = pkg.create_raytracer_from_arrays(sc_big, 70, 64, 64, seed=2, flags=pkg.FLAG_TRUE_CLOSEST_HIT | pkg.FLAG_DEVICE_LBVH)
        host = pkg.create_raytracer_from_arrays(sc_big, 70, 64, 64, seed=2, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
        di, ds, hs = dev.bvh_build_info(), dev.accel_stats(), host.accel_stats()
        if expect_device is not None:
            assert di["on_device"] == expect_device
        print("\n[120k triangles, %s] device LBVH requested: on device %s, device %.2f ms, wall %.2f ms, %d nodes, depth %d | host SAH: %.1f ms, %d nodes, depth %d"
              % (label, di["on_device"], di["device_ms"], ds["bvh_build_ms"], ds["nodes"], ds["max_depth"], hs["bvh_build_ms"], hs["nodes"], hs["max_depth"]))
        v = np.asarray(sc_big["tri_verts"], np.float32).reshape(-1, 3); lo_, hi_ = v.min(0), v.max(0)
        org = rng.uniform(lo_, hi_, (60000, 3)); tgt = rng.uniform(lo_, hi_, (60000, 3))
        rays = np.concatenate([org, tgt - org], axis=1).astype(np.float32)
        d_tuv, d_prim = dev.intersect_rays(rays); h_tuv, h_prim = host.intersect_rays(rays)
        assert np.array_equal(d_prim, h_prim) and np.array_equal(bits(d_tuv[d_prim != 0xFFFFFFFF]), bits(h_tuv[h_prim != 0xFFFFFFFF]))
        dev.render(1); host.render(1)
        assert np.array_equal(bits(dev.film.pixel_datas()[0]), bits(host.film.pixel_datas()[0]))


def test_bvh_optimisation_changes_the_tree_not_the_answers(pkg, scenes, oracle, monkeypatch):
    """The host BVH is post-optimised by subtree re-insertion (csrc/bvh.cpp, MI355RT_BVH_OPT passes).  Any conservative tree gives the
    same hits: closest hits of random rays and a rendered film are identical with 0 and with 4 passes (and equal to the oracle), the
    optimised tree holds the same triangles in no more nodes and is no deeper."""
    rng = np.random.default_rng(5)
    sc = scenes("thai2")
    lo, hi = sc["tri_verts"].reshape(-1, 3).min(0), sc["tri_verts"].reshape(-1, 3).max(0)
    o = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), size=(20000, 3)).astype(np.float32)
    d = (rng.uniform(lo, hi, size=(20000, 3)) - o).astype(np.float32)
    rays = np.concatenate([o, d], axis=1)
    res = {}
    for passes in ("0", "4"):
        monkeypatch.setenv("MI355RT_BVH_OPT", passes)
        rt = make(pkg, scenes, "thai2", 96, 64, seed=2, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
        st = rt.accel_stats()
        tuv, prim = rt.intersect_rays(rays)
        c = rt.render(2)
        res[passes] = (st, prim.copy(), bits(tuv).copy(), bits(rt.film.pixel_datas()[0]).copy(), (c.primary, c.bounce, c.shadow))
    (s0, p0, t0, f0, c0), (s4, p4, t4, f4, c4) = res["0"], res["4"]
    assert s4["nodes"] == s0["nodes"] and s4["leaves"] == s0["leaves"] and s4["max_depth"] <= s0["max_depth"]
    assert (p0 != 0xFFFFFFFF).mean() > 0.2
    hit = p0 != 0xFFFFFFFF
    assert np.array_equal(p0, p4) and np.array_equal(t0[hit], t4[hit]) and np.array_equal(f0, f4) and c0 == c4
    orc = oracle.Oracle(sc, 96, 64, seed=2, flags=oracle.FLAG_BRUTE_FORCE)
    orc.render(2, nthreads=8)
    assert np.array_equal(f4, bits(orc.film()[0]))


def test_randomised_call_sequences_match_the_oracle(pkg, scenes, oracle):
    """tools/parity_fuzz.py, 30 cases of a fixed seed: random scene, size, RNG seed, recursion setting, leaf size, semantics, stripes,
    camera moves and sequences of render / trace_frame_additive / film.clear — films, pixels and counters bit-equal to the oracle.
    (profiles/r03_notes.md records a 1 000-case run.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("parity_fuzz", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "parity_fuzz.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    rng = np.random.default_rng(3)
    for _ in range(30):
        fuzz.one_case(pkg, oracle, scenes, rng, verbose=False)


@pytest.mark.parametrize("modes", [("FUZZ_SPP", "FUZZ_SOUP"), ("FUZZ_BUILD", "FUZZ_SOUP"), ("FUZZ_WILD", "FUZZ_SPP", "FUZZ_SOUP", "FUZZ_BUILD"), ("FUZZ_GRAZE", "FUZZ_SOUP")],
                         ids=lambda m: "+".join(x[5:].lower() for x in m))
def test_randomised_cases_of_the_wider_fuzz_modes(pkg, scenes, oracle, monkeypatch, modes):
    """The fuzz tool's other dimensions, 25 cases each of a fixed seed: many samples per pixel in passes of odd sample counts, random triangle soups
    (slivers, degenerate, duplicate, axis-parallel, far-reaching triangles), the device-built tree, device groups sharing the GPU, wild camera
    moves (the eye inside or behind the geometry), wild moves that end within 1e-1 ... 1e-6 of the scene's extent of the pose where the scene's ROOT box
    stops lying wholly in front of the eye (FUZZ_GRAZE).  The library tests its 16 sub-boxes, which hug the geometry: its own switch can lie further along
    the dolly axis, and a case grazes it only where a sub-box shares the root box's extreme corner.  Measured once from the library's report
    on these 25 cases: 21 render with the structures in use, their widest cull rectangle between 2.9 and 164 screen units (an ordinary view: 0.4 to 0.8)
    and 5 792 in one case — closer to the switch than any other fuzz mode gets, at the library's switch itself once.  tests/test_gpu_poses.py bisects on the
    library's own report instead.  (profiles/r03_notes.md records 1 800 cases
    of the first four modes.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("parity_fuzz", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "parity_fuzz.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    for m in ("FUZZ_WILD", "FUZZ_SPP", "FUZZ_SOUP", "FUZZ_BUILD", "FUZZ_GRAZE"):
        monkeypatch.delenv(m, raising=False)
    for m in modes:
        monkeypatch.setenv(m, "1")
    rng = np.random.default_rng(31 + len(modes))
    for _ in range(25):
        fuzz.one_case(pkg, oracle, scenes, rng, verbose=False)
