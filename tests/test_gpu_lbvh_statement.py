"""The BVH the device builds (csrc/lbvh.hip, MI355RT_FLAG_DEVICE_LBVH) held to its numpy statement, node for node.

oracle/bvh_statement.py states the tree exactly: keys, stable order, Karras' hierarchy and numbering, exact boxes, outward rounded
halves, the triangle words.  The handle's tree is read out (RayTracer.bvh_read) and compared word for word; check_tree, which
shares nothing with the statement's build, walks the same arrays so that "other bits" can be told from "an invalid tree".  The
cases, their rays and the two chain scenes of the depth limit come from tests/test_bvh_statement.py, where they are checked on the
CPU; the statement's trees are built once per case and shared."""
import numpy as np
import pytest

from test_bvh_statement import (CASE_NAMES, MISS, N_RAYS, bits, brute_oracle, case_rays, case_scene, case_triangles, chain_of_height, chain_rays,
                                deepest_triangles, scene_with, statement, statement_tree)

pytestmark = pytest.mark.gpu


def lbvh_flags(pkg):
    return pkg.FLAG_TRUE_CLOSEST_HIT | pkg.FLAG_DEVICE_LBVH


def assert_equals_statement(read, tree, verts, geom, label):
    """the read-out against the statement: order, triangle words, all eight node words, the scalars; then check_tree on the device's arrays"""
    S = statement()
    facts = None
    try:
        facts = S.check_tree(read["nodes"], read["tris"], verts, geom, root=read["root"], leaves=read["leaves"], max_leaf=read["max_leaf"])
        valid = "check_tree accepts the device's tree (%r)" % (facts,)
    except AssertionError as e:
        valid = "check_tree REFUSES the device's tree: %s" % e
    assert read["tris"].shape == tree["tris"].shape, "%s: %d triangle slots, statement %d; %s" % (label, read["tris"].shape[0], tree["tris"].shape[0], valid)
    bad = np.nonzero(read["tris"][:, 3] != tree["order"])[0]
    assert bad.size == 0, "%s: order differs at %d positions, first %d: device triangle %d, statement %d; %s" % (
        label, bad.size, bad[0], read["tris"][bad[0], 3], tree["order"][bad[0]], valid)
    assert np.array_equal(read["tris"], tree["tris"]), "%s: triangle words differ; %s" % (label, valid)
    diff = S.first_difference(read["nodes"], tree["nodes"])
    assert diff is None, "%s: %s; %s" % (label, diff, valid)
    assert (read["root"], read["leaves"], read["max_depth"], read["max_leaf"]) == (0, tree["leaves"], tree["max_depth"], 1), (label, valid)
    assert np.array_equal(bits(read["scene_min"]), bits(tree["scene_min"])) and np.array_equal(bits(read["scene_max"]), bits(tree["scene_max"])), label
    assert facts is not None, "%s: %s" % (label, valid)
    assert facts["path_inner"] == read["max_depth"] <= S.MAX_DEPTH and facts["inner"] == verts.shape[0] - 1, (label, facts)


def assert_hits_equal_oracle(rt, orc, rays, label):
    o_tuv, o_prim = orc.intersect(rays, brute=True)
    g_tuv, g_prim = rt.intersect_rays(rays)
    bad = np.nonzero(g_prim != o_prim)[0]
    assert bad.size == 0, "%s: %d of %d rays report another triangle than the oracle; first: ray %d %r device %d oracle %d" % (
        label, bad.size, rays.shape[0], bad[0], rays[bad[0]].tolist(), g_prim[bad[0]], o_prim[bad[0]])
    hit = o_prim != MISS
    assert np.array_equal(bits(g_tuv[hit]), bits(o_tuv[hit])), "%s: t, u, v differ from the oracle on %d hits" % (label, int((bits(g_tuv[hit]) != bits(o_tuv[hit])).any(axis=1).sum()))
    return o_prim


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_tree_equals_the_statement(pkg, scenes, name):
    """Built on the device; the read-out equals the statement bit for bit (order, triangle words, all eight node words, max_depth, leaves,
    max_leaf == 1); check_tree accepts the device's arrays; a second handle of the same arrays reads back the same bytes (the order in which
    threads arrive in the refit does not show)."""
    sc = case_scene(name, scenes)
    verts, geom = case_triangles(name, scenes)
    tree, secs = statement_tree(name, scenes)
    rt = pkg.create_raytracer_from_arrays(sc, 70, 8, 8, seed=3, flags=lbvh_flags(pkg))
    assert rt.bvh_build_info()["on_device"], pkg.lib().mi355rt_last_error(rt._h).decode()
    read = rt.bvh_read()
    print("\n[%s] n %d, nodes %d, height %d (statement %d), statement %.2f s" % (name, verts.shape[0], read["nodes"].shape[0], read["max_depth"], tree["max_depth"], secs))
    assert_equals_statement(read, tree, verts, geom, name)
    st = rt.accel_stats()
    assert (st["nodes"], st["leaves"], st["max_depth"], st["max_leaf"]) == (verts.shape[0] - 1, verts.shape[0], tree["max_depth"], 1)
    again = pkg.create_raytracer_from_arrays(sc, 70, 8, 8, seed=3, flags=lbvh_flags(pkg))
    assert again.bvh_build_info()["on_device"]
    read2 = again.bvh_read()
    assert read2["nodes"].tobytes() == read["nodes"].tobytes() and read2["tris"].tobytes() == read["tris"].tobytes()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_walk_of_the_device_tree_gives_the_oracles_hits(pkg, oracle, scenes, name):
    """2 048 rays per case (origins in the scene box widened by half its size, targets inside it; test_bvh_statement.case_rays): closest hits
    over the device-built tree equal the brute-force oracle in the triangle and in t, u, v bit for bit; occlusion equals the host-built
    handle's.  By the oracle alone, at least 10 % of the rays hit and at least 10 % miss.

    WHAT THIS FOUND.  far800 (800 triangles of ~1e-3 at +5000, a scene box of 0.012 across; its tree equals the statement): 2 of the 2 048 rays
    lost an edge-grazing hit (u = -0.0), over the host-built tree as over the device-built one — the walk, not a builder:
      ray 177  o (4999.99951171875, 4999.9912109375, 5000.0)  d (0, 16252928, 0)          walk: triangle 724, t 8.11e-10   oracle: triangle 7, t 5.71e-10
      ray 245  o (5000.0, 4999.99755859375, 5000.0107421875)  d (0, 2621440, -12582912)   walk: triangle 232, t 9.55e-10   oracle: triangle 327, t 5.39e-10
    Both have a zero direction component on an axis on which the origin lies exactly in a face of the triangle's box.  So far from the origin the
    padding (1e-6) is below one f32 ulp (4.9e-4), the face sits ON the vertices, and 5000.0 is a binary16 value.  The walk measured a plane as
    fma(b, 1 / d', -(o / d')): for b == o the rounding error of o / d' alone, of either sign, and a negative one dropped the box.  ray_init
    (traverse.hpp) now hands the near planes -(o / d') two ulps low and the far planes two ulps high; all 17 cases pass."""
    sc = case_scene(name, scenes)
    rt = pkg.create_raytracer_from_arrays(sc, 70, 8, 8, seed=3, flags=lbvh_flags(pkg))
    assert rt.bvh_build_info()["on_device"]
    rays = case_rays(name, scenes)
    assert rays.shape == (N_RAYS, 6)
    orc = brute_oracle(oracle, sc)
    share = float((orc.intersect(rays, brute=True)[1] != MISS).mean())
    print("\n[%s] oracle hit share %.3f" % (name, share))
    assert 0.1 <= share <= 0.9                                   # by the oracle alone: at least 10 % hit, at least 10 % miss
    assert_hits_equal_oracle(rt, orc, rays, name)
    host = pkg.create_raytracer_from_arrays(sc, 70, 8, 8, seed=3, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    assert not host.bvh_build_info()["on_device"]
    assert np.array_equal(rt.occluded_rays(rays), host.occluded_rays(rays))


def _chain_handles(pkg, scenes, height, monkeypatch):
    monkeypatch.setenv("MI355RT_DEBUG_GUARD", "1")
    verts, geom, tree = chain_of_height(height)
    assert tree["max_depth"] == height
    sc = scene_with(scenes, verts, geom)
    dev = pkg.create_raytracer_from_arrays(sc, 70, 8, 8, seed=4, flags=lbvh_flags(pkg))
    host = pkg.create_raytracer_from_arrays(sc, 70, 8, 8, seed=4, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    assert not host.bvh_build_info()["on_device"]
    return sc, verts, geom, tree, dev, host


def _chain_rays_and_film(pkg, oracle, sc, tree, rt, host, height):
    """2 048 rays from the large end at the deepest triangles: closest hits equal the brute-force oracle, at least 64 answers among the 8
    deepest triangles; a 1-spp render gives the host-built handle's film bits; no guard byte is touched"""
    rays = chain_rays(height)
    o_prim = assert_hits_equal_oracle(rt, brute_oracle(oracle, sc), rays, "chain %d" % height)
    deep, _ = deepest_triangles(tree)
    n_deep = int(np.isin(o_prim, deep).sum())
    print("\n[chain of height %d] oracle hit share %.3f, %d rays answer one of the 8 deepest triangles" % (height, float((o_prim != MISS).mean()), n_deep))
    assert n_deep >= 64
    rt.render(1); host.render(1)
    for a, b in zip(rt.film.pixel_datas(), host.film.pixel_datas()):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    assert rt.debug_check_guards() == 0


def test_height_31_is_built_on_the_device_and_walked(pkg, oracle, scenes, monkeypatch):
    """The deepest tree the traversal stack serves: the chain scene of statement height exactly 31 (asserted on the CPU in
    test_bvh_statement.test_chain_scenes_have_statement_heights_31_and_32) is built on the device, equals the statement, reports
    max_depth 31, and is walked to its deepest leaves.

    WHY HEIGHT h NEEDS AT MOST THE h + 2 ROWS THAT ARE LAUNCHED.  Renderer::traversal_rows() is max_depth + 1 = h + 1, and stack_bytes(depth)
    (kernels.hip) allocates depth + 1 rows per lane: h + 2 rows, 0 .. h + 1.  In the persistent loop (traverse.hpp, inner_pred /
    pop_or_finish) row 0 holds the sentinel, deferred node k sits in row k + 1 and sp counts the deferred nodes.  A walk defers at most one
    child per inner node on the path from the root to where it stands, and what it pops it has taken off first, so sp <= number of inner
    nodes above the current node, pushes included: sp <= h.  A push writes row sp + 1 <= h (the pushing node has at most h - 1 inner nodes
    above it, so sp <= h - 1 before the push); a pop reads row sp <= h; a lane that does NOT push still writes row sp + 1 — the spare row —
    which is at most row h + 1, the last one allocated.  The branching walk (inner_step / ray_pop: intersect_rays, occluded_rays) keeps
    deferred node k in row k, rows 0 .. h - 1.  So height 31 uses every row it is given and none beyond; this test pins that limit, it does
    not go past it."""
    sc, verts, geom, tree, dev, host = _chain_handles(pkg, scenes, 31, monkeypatch)
    assert dev.bvh_build_info()["on_device"], pkg.lib().mi355rt_last_error(dev._h).decode()
    assert_equals_statement(dev.bvh_read(), tree, verts, geom, "chain 31")
    assert dev.accel_stats()["max_depth"] == 31
    _chain_rays_and_film(pkg, oracle, sc, tree, dev, host, 31)


def test_height_32_is_refused_by_the_device_builder_and_served_by_the_host(pkg, oracle, scenes, monkeypatch):
    """one triangle more: statement height 32.  The device builder refuses it and says so, the host tree serves (within the stack), the same
    ray and film checks pass"""
    S = statement()
    sc, verts, geom, tree, dev, host = _chain_handles(pkg, scenes, 32, monkeypatch)
    assert not dev.bvh_build_info()["on_device"]
    err = pkg.lib().mi355rt_last_error(dev._h).decode()
    assert "deeper than the traversal stack" in err and "32 levels" in err, err
    read = dev.bvh_read()
    facts = S.check_tree(read["nodes"], read["tris"], verts, geom, root=read["root"], leaves=read["leaves"], max_leaf=read["max_leaf"])
    assert facts["path_inner"] == read["max_depth"] == dev.accel_stats()["max_depth"] <= S.MAX_DEPTH
    href = host.bvh_read()
    assert href["nodes"].tobytes() == read["nodes"].tobytes() and href["tris"].tobytes() == read["tris"].tobytes()
    _chain_rays_and_film(pkg, oracle, sc, tree, dev, host, 32)
