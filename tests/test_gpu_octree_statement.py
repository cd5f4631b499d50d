"""The device walk held to the independent statement of the reference's octree (oracle/octree_statement.py).

Both device paths that claim the reference's OctTreeIntersector semantics - flags 0 (BVH + confirm step) and
FLAG_OCTREE_SEMANTICS (the direct walk of the octree) - must give the statement's hit record for every ray: the triangle,
and t, u, v bit for bit.  The rays are built from the statement's own cubes (test_octree_statement.statement_rays); the
statement's answers are computed once per case on the CPU and shared by both paths."""
import numpy as np
import pytest

from test_octree_statement import MISS, WALK_CASES, bits, scene_of, statement_tree, statement_walk, tie_walk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", ["bvh_confirm", "octree_walk"])
@pytest.mark.parametrize("name,tpl", WALK_CASES, ids=["%s-%d" % c for c in WALK_CASES])
def test_device_walk_equals_the_statement(pkg, scenes, name, tpl, path):
    sc = scene_of(name, scenes)
    rays, tuv, prim, blocked, secs = statement_walk(name, tpl, scenes)
    n = rays.shape[0]
    hit = prim != MISS
    assert n <= 4096
    # the rays do what they are for: hits and misses, occluded and free rays, at least 5 % each
    assert min(hit.sum(), (~hit).sum()) >= 0.05 * n and min(blocked.sum(), (blocked == 0).sum()) >= 0.05 * n
    flags = pkg.FLAG_OCTREE_SEMANTICS if path == "octree_walk" else 0
    rt = pkg.create_raytracer_from_arrays(sc, tpl, 8, 8, flags=flags)
    # the tree the handle built is the statement's, as far as the handle tells
    st = statement_tree(name, tpl, scenes).stats()
    assert rt.octree_stats() == {k: st[k] for k in ("nodes", "inner", "leaves", "empty", "depth", "tri_refs")}
    g_tuv, g_prim = rt.intersect_rays(rays)
    bad = np.nonzero(g_prim != prim)[0]
    assert bad.size == 0, "%d of %d rays report another triangle than the statement; first: ray %d %r device %d statement %d" % (
        bad.size, n, bad[0], rays[bad[0]].tolist(), g_prim[bad[0]], prim[bad[0]])
    assert np.array_equal(bits(g_tuv[hit]), bits(tuv[hit])), "t, u, v differ from the statement on %d hits" % int((bits(g_tuv[hit]) != bits(tuv[hit])).any(axis=1).sum())
    assert np.array_equal(rt.occluded_rays(rays), blocked)
    # the true closest hit differs somewhere: otherwise the rays would not exercise the semantics
    closest = pkg.create_raytracer_from_arrays(sc, tpl, 8, 8, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
    _, c_prim = closest.intersect_rays(rays)
    print("\n[%s at %d, %s] %d rays, %d hits, %d occluded, %d whose octree answer is not the true closest hit; statement walk %.1f s"
          % (name, tpl, path, n, int(hit.sum()), int(blocked.sum()), int((c_prim != prim).sum()), secs))
    assert (c_prim != prim).sum() > 0


@pytest.mark.parametrize("path", ["bvh_confirm", "octree_walk"])
def test_device_walk_keeps_the_stable_order(pkg, scenes, path):
    """the recorded rays of 4boxes at 5 on which children of equal t, walked in the other order, give another answer
    (test_octree_statement.test_stable_order_decides_on_the_recorded_rays): the device gives the statement's"""
    rays, tuv, prim = tie_walk(scenes)
    rt = pkg.create_raytracer_from_arrays(scenes("4boxes"), 5, 8, 8, flags=pkg.FLAG_OCTREE_SEMANTICS if path == "octree_walk" else 0)
    g_tuv, g_prim = rt.intersect_rays(rays)
    assert np.array_equal(g_prim, prim), "rays %r" % np.nonzero(g_prim != prim)[0].tolist()
    m = prim != MISS
    assert np.array_equal(bits(g_tuv[m]), bits(tuv[m]))
