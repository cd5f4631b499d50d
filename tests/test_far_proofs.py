"""The two host-side proofs that leave rays out — the depth cube maps around the lights (shadow rays) and the per-triangle direction masks
(reflection rays) — on scenes far from the origin and under lights far from the scene (tests/far_cases.py).  Their paddings are fractions of the
scene's diagonal and know nothing of the size of the coordinates; at +4096 one f32 ulp is already more than the BVH's own padding.  Checked here on
the CPU against the oracle's brute-force intersector: no ray that a proof calls free may be blocked (light maps) or hit anything (masks).  No GPU.

The map, tail2 and the lookup are restated as renderer.cpp (the light-map block of the scene upload) and kernels.hip (light_proves_unoccluded)
compute them; texel_of / lookup / sample_points are tests/test_lightmap.py's, census is tests/test_reflmask.py's."""
import numpy as np
import pytest

import far_cases as fc
from test_lightmap import lookup, sample_points
from test_reflmask import census

F = np.float32
MISS = 0xFFFFFFFF
RES = 512                                                            # the shipped resolution
PER_TRI = 24


def light_map_and_tail2(pkg, scene):
    """renderer.cpp: pad = 2e-4 * diag + 1e-7 over the f32 vertices' box; the map at RES; tail2 from (nearest - pad)^2, rounded down"""
    _, _, diag = fc.box_of(scene)
    pad = 2e-4 * diag + 1e-7
    dist2, nearest = pkg.debug_light_map(scene["tri_verts"], np.asarray(scene["lights"], F)[0, :3], pad, RES)
    tail = max(nearest - pad, 0.0)
    tail2 = F(min(tail * tail * (1.0 - 1e-6), 3.0e38)) if np.isfinite(tail) else F(3.0e38)
    if float(tail2) > tail * tail:
        tail2 = np.nextafter(tail2, F(0.0))
    return dist2, tail2


def proves_unoccluded(dist2, tail2, l):
    """kernels.hip, light_proves_unoccluded, in f32 (unfused, as the library is built): l = light - hp"""
    l = l.astype(F)
    l2 = ((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]).astype(F) + l[:, 2] * l[:, 2]).astype(F)
    v = (-l).astype(F)
    ok = (np.abs(v).max(1) > 0) & (l2 < F(3.0e38))
    with np.errstate(all="ignore"):
        bound = lookup(dist2, v)
    return ok & ((l2 * F(0.98011)).astype(F) < bound) & ((l2 * F(1.0002e-4)).astype(F) < tail2)


def shadow_census(pkg, oracle, scene, seed):
    """(points, proved free, blocked, proved free AND blocked): the shadow rays of mod.rs:224-225 from points on every triangle to light 0"""
    dist2, tail2 = light_map_and_tail2(pkg, scene)
    tris = np.asarray(scene["tri_verts"], F).reshape(-1, 9).astype(np.float64)
    hp = sample_points(tris, PER_TRI, np.random.default_rng(seed)).astype(F)           # the reference's hit point is an f32 point
    light = np.asarray(scene["lights"], F)[0, :3]
    l = (light[None, :] - hp).astype(F)                                                # mod.rs:215
    proved = proves_unoccluded(dist2, tail2, l)
    o = (hp + (l * F(0.01)).astype(F)).astype(F)                                       # oracle.c, shade: pos + 0.01 dir
    orc = oracle.Oracle(scene, 8, 8, seed=1, flags=oracle.FLAG_BRUTE_FORCE)
    tuv, prim = orc.intersect(np.concatenate([o, l], 1), brute=True, nthreads=8)
    blocked = (prim != MISS) & (tuv[:, 0] > F(0.01)) & (tuv[:, 0] < F(1.0))            # oracle.c, shade: the closest hit decides
    assert float(tail2) > 0.0 and np.isfinite(dist2).any()
    return hp.shape[0], int(proved.sum()), int(blocked.sum()), int((proved & blocked).sum())


# the light 2 diagonals away is the control: near enough to cast shadows; then the far lights; every translation with the scene's own light and with the
# light at 2 diagonals
LIGHT_CASES = [(name, fc.OFFSETS[0], d) for name in fc.SCENE_NAMES for d in (2.0,) + fc.LIGHT_DIAGONALS] + \
              [(name, off, d) for name in fc.SCENE_NAMES for off in fc.OFFSETS[1:] for d in (None, 2.0)]


@pytest.mark.parametrize("name,offset,diagonals", LIGHT_CASES, ids=lambda x: "own" if x is None else str(x).replace(" ", ""))
def test_no_shadow_ray_proved_free_is_blocked(pkg, oracle, scenes, name, offset, diagonals):
    sc = fc.case_scene(scenes(name), offset, diagonals)
    assert fc.is_finite(sc)
    n, proved, blocked, both = shadow_census(pkg, oracle, sc, seed=3)
    print("\n[%s %r light %s] %d points, %d proved free, %d blocked, %d both" % (name, offset, diagonals, n, proved, blocked, both))
    assert both == 0
    assert proved > 0                                                # not an all-zero map
    if diagonals == 2.0:
        assert blocked > 0                                           # near enough to cast shadows: the check could fail
        assert abs(fc.light_diagonals(sc) - 2.0) < 1e-2


@pytest.mark.parametrize("offset", fc.OFFSETS, ids=lambda x: str(x).replace(" ", ""))
@pytest.mark.parametrize("name", fc.SCENE_NAMES)
def test_no_skipped_reflection_ray_hits_anything_far_away(pkg, oracle, scenes, name, offset):
    sc = fc.moved(scenes(name), offset)
    at_origin = offset == fc.OFFSETS[0]
    # at the origin as tests/test_reflmask.py runs it; far away the masks may stand down (no skips at all), so the rounds are bounded
    r = census(pkg, oracle, sc, 96, 72, np.random.default_rng(11), dirs=(64, 4), want=200000 if at_origin else 60000, max_rounds=40 if at_origin else 3)
    print("\n[%s %r] generated %d, skipped %d, hits %d, per level %r" % (name, offset, r["generated"], r["skipped"], r["hits"], r["per_level"]))
    assert r["hits"] == 0, r
    assert r["generated"] >= 100000, r
    if at_origin:
        assert r["skipped"] >= 200000, r
