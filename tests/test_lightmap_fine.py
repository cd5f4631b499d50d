"""The lights' depth cube maps at the fine resolutions (csrc/lightmap.cpp; host code, runs without a GPU): 1024 and 2048 texels per face edge, built on
several threads.  The bound of a texel must still lie at or below the squared distance of every point of every triangle seen in its directions — the
brute-force check of tests/test_lightmap.py, with the light inside, on and outside the geometry — and the threaded build must equal the build with one
thread bit for bit: a texel belongs to one band of rows, a band to one thread, and a minimum does not depend on the order it is taken in."""
import numpy as np
import pytest

from test_lightmap import lookup, sample_points

# inside: within the first sphere / the first box; on: a vertex of the scene (taken from the mesh below); outside: the scene's own light
LIGHTS = {"ico2": {"inside": (0.05, 0.02, 0.01)}, "4boxes": {"inside": (0.1, 0.05, -0.1)}}


def light_of(sc, name, where):
    if where == "inside":
        return np.asarray(LIGHTS[name]["inside"], np.float32)
    if where == "on":
        return np.asarray(sc["tri_verts"][0, :3], np.float32)
    return np.asarray(sc["lights"][0, :3], np.float32)


def build(pkg, monkeypatch, threads, tris, light, pad, res):
    monkeypatch.setenv("MI355RT_LIGHT_MAP_THREADS", str(threads))
    return pkg.debug_light_map(tris, light, pad, res)


@pytest.mark.parametrize("res", [1024, 2048])
@pytest.mark.parametrize("where", ["inside", "on", "outside"])
@pytest.mark.parametrize("name", ["ico2", "4boxes"])
def test_fine_maps_bound_every_point_and_do_not_depend_on_the_threads(pkg, scenes, monkeypatch, name, where, res):
    sc = scenes(name)
    tris = sc["tri_verts"].astype(np.float64)
    L32 = light_of(sc, name, where)
    pts_all = tris.reshape(-1, 3)
    pad = 2e-4 * np.linalg.norm(pts_all.max(0) - pts_all.min(0))
    dist2, nearest = build(pkg, monkeypatch, 8, sc["tri_verts"], L32, pad, res)
    assert dist2.shape == (6, res, res)
    one, nearest_one = build(pkg, monkeypatch, 1, sc["tri_verts"], L32, pad, res)
    assert nearest == nearest_one
    assert np.array_equal(dist2.view(np.uint32), one.view(np.uint32))
    del one
    L = L32.astype(np.float64)
    pts = sample_points(tris, 24, np.random.default_rng(3))
    d = pts - L
    d2 = (d * d).sum(1)
    ok = d2 > 1e-12
    bound = lookup(dist2, d[ok])
    assert np.all(np.isfinite(bound))                          # a texel that sees a triangle point knows about it
    assert np.all(bound.astype(np.float64) <= d2[ok])
    assert nearest ** 2 <= d2.min() * (1 + 1e-9)
    if where == "on":
        assert nearest == 0.0
    # the padding is in there: the bound stays below points pushed `pad` towards the light as well
    pushed = d[ok] * (1.0 - np.minimum(pad / np.sqrt(d2[ok]), 1.0))[:, None]
    assert np.all(bound.astype(np.float64) <= (pushed * pushed).sum(1) * (1 + 1e-6) + 1e-12)
    if where == "outside":
        # not trivially zero, and worth the texels: where a texel sees sampled points its bound is within a few percent of the nearest of them
        face_bound = bound.astype(np.float64)
        assert np.median(np.sqrt(face_bound / d2[ok])) > 0.5
        assert (dist2 > 0).sum() > 0 and np.isinf(dist2).sum() > 0


def test_the_fine_map_is_never_below_the_coarse_one(pkg, scenes, monkeypatch):
    """a texel of the 1024 map covers a quarter of a texel of the 512 map and is padded by a smaller angle: what it sees, its parent sees — its bound cannot be lower
    (up to the rounding of the two builds, 1e-6 relative)"""
    sc = scenes("thai2")
    pts_all = sc["tri_verts"].astype(np.float64).reshape(-1, 3)
    pad = 2e-4 * np.linalg.norm(pts_all.max(0) - pts_all.min(0))
    L = np.asarray(sc["lights"][0, :3], np.float32)
    coarse, _ = build(pkg, monkeypatch, 8, sc["tri_verts"], L, pad, 512)
    fine, _ = build(pkg, monkeypatch, 8, sc["tri_verts"], L, pad, 1024)
    up = np.repeat(np.repeat(coarse, 2, axis=1), 2, axis=2).astype(np.float64)
    assert np.all(fine.astype(np.float64) >= up * (1 - 1e-6))
    assert (fine > up).mean() > 0.01


@pytest.mark.parametrize("res", [512, 1024])
def test_many_triangles_on_several_threads_equal_one_thread(pkg, scenes, monkeypatch, res):
    """thai2 has 20 k triangles: the first phase hands them out to five threads in runs of 1024, each with its own rectangle lists and its own nearest
    distance — the merge of those, not only the bands of the second phase, must give the one-thread map bit for bit"""
    sc = scenes("thai2")
    pts_all = sc["tri_verts"].astype(np.float64).reshape(-1, 3)
    pad = 2e-4 * np.linalg.norm(pts_all.max(0) - pts_all.min(0))
    L = np.asarray(sc["lights"][0, :3], np.float32)
    one, nearest_one = build(pkg, monkeypatch, 1, sc["tri_verts"], L, pad, res)
    for threads in (8, 3):
        many, nearest_many = build(pkg, monkeypatch, threads, sc["tri_verts"], L, pad, res)
        assert nearest_many == nearest_one
        assert np.array_equal(many.view(np.uint32), one.view(np.uint32))
