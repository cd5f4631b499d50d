"""The per-triangle direction masks that prove reflection rays free (csrc/reflmask.cpp), checked on the CPU against the reference's
own f32 triangle test: real reflection rays are generated through the oracle — primary hit -> hit point in f32 -> hemisphere direction from the
sample table -> origin, for both levels — and every ray that the mask and the kernel's guard (restated here in f32, operation for operation) would
leave out is tested against EVERY triangle by brute force.  Not one may report a hit.  No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

F = np.float32
BINS = 8
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def env(pkg, oracle, scene_io):
    return pkg, oracle, scene_io


def world_pad(verts):
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    return 2e-4 * float(np.sqrt(((v.max(0) - v.min(0)) ** 2).sum())) + 1e-7


def dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]          # vecmath.rs:74-76, f32


def normals32(verts):
    v = np.asarray(verts, F).reshape(-1, 3, 3)
    a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    with np.errstate(all="ignore"):
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F)
        ln = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(F)
        return (c / ln[:, None]).astype(F)


def would_skip(words, info, prim, hu, hv, n, bo, bd, bary=None, height_scale=1.0):
    """kernels.hip, reflection_proves_miss, in f32"""
    B = BINS
    beta = F(info["bary_margin"] if bary is None else bary)
    with np.errstate(all="ignore"):
        ok = (hu > beta) & (hv > beta) & ((hu + hv).astype(F) < F(F(1.0) - beta))
        ab = np.abs(bd)
        m = np.where((ab[:, 0] >= ab[:, 1]) & (ab[:, 0] >= ab[:, 2]), 0, np.where(ab[:, 1] >= ab[:, 2], 1, 2))
        idx = np.arange(bd.shape[0])
        vm = bd[idx, m]
        va = np.where(m == 0, bd[:, 1], bd[:, 0]).astype(F)
        vb = np.where(m == 2, bd[:, 1], bd[:, 2]).astype(F)
        am = np.abs(vm)
        ok &= am > 0
        u = (va / am).astype(F); v = (vb / am).astype(F)
        i = np.clip(np.trunc(((u * F(0.5) + F(0.5)).astype(F) * F(B)).astype(F)), 0, B - 1)
        j = np.clip(np.trunc(((v * F(0.5) + F(0.5)).astype(F) * F(B)).astype(F)), 0, B - 1)
        i = np.nan_to_num(i).astype(np.int64); j = np.nan_to_num(j).astype(np.int64)
        bit = ((2 * m + (vm < 0)) * B + i) * B + j
        word = words[prim, bit >> 5]
        ok &= ((word >> (bit & 31).astype(np.uint32)) & 1) == 0
        g = words[prim, -4:].copy().view(F)
        rel = (bo - g[:, :3]).astype(F)
        ok &= dot32(rel, n).astype(F) > (g[:, 3] * F(height_scale)).astype(F)
    return ok, bit


def reflection_rays(orc, verts, table, rays6, rng, dirs_per_hit, brute):
    """the reflection rays of mod.rs:178-196 that start where rays6 hit: (prim, u, v, normal, origin, direction) per ray"""
    tuv, prim = orc.intersect(rays6, brute=brute, nthreads=16)
    hit = prim != MISS
    tuv, prim, r = tuv[hit], prim[hit].astype(np.int64), np.asarray(rays6, F).reshape(-1, 6)[hit]
    n_all = normals32(verts)
    hp = (r[:, :3] + (tuv[:, :1] * r[:, 3:]).astype(F)).astype(F)                # mod.rs:212
    k = dirs_per_hit
    prim = np.repeat(prim, k); hp = np.repeat(hp, k, 0); hu = np.repeat(tuv[:, 1], k); hv = np.repeat(tuv[:, 2], k)
    n = n_all[prim]
    jx = rng.integers(0, 65535, prim.size)
    d = table[jx]
    with np.errstate(all="ignore"):
        for _ in range(200):                                                      # sample_generator.rs:26-29: the first entry in the normal's hemisphere
            rej = dot32(d, n) <= 0
            if not rej.any():
                break
            jx = np.where(rej, (jx + 1) % 65535, jx); d = table[jx]
        keep = dot32(d, n) > 0                                                    # (degenerate normals keep what they hold in the reference; not needed here)
        bo = (hp + (F(0.00001) * d).astype(F)).astype(F)                          # mod.rs:192-193
    return prim[keep], hu[keep], hv[keep], n[keep], bo[keep], d[keep]


def census(pkg, O, scene, w, h, rng, dirs=(24, 6), want=200000, max_rounds=40, bary=None, height_scale=1.0, min_cos=0.0, pad_angle=0.0):
    verts = np.asarray(scene["tri_verts"], F).reshape(-1, 9)
    words, info = pkg.debug_reflect_mask(verts, world_pad(verts), BINS, min_cos=min_cos, pad_angle=pad_angle)     # 0: the shipped margins
    assert info["built"] and words is not None
    orc = O.Oracle(scene, w, h, seed=5)
    table = orc.sample_table().astype(F)
    generated = skipped = hits = 0
    per_level = [[0, 0], [0, 0]]
    for rnd in range(max_rounds):
        pix = rng.integers(0, w * h, 20000)
        rays = np.stack([orc.primary_ray(int(p), rnd) for p in pix])
        for level in range(2):
            prim, hu, hv, n, bo, bd = reflection_rays(orc, verts, table, rays, rng, dirs[level], brute=False)
            if prim.size == 0:
                break
            sk, _ = would_skip(words, info, prim, hu, hv, n, bo, bd, bary, height_scale)
            rays = np.concatenate([bo, bd], 1)
            generated += prim.size; skipped += int(sk.sum())
            per_level[level][0] += prim.size; per_level[level][1] += int(sk.sum())
            if sk.any():
                _, p2 = orc.intersect(rays[sk], brute=True, nthreads=16)
                hits += int((p2 != MISS).sum())
        if skipped >= want:
            break
    return dict(generated=generated, skipped=skipped, hits=hits, per_level=per_level, info=info)


def soup_scene(base, rng, kind):
    """random triangle soups like tools/parity_fuzz.py's, plus coplanar fans and a closed box seen from inside, around the 4boxes camera's view"""
    sc = dict(base)
    v = np.asarray(base["tri_verts"], np.float64).reshape(-1, 3); lo, hi = v.min(0), v.max(0); ext = float((hi - lo).max())
    if kind == "box":                                                              # a closed box around everything (camera included), plus the scene
        cam = np.asarray(base["camera_matrix"], np.float64).reshape(4, 4)
        pts = np.concatenate([v, cam[:3, 3][None], cam[3, :3][None]])
        a, b = pts.min(0) - 0.3 * ext, pts.max(0) + 0.3 * ext
        c = np.array([[x, y, z] for x in (a[0], b[0]) for y in (a[1], b[1]) for z in (a[2], b[2])])
        quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
        t = np.array([[c[q[0]], c[q[1]], c[q[2]]] for q in quads] + [[c[q[0]], c[q[2]], c[q[3]]] for q in quads])
        t = np.concatenate([t, v.reshape(-1, 3, 3)])
    else:
        n = 80
        centre = rng.uniform(lo, hi, (n, 1, 3))
        size = ext * 10.0 ** rng.uniform(-2.0, -0.6, (n, 1, 1))
        t = centre + rng.uniform(-1.0, 1.0, (n, 3, 3)) * size
        what = rng.random(n)
        for i in range(n):
            if what[i] < 0.08: t[i, 2] = t[i, 1]
            elif what[i] < 0.12: t[i, 2] = 0.5 * (t[i, 0] + t[i, 1])
            elif what[i] < 0.25 and i: t[i] = t[int(rng.integers(0, i))]          # the same triangle twice
            elif what[i] < 0.40: t[i, :, int(rng.integers(0, 3))] = t[i, 0, int(rng.integers(0, 3))]
            elif what[i] < 0.45: t[i, 1] = t[i, 0] + (t[i, 1] - t[i, 0]) * 1e-3    # a sliver
            elif what[i] < 0.60 and i:                                            # a coplanar fan: shares an edge and the plane with an earlier triangle
                s = t[int(rng.integers(0, i))]
                w_ = rng.uniform(-1.5, 1.5, 2)
                t[i] = np.stack([s[0], s[1], s[0] + w_[0] * (s[1] - s[0]) + w_[1] * (s[2] - s[0])])
    sc["tri_verts"] = t.astype(F).reshape(-1, 9)
    sc["tri_geom"] = np.zeros(t.shape[0], np.uint32)
    return sc


SCENES = [("ico2", 96, 72), ("4boxes", 96, 72), ("ico3_tex", 96, 72), ("thai2", 160, 120)]


@pytest.mark.parametrize("name,w,h", SCENES)
def test_no_skipped_reflection_ray_hits_anything(env, name, w, h):
    pkg, O, sio = env
    scene = sio.load_scene_file(os.path.join(ge.SCENES, name + ".scene"))
    r = census(pkg, O, scene, w, h, np.random.default_rng(11), dirs=(64, 4))
    print(name, {k: r[k] for k in ("generated", "skipped", "hits", "per_level")}, "build %.0f ms" % r["info"]["build_ms"])
    assert r["hits"] == 0, r
    assert r["skipped"] >= 200000, r
    if name == "thai2":
        assert r["skipped"] >= 0.10 * r["generated"], r                            # the test cannot pass on an all-set mask


@pytest.mark.parametrize("kind,seed", [("soup", 1), ("soup", 2), ("box", 3)])
def test_no_skipped_reflection_ray_hits_anything_in_a_soup(env, kind, seed):
    pkg, O, sio = env
    rng = np.random.default_rng(seed)
    scene = soup_scene(sio.load_scene_file(os.path.join(ge.SCENES, "4boxes.scene")), rng, kind)
    # few primary rays meet a sparse soup: many directions per hit
    r = census(pkg, O, scene, 96, 72, rng, dirs=(16, 4) if kind == "box" else (256, 8), max_rounds=2 if kind == "box" else 80)
    print(kind, seed, {k: r[k] for k in ("generated", "skipped", "hits", "per_level")})
    assert r["hits"] == 0, r
    if kind != "box":
        assert r["skipped"] >= 200000, r
    else:
        # The box's walls are so large that the guard's height margin (ulps of the longest edge) exceeds the reflection ray's 1e-5 lift: with the shipped guard
        # nothing that starts on a wall is skipped.  So the box checks the MASK: barycentric margin off, height margin zero (only the sign of the height, without
        # which a ray may start below its own plane).  Rays from the inside of a wall whose normal points outwards leave the box (mod.rs:186-189 draws from the
        # normal's hemisphere whichever side was hit) and are free; every ray that stays inside hits something, and its bin must be set.
        assert r["generated"] >= 200000, r
        r = census(pkg, O, scene, 96, 72, np.random.default_rng(seed), dirs=(16, 4), max_rounds=4, bary=-1.0, height_scale=0.0)
        print(kind, seed, "mask bits and the sign of the height only:", {k: r[k] for k in ("generated", "skipped", "hits")})
        assert r["hits"] == 0 and r["skipped"] >= 200000, r


def clear_bin_rays_that_hit(verts, words, t):
    """geometry in double: rays from points of triangle t (inside the guard's barycentric margin) in a 5 x 5 grid of directions of each of its CLEAR bins,
    against every other triangle; returns the (bin, other triangle) pairs that are hit"""
    v = np.asarray(verts, np.float64).reshape(-1, 3, 3)
    nbits = 6 * BINS * BINS
    bits = ((words[t, :nbits // 32, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(nbits).astype(bool)
    bary = np.array([[1 / 3, 1 / 3], [0.03, 0.03], [0.94, 0.03], [0.03, 0.94], [0.45, 0.45], [0.1, 0.6]])
    pts = v[t, 0] + bary[:, :1] * (v[t, 1] - v[t, 0]) + bary[:, 1:] * (v[t, 2] - v[t, 0])
    g = np.linspace(0.0, 1.0, 5)
    bad = []
    for b in np.nonzero(~bits)[0]:
        f, i, j = b // (BINS * BINS), (b // BINS) % BINS, b % BINS
        m = f >> 1; a = (1, 0, 0)[m]; c = (2, 2, 1)[m]; sg = -1.0 if f & 1 else 1.0
        uu, vv = np.meshgrid((i + g) / BINS * 2 - 1, (j + g) / BINS * 2 - 1)
        d = np.zeros((uu.size, 3)); d[:, m] = sg; d[:, a] = uu.ravel(); d[:, c] = vv.ravel()
        for u in range(v.shape[0]):
            if u == t:
                continue
            e1, e2 = v[u, 1] - v[u, 0], v[u, 2] - v[u, 0]
            for o in pts:
                pv = np.cross(d, e2); det = pv @ e1
                with np.errstate(all="ignore"):
                    inv = 1.0 / det
                    tv = o - v[u, 0]
                    uu_ = (pv @ tv) * inv
                    q = np.cross(tv, e1)
                    vv_ = (d @ q) * inv
                    tt = (q @ e2) * inv
                    hit = (np.abs(det) > 0) & (uu_ >= 0) & (vv_ >= 0) & (uu_ + vv_ <= 1) & (tt >= 0)
                if hit.any():
                    bad.append((int(b), u)); break
    return bad, int((~bits).sum())


WIDE = {
    # a wide flat triangle passing low over a small one: all nine vertex differences are nearly flat, their conic hull points straight up
    "ceiling": [[-0.5, -0.5, 0, 0.5, -0.5, 0, 0, 0.5, 0], [100, 0, 1, -100, 100, 1, -100, -100, 1]],
    # the same with one vertex of U BELOW T's plane and its interior above T
    "tilted": [[-0.5, -0.5, 0, 0.5, -0.5, 0, 0, 0.5, 0], [100, 0, -0.5, -100, 100, 2, -100, -100, 2]],
    # U covers only half of the sky over T; and a second small triangle beside T under the same ceiling
    "half": [[-0.5, -0.5, 0, 0.5, -0.5, 0, 0, 0.5, 0], [0.2, -300, 0.3, 0.2, 300, 0.3, 400, 0, 0.3], [2, 2, 0.1, 3, 2, 0.1, 2, 3, 0.1]],
    # far above: the cap path
    "far": [[-0.5, -0.5, 0, 0.5, -0.5, 0, 0, 0.5, 0], [100, 0, 20, -100, 100, 20, -100, -100, 20]],
}


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_flat_occluders_over_small_triangles(env, name):
    pkg, _, _ = env
    verts = np.asarray(WIDE[name], F)
    words, info = pkg.debug_reflect_mask(verts, world_pad(verts), BINS)
    assert info["built"]
    for t in range(verts.shape[0]):
        bad, nclear = clear_bin_rays_that_hit(verts, words, t)
        assert not bad, (name, t, bad[:5])
    if name in ("ceiling", "far"):                               # straight up from T leads to U: the bins around +z are set
        nbits = 6 * BINS * BINS
        bits = ((words[0, :nbits // 32, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(6, BINS, BINS).astype(bool)
        assert bits[4].all()
    if name == "half":
        assert clear_bin_rays_that_hit(verts, words, 0)[1] > 0   # the other half of the sky stays provable


def test_low_wide_ceiling_over_a_tessellated_scene(env):
    """a low, wide, flat ceiling (two triangles a hundred times the scene's size) over ico2, lower than its highest geometry on each of the three axes in
    turn; the census with the guard's margins, and the mask bits alone (no guard at all would still have to be right about every OTHER triangle:
    only rays that start below their own plane may hit, and those hit their own triangle or a coplanar one)"""
    pkg, O, sio = env
    base = sio.load_scene_file(os.path.join(ge.SCENES, "ico2.scene"))
    v = np.asarray(base["tri_verts"], np.float64).reshape(-1, 3); lo, hi = v.min(0), v.max(0); ext = float((hi - lo).max())
    for ax in range(3):
        a, b = (ax + 1) % 3, (ax + 2) % 3
        c = np.zeros((4, 3)); c[:, ax] = hi[ax] - 0.2 * (hi[ax] - lo[ax])
        c[:, a] = [-100 * ext, 100 * ext, 100 * ext, -100 * ext]; c[:, b] = [-100 * ext, -100 * ext, 100 * ext, 100 * ext]
        sc = dict(base)
        t = np.concatenate([v.reshape(-1, 3, 3), np.array([[c[0], c[1], c[2]], [c[0], c[2], c[3]]])])
        sc["tri_verts"] = t.astype(F).reshape(-1, 9)
        sc["tri_geom"] = np.concatenate([np.asarray(base["tri_geom"], np.uint32), np.zeros(2, np.uint32)])
        r = census(pkg, O, sc, 96, 72, np.random.default_rng(ax), dirs=(64, 4), want=50000, max_rounds=2)
        print("ceiling on axis", ax, {k: r[k] for k in ("generated", "skipped", "hits")})
        assert r["hits"] == 0 and r["generated"] >= 200000, r


def test_builder_invariants(env):
    pkg, O, sio = env
    scene = sio.load_scene_file(os.path.join(ge.SCENES, "ico2.scene"))
    verts = np.asarray(scene["tri_verts"], F).reshape(-1, 9).copy()
    verts[3, 6:9] = verts[3, 3:6]                                                  # two equal vertices
    verts[5, 6:9] = 0.5 * (verts[5, 0:3] + verts[5, 3:6])                          # three vertices on a line
    verts[7, 3:6] = verts[7, 0:3] + (verts[7, 3:6] - verts[7, 0:3]) * 1e-5         # a sliver
    verts[9, 0] = np.nan
    words, info = pkg.debug_reflect_mask(verts, world_pad(np.nan_to_num(verts)), BINS)
    assert info["built"] and info["stride"] == 6 * BINS * BINS // 32 + 4
    nbits = 6 * BINS * BINS
    bits = ((words[:, :nbits // 32, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1, nbits).astype(bool)
    for t in (3, 5, 7, 9):
        assert bits[t].all(), t                                                    # the whole mask of a degenerate triangle is set
    assert (~bits).any()
    # a bin that contains a direction below the minimum cosine is set: probe every bin with a dense grid of its directions (corners included)
    n = normals32(verts).astype(np.float64)
    g = np.linspace(0.0, 1.0, 5)
    for f in range(6):
        m = f >> 1; a = (1, 0, 0)[m]; b = (2, 2, 1)[m]; sg = -1.0 if f & 1 else 1.0
        for i in range(BINS):
            for j in range(BINS):
                uu, vv = np.meshgrid((i + g) / BINS * 2 - 1, (j + g) / BINS * 2 - 1)
                d = np.zeros((uu.size, 3)); d[:, m] = sg; d[:, a] = uu.ravel(); d[:, b] = vv.ravel()
                d /= np.linalg.norm(d, axis=1)[:, None]
                low = (n @ d.T).min(1) < info["min_cos"]                           # per triangle: some direction of the bin is too flat
                bit = (f * BINS + i) * BINS + j
                ok = ~np.isfinite(n).all(1) | ~low | bits[:, bit]
                assert ok.all(), (f, i, j, np.nonzero(~ok)[0][:5])
    # past its work budget no mask is built
    none, info2 = pkg.debug_reflect_mask(verts, world_pad(np.nan_to_num(verts)), BINS, work_budget=10)
    assert none is None and not info2["built"]
