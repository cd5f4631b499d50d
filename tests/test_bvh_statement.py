"""The binary BVH held to an independent statement, without a GPU.

oracle/bvh_statement.py states the tree csrc/lbvh.hip builds on the device — keys, order, Karras' hierarchy, boxes, the
emitted words — and has a check_tree() for the tree of ANY builder.  Here the statement is checked against itself (the directed
half rounding against exact rational bounds, the keys against Python integers, the hierarchy against brute force), check_tree
walks the HOST builder's tree (mi355rt_debug_bvh_read without a handle), and the two chain scenes that pin the depth limit are
chosen and asserted.  tests/test_gpu_lbvh_statement.py holds the device build to the statement word for word, on the cases and
rays made here.

DEPTH CONVENTIONS.  The device builder reports the root's HEIGHT (a node over two leaves has height 1); the host builder
(bvh.cpp, emit_leaf) reports the depth of the deepest LEAF, the root having depth 0.  Both are the greatest number of inner nodes
on a root-to-leaf path, which is what check_tree counts, and what the traversal stack serves: at most traversal_rows() - 1 =
max_depth, and max_depth <= 31."""
import importlib.util
import os
import sys
import time
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF
N_RAYS = 2048


def statement():
    name = "bvh_statement"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "oracle", "bvh_statement.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- the cases
def _blob(n, seed, spread=0.2, extent=10.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.3 * extent, 0.7 * extent, (n, 1, 3))
    return (c + rng.uniform(-spread, spread, (n, 3, 3))).astype(np.float32).reshape(n, 9)


def _identical():
    return np.repeat(_blob(1, 21, spread=1.5), 300, axis=0)


def _copies():
    """2 000 triangles: 1 000 copies of 7 originals (runs of equal keys of ~143) among 1 000 spread ones, shuffled"""
    rng = np.random.default_rng(22)
    seven = _blob(7, 23, spread=0.8)
    v = np.concatenate([seven[rng.integers(0, 7, 1000)], _blob(1000, 24)])
    return v[rng.permutation(2000)]


def _plane(axis):
    v = _blob(500, 25 + axis, spread=0.4)
    v[:, axis::3] = np.float32(1.25)                       # a zero extent on this axis: sinv = 0
    return v


def _line():
    """400 small triangles whose centres lie on one line across the scene box: the three key coordinates move together"""
    rng = np.random.default_rng(28)
    c = np.array([-3.0, 0.5, -1.5]) + rng.uniform(0.0, 10.0, (400, 1, 1)) * np.array([1.0, 0.5, 0.25])
    return (c + rng.uniform(-0.05, 0.05, (400, 3, 3))).astype(np.float32).reshape(400, 9)


def _max_corner():
    """200 triangles and one (a point) whose box centre is exactly the scene's max corner: its cell number is clamped to 2097151 on every axis"""
    v = _blob(200, 29)
    corner = v.reshape(-1, 3).max(axis=0) + np.float32(1.0)
    return np.concatenate([v[:100], np.tile(corner, 3)[None, :], v[100:]]).astype(np.float32)


CASES = {
    "blob5": lambda: _blob(5, 11), "blob6": lambda: _blob(6, 12),                       # 5: the smallest the device serves
    "blob255": lambda: _blob(255, 13), "blob256": lambda: _blob(256, 14), "blob257": lambda: _blob(257, 15),      # around one block
    "blob4099": lambda: _blob(4099, 16),                                               # 17 blocks: the refit hands boxes across blocks
    "identical300": _identical,                                                        # every key equal
    "copies2000": _copies,
    "plane_x": lambda: _plane(0), "plane_y": lambda: _plane(1), "plane_z": lambda: _plane(2),
    "line400": _line,
    "max_corner201": _max_corner,
    "far800": lambda: _blob(800, 8, spread=1e-3, extent=1e-2) + np.float32(5000.0),     # coarse halves, coarse f32
    "huge50": lambda: _blob(50, 10) * np.float32(1e4),                                 # beyond the half range: +-inf and +-65504 in the boxes
}
SCENE_FILE_CASES = ("4boxes", "ico2")
CASE_NAMES = tuple(CASES) + SCENE_FILE_CASES
# share of the rays aimed at a point of a triangle (the rest at a uniform point of the scene box), and the power of two the directions
# are scaled by: the triangle test refuses |det| < f32 epsilon, and det grows with the direction's length (far800: edges of ~1e-3)
RAY_PLAN = {"line400": (0.6, 0), "far800": (0.2, 30), "huge50": (0.6, 0), "4boxes": (0.0, 0), "ico2": (0.2, 0)}
N_GEOM = 3                                          # tri_geom of the generated cases: below every scene file's material count


def case_triangles(name, scenes):
    """(tri_verts (n, 9) f32, tri_geom (n,) u32)"""
    if name not in CASES:                             # a scene file
        sc = scenes(name)
        return np.ascontiguousarray(sc["tri_verts"], np.float32).reshape(-1, 9), np.ascontiguousarray(sc["tri_geom"], np.uint32)
    v = np.ascontiguousarray(CASES[name](), np.float32)
    return v, ((np.arange(v.shape[0]) * 7 + 1) % N_GEOM).astype(np.uint32)


def case_scene(name, scenes):
    """a scene dict the library and the oracle take: the case's triangles with 4boxes' materials, lights and camera"""
    if name in SCENE_FILE_CASES:
        return scenes(name)
    v, g = case_triangles(name, scenes)
    return scene_with(scenes, v, g)


def scene_with(scenes, verts, geom):
    sc = dict(scenes("4boxes"))
    assert len(sc["mat_kind"]) >= N_GEOM
    sc["tri_verts"] = np.ascontiguousarray(verts, np.float32).reshape(-1, 9); sc["tri_geom"] = np.ascontiguousarray(geom, np.uint32)
    return sc


def brute_oracle(oracle, sc):
    """the CPU oracle for brute-force closest hits; its octree is never walked here, so it is kept to one leaf (300 identical triangles would split to the last level)"""
    return oracle.Oracle(sc, 8, 8, tris_per_leaf=1 << 30, flags=oracle.FLAG_BRUTE_FORCE)


_TREES = {}


def statement_tree(name, scenes):
    """the statement's tree of a case, built once: (tree dict, CPU seconds)"""
    if name not in _TREES:
        v, g = case_triangles(name, scenes)
        t0 = time.perf_counter()
        tree = statement().build(v, g)
        _TREES[name] = (tree, time.perf_counter() - t0)
    return _TREES[name]


def _points_on(verts, which, rng):
    """a point well inside each of the triangles verts[which], in float64"""
    t = np.asarray(verts, np.float64).reshape(-1, 3, 3)[which]
    u = rng.uniform(0.1, 0.45, (len(which), 1)); w = rng.uniform(0.1, 0.45, (len(which), 1))
    return t[:, 0] + u * (t[:, 1] - t[:, 0]) + w * (t[:, 2] - t[:, 0])


def case_rays(name, scenes):
    """2 048 rays: origins in the scene box widened by half its size, targets inside it — a share of them on the geometry itself"""
    v, _ = case_triangles(name, scenes)
    share, scale = RAY_PLAN.get(name, (0.4, 0))
    rng = np.random.default_rng(1000 + CASE_NAMES.index(name))
    p = v.reshape(-1, 3).astype(np.float64); lo, hi = p.min(axis=0), p.max(axis=0)
    wide = np.where(hi > lo, hi - lo, (hi - lo).max())          # a flat scene: widened by its largest extent there, or every ray lies in the plane
    org = rng.uniform(lo - 0.5 * wide, hi + 0.5 * wide, (N_RAYS, 3))
    tgt = rng.uniform(lo, hi, (N_RAYS, 3))
    k = int(share * N_RAYS)
    tgt[:k] = _points_on(v, rng.integers(0, v.shape[0], k), rng)
    o32 = org.astype(np.float32); d32 = (tgt.astype(np.float32) - o32) * np.float32(2.0 ** scale)
    return np.concatenate([o32, d32], axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the chain scenes
def chain_scene(count):
    """A scene whose device tree is one long chain.  The scene box is exactly [0, 2]^3, held by one small anchor triangle at each of the
    two corners (keys 0 and 2^63 - 1).  Triangle m = 0 .. count - 1 has the single key bit 2^m: x is bit 2, y bit 1, z bit 0 of a triple,
    so its box centre is 2^(m // 3 - 20) on axis 2 - m % 3, with the box centre +- 2^-23 there (exact in f32), and [0, 2^-22] on the other
    two axes (centre 2^-23: cell 0).  The radix tree over 0, 1, 2, 4, ..., 2^(count - 1), 2^63 - 1 peels one key off per level.
    Returns (tri_verts, tri_geom); triangle 0 and 1 are the anchors, triangle m + 2 has the key 2^m."""
    s, e, h = 2.0 ** -22, 2.0 ** -20, 2.0 ** -23
    t = [[0, 0, 0, s, 0, 0, 0, s, 0], [2, 2, 2, 2 - e, 2, 2, 2, 2 - e, 2]]
    for m in range(count):
        a = 2 - m % 3; b, c = (a + 1) % 3, (a + 2) % 3
        mid = 2.0 ** (m // 3 - 20)
        v = np.zeros((3, 3))
        v[0, a] = mid - h; v[1, a] = mid + h; v[1, b] = s; v[2, a] = mid; v[2, c] = s
        t.append(v.reshape(9).tolist())
    v32 = np.array(t, np.float32)
    assert np.array_equal(v32.astype(np.float64), np.array(t))                  # every coordinate is exact in f32
    return v32, ((np.arange(count + 2) * 7 + 1) % N_GEOM).astype(np.uint32)


_CHAIN = {}


def chain_of_height(height):
    """(tri_verts, tri_geom, statement tree) of the chain scene whose STATEMENT height is `height`: the count is found here, from the statement"""
    if height not in _CHAIN:
        for count in range(1, 64):
            v, g = chain_scene(count)
            tree = statement().build(v, g)
            if tree["max_depth"] == height:
                _CHAIN[height] = (v, g, tree)
                break
        else:
            raise AssertionError("no chain scene of height %d" % height)
    return _CHAIN[height]


def deepest_triangles(tree, k=8):
    """the triangles (prim) in the k deepest leaves of a statement tree"""
    n = tree["order"].shape[0]
    leaf_depth = np.zeros(n, np.int64)
    todo = [(0, 0)]
    while todo:
        ref, above = todo.pop()
        if ref < 0:
            leaf_depth[~ref] = above
        else:
            todo.append((int(tree["left"][ref]), above + 1)); todo.append((int(tree["right"][ref]), above + 1))
    pos = np.argsort(-leaf_depth, kind="stable")[:k]
    return tree["order"][pos].astype(np.int64), leaf_depth[pos]


def chain_rays(height):
    """2 048 rays from beyond the large end of the chain (the triangles at 2^-11 .. 2^-10) at points inside the 16 deepest triangles.  The
    triangles are 2^-22 across: the directions are scaled by 2^38 (exact) so that the triangle test's |det| >= f32 epsilon rule lets them be hit."""
    v, _, tree = chain_of_height(height)
    rng = np.random.default_rng(77 + height)
    deep, _ = deepest_triangles(tree, 16)
    tgt = _points_on(v, deep[np.arange(N_RAYS) % 16], rng)
    org = 2.0 ** -10 * (1.0 + 0.5 * rng.uniform(0.0, 1.0, (N_RAYS, 3)))
    o32 = org.astype(np.float32); d32 = (tgt.astype(np.float32) - o32) * np.float32(2.0 ** 38)
    return np.concatenate([o32, d32], axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the statement against itself
def _half_values():
    """every finite binary16 value as an exact Fraction, ascending, with its bit pattern; -0 before +0"""
    pats = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    vals = pats.view(np.float16).astype(np.float64)
    keep = np.isfinite(vals)
    rows = sorted(((Fraction(float(x)), 0 if (int(p) & 0x8000) else 1, int(p)) for x, p in zip(vals[keep], pats[keep])))
    return rows


def test_directed_half_rounding_is_the_tightest_bound_on_the_right_side():
    """half_bits_directed against exact rational arithmetic: the result is the smallest binary16 >= x (up) or the largest <= x (down),
    +-inf where no finite one exists.  Random f32 values over the whole exponent range of binary16 and beyond, and the edges."""
    S = statement()
    rng = np.random.default_rng(5)
    x = np.concatenate([
        (rng.uniform(-1, 1, 4000) * 10.0 ** rng.uniform(-9, 5.2, 4000)).astype(np.float32),
        rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32),              # any bit pattern (NaNs are dropped below)
        np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 5.9604645e-8, -5.9604645e-8, 5.96e-8, 2.98e-8, -2.98e-8, 6.1035156e-5, 6.1e-5, -6.1e-5,
                  65504.0, -65504.0, 65504.004, -65504.004, 65519.99, 65520.0, -65520.0, 70000.0, -70000.0, 3.4e38, -3.4e38, 1.0, 1.0004883, 1.0004, -1.0004,
                  np.inf, -np.inf], np.float32)])
    x = x[~np.isnan(x)]
    rows = _half_values()
    fin = [r[0] for r in rows]
    import bisect
    for up in (False, True):
        got = S.half_bits_directed(x, up)
        for xi, gi in zip(x.tolist(), got.tolist()):
            if np.isinf(xi):
                want = (0x7C00 if xi > 0 else 0xFC00)
            else:
                f = Fraction(xi)
                if up:
                    k = bisect.bisect_left(fin, f)                  # first finite half >= x
                    want = 0x7C00 if k == len(fin) else None
                else:
                    k = bisect.bisect_right(fin, f) - 1             # last finite half <= x
                    want = 0xFC00 if k < 0 else None
                if want is None:
                    if fin[k] == 0:                                 # +-0: any zero is the tightest bound; the sign follows the round to nearest
                        assert gi in (0x0000, 0x8000), (xi, up, hex(gi))
                        continue
                    want = rows[k][2]
            assert gi == want, (xi, up, hex(gi), hex(want))
    nan = np.array([np.nan], np.float32)
    assert S.half_bits_directed(nan, True)[0] == 0x7C00 and S.half_bits_directed(nan, False)[0] == 0xFC00
    # the zero edges, exactly as bvh.cpp's half_bits_directed gives them
    z = np.array([0.0, -0.0, 1e-40, -1e-40], np.float32)
    assert S.half_bits_directed(z, True).tolist() == [0x0000, 0x8000, 0x0001, 0x8000]
    assert S.half_bits_directed(z, False).tolist() == [0x0000, 0x8000, 0x0000, 0x8001]


def test_keys_against_python_integers():
    """the key of a few hundred triangles, restated with exact rationals for the f32 steps that are exact by construction: the points sit
    on a grid of k / 2^21 in a [0, 1]^3 scene box, so every product and difference of the key is exact and the cell is k itself"""
    S = statement()
    rng = np.random.default_rng(6)
    k = rng.integers(0, 2 ** 21, (400, 3))
    k[0] = 0; k[1] = 2 ** 21 - 1; k[2] = (2 ** 21 - 1, 0, 0); k[3] = (0, 2 ** 21 - 1, 0); k[4] = (0, 0, 2 ** 21 - 1); k[5] = (1, 2, 4)
    c = k.astype(np.float64) / 2.0 ** 21
    tri = np.concatenate([c, c, c], axis=1)                                       # point triangles: the box centre is the point
    anchors = np.array([[0.0] * 9, [1.0] * 9])
    v = np.concatenate([anchors, tri]).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), np.concatenate([anchors, tri]))
    smin, smax = S.scene_bounds(v)
    assert smin.tolist() == [0, 0, 0] and smax.tolist() == [1, 1, 1]
    keys = S.morton_keys(v, smin, smax)
    assert int(keys[0]) == 0 and int(keys[1]) == 2 ** 63 - 1                      # the max corner: clamped to 2097151 on every axis
    for row, key in zip(k.tolist(), keys[2:].tolist()):
        want = 0
        for b in range(21):
            want |= ((row[0] >> b) & 1) << (3 * b + 2) | ((row[1] >> b) & 1) << (3 * b + 1) | ((row[2] >> b) & 1) << (3 * b)
        assert int(key) == want, (row, hex(int(key)), hex(want))
    # a zero extent gives cell 0 on that axis; a general scene: floor((c - smin) / extent * 2^21) within one cell of the exact value
    g = _blob(300, 31); g[:, 1::3] = np.float32(-2.5)
    smin, smax = S.scene_bounds(g)
    q = S.quantised_centres(g, smin, smax)
    assert not q[:, 1].any() and q.min() >= 0 and q.max() <= 2097151
    tv = g.reshape(-1, 3, 3).astype(np.float64)
    for a in (0, 2):
        exact = (0.5 * (tv[:, :, a].min(axis=1) + tv[:, :, a].max(axis=1)) - float(smin[a])) / (float(smax[a]) - float(smin[a])) * 2.0 ** 21
        assert np.abs(q[:, a] - np.minimum(np.floor(exact), 2097151)).max() <= 1


def _common_prefix(a, b):
    """length of the common prefix of two (key, position) pairs, as 64 + 32 bits"""
    x = ((a[0] ^ b[0]) << 32) | (a[1] ^ b[1])
    return 96 - x.bit_length()


@pytest.mark.parametrize("n,seed,keybits", [(2, 1, 3), (3, 2, 2), (7, 3, 2), (16, 4, 0), (33, 5, 4), (64, 6, 3), (64, 7, 40), (61, 8, 1)])
def test_hierarchy_against_brute_force(n, seed, keybits):
    """for every inner node of the radix tree: its leaves are a contiguous range [lo, hi] that holds the node's own number as one end, all
    pairs in it share a prefix, and the range is MAXIMAL (neither neighbour shares that prefix); its children split the range at the first bit
    that differs, and are numbered gamma and gamma + 1.  Few key bits give long runs of equal keys (0 bits: all keys equal)."""
    S = statement()
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.integers(0, 2 ** keybits, n).astype(np.uint64) << np.uint64(rng.integers(0, 63 - keybits)))
    lo, hi, left, right = S.radix_tree(keys)
    pairs = [(int(k), i) for i, k in enumerate(keys)]
    assert lo[0] == 0 and hi[0] == n - 1
    covered = np.zeros(n, int)
    for i in range(n - 1):
        a, b = int(lo[i]), int(hi[i])
        assert i in (a, b) and a < b
        inside = min(_common_prefix(pairs[p], pairs[q]) for p in range(a, b + 1) for q in range(p + 1, b + 1))
        assert inside == _common_prefix(pairs[a], pairs[b])
        for nb in (a - 1, b + 1):
            if 0 <= nb < n:
                assert max(_common_prefix(pairs[nb], pairs[p]) for p in range(a, b + 1)) < inside, "range of node %d is not maximal" % i
        # the split: the left part shares more than the node's prefix, and so does the right part; across the split exactly the node's prefix
        kids = []
        for ref in (int(left[i]), int(right[i])):
            kids.append((~ref, ~ref) if ref < 0 else (int(lo[ref]), int(hi[ref])))
            if ref < 0:
                covered[~ref] += 1
        (la, lb), (ra, rb) = kids
        assert la == a and rb == b and ra == lb + 1
        gamma = lb
        assert (left[i] < 0 or left[i] == gamma) and (right[i] < 0 or right[i] == gamma + 1)
        assert _common_prefix(pairs[gamma], pairs[gamma + 1]) == inside
        assert la == lb or _common_prefix(pairs[la], pairs[lb]) > inside
        assert ra == rb or _common_prefix(pairs[ra], pairs[rb]) > inside
    assert (covered == 1).all()


def test_statement_tree_is_a_valid_tree_on_every_case(scenes):
    """check_tree, which shares nothing with build(), accepts the statement's own tree on every case; n, nodes, height and seconds are printed"""
    S = statement()
    for name in CASE_NAMES:
        v, g = case_triangles(name, scenes)
        tree, secs = statement_tree(name, scenes)
        facts = S.check_tree(tree["nodes"], tree["tris"], v, g, root=0, leaves=tree["leaves"], max_leaf=1)
        assert facts["path_inner"] == tree["max_depth"] and facts["inner"] == v.shape[0] - 1
        assert np.array_equal(tree["scene_min"], v.reshape(-1, 3).min(0)) and np.array_equal(tree["scene_max"], v.reshape(-1, 3).max(0))
        print("\n[%s] n %d, nodes %d, height %d, statement %.2f s" % (name, v.shape[0], tree["nodes"].shape[0], tree["max_depth"], secs))
    # the cases are what they claim to be
    assert np.unique(statement_tree("identical300", scenes)[0]["keys"]).size == 1
    k = statement_tree("copies2000", scenes)[0]["keys"]
    assert 900 < np.unique(k).size < 1100 and np.unique(k, return_counts=True)[1].max() > 100
    for a, name in enumerate(("plane_x", "plane_y", "plane_z")):
        v, _ = case_triangles(name, scenes)
        assert not S.quantised_centres(v, *S.scene_bounds(v))[:, a].any()
    v, _ = case_triangles("max_corner201", scenes)
    assert S.quantised_centres(v, *S.scene_bounds(v))[100].tolist() == [2097151] * 3
    inf_halves = 0
    for w in statement_tree("huge50", scenes)[0]["nodes"][:, [0, 1, 2, 4, 5, 6]].reshape(-1):
        inf_halves += int((int(w) & 0x7FFF) == 0x7C00) + int((int(w) >> 16 & 0x7FFF) == 0x7C00)
    assert inf_halves > 0


def test_check_tree_notices_what_it_is_there_for(scenes):
    """a box one half-precision step too small, a triangle in two leaves, a lost triangle and a wrong edge are each refused"""
    S = statement()
    v, g = case_triangles("blob257", scenes)
    tree, _ = statement_tree("blob257", scenes)
    nodes, tris = tree["nodes"], tree["tris"]
    S.check_tree(nodes, tris, v, g)
    # shrink one maximum by one step where the box is tight against a vertex: find a child box whose stepped maximum no longer holds it
    found = False
    for i in range(nodes.shape[0]):
        bad = nodes.copy()
        hi = int(bad[i, 0]) >> 16
        hi = hi - 1 if not hi & 0x8000 else hi + 1
        bad[i, 0] = (int(bad[i, 0]) & 0xFFFF) | hi << 16
        try:
            S.check_tree(bad, tris, v, g)
        except AssertionError as e:
            assert "does not hold" in str(e)
            found = True
            break
    assert found
    leaf_rows = np.nonzero(nodes[:, 3].view(np.int32) < 0)[0]
    bad = nodes.copy(); bad[leaf_rows[0], 3] = bad[leaf_rows[1], 3]
    with pytest.raises(AssertionError, match="in no leaf|more than one leaf|does not hold"):
        S.check_tree(bad, tris, v, g)
    bad_t = tris.copy(); bad_t[5, 4] ^= 1
    with pytest.raises(AssertionError, match="e1 differs"):
        S.check_tree(nodes, bad_t, v, g)
    bad_t = tris.copy(); bad_t[5, 3] = bad_t[6, 3]
    with pytest.raises(AssertionError, match="permutation"):
        S.check_tree(nodes, bad_t, v, g)


# ---------------------------------------------------------------------------------------------------- the host builder's tree
HOST_CASES = CASE_NAMES + ("thai2",)


@pytest.mark.parametrize("passes", ["0", "4"])
def test_host_tree_passes_check_tree(pkg, scenes, monkeypatch, passes):
    """The binary tree of the HOST builder (bvh.cpp: binned SAH, MI355RT_BVH_OPT passes of re-insertion), read out through
    mi355rt_debug_bvh_read without a handle and walked by check_tree: every triangle in exactly one leaf, the triangle words right on the
    bits, every child box holds every vertex below it, leaves and max_leaf as reported.  The host's max_depth is the depth of its deepest
    leaf with the root at depth 0: the number of inner nodes on the longest path, which must not exceed 31 (traversal_rows() - 1)."""
    S = statement()
    monkeypatch.setenv("MI355RT_BVH_OPT", passes)
    for name in HOST_CASES:
        v, g = case_triangles(name, scenes)
        t = pkg.debug_bvh(v, g)
        facts = S.check_tree(t["nodes"], t["tris"], v, g, root=t["root"], leaves=t["leaves"], max_leaf=t["max_leaf"])
        assert facts["path_inner"] == t["max_depth"] <= S.MAX_DEPTH, name
        assert t["max_leaf"] <= 4 and t["tris"].shape[0] == v.shape[0]
        assert np.array_equal(t["scene_min"], v.reshape(-1, 3).min(0)) and np.array_equal(t["scene_max"], v.reshape(-1, 3).max(0))
    for height in (31, 32):                                                   # the chain scenes: the host tree stays within the stack
        v, g, _ = chain_of_height(height)
        t = pkg.debug_bvh(v, g)
        facts = S.check_tree(t["nodes"], t["tris"], v, g, root=t["root"], leaves=t["leaves"], max_leaf=t["max_leaf"])
        assert facts["path_inner"] == t["max_depth"] <= S.MAX_DEPTH
    one = _blob(1, 41)                                                        # a scene of one leaf: the root is a leaf code
    t = pkg.debug_bvh(one)
    assert t["root"] < 0 and S.check_tree(t["nodes"], t["tris"], one, np.zeros(1, np.uint32), root=t["root"], leaves=1, max_leaf=1)["path_inner"] == 0 == t["max_depth"]


def test_bvh_read_size_query_and_short_buffers(pkg):
    import ctypes as C
    L = pkg.lib()
    v = _blob(37, 42); g = (np.arange(37) % 3).astype(np.uint32)
    F, U = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    vp, gp = v.ctypes.data_as(F), g.ctypes.data_as(U)
    info = np.zeros(8, np.uint32); bounds = np.zeros(6, np.float32)
    assert L.mi355rt_debug_bvh_read(None, vp, gp, 37, info.ctypes.data_as(U), bounds.ctypes.data_as(F), None, 0, None, 0) == 0
    nn, nt = int(info[0]), int(info[1])
    assert nn > 0 and nt == 37 and np.array_equal(bounds[:3], v.reshape(-1, 3).min(0)) and np.array_equal(bounds[3:], v.reshape(-1, 3).max(0))
    for ncap, tcap in ((nn - 1, nt), (nn, nt - 1), (0, 0)):
        nodes = np.full((nn, 8), 0xA5A5A5A5, np.uint32); tris = np.full((nt, 12), 0xA5A5A5A5, np.uint32); info2 = np.full(8, 0xA5A5A5A5, np.uint32)
        assert L.mi355rt_debug_bvh_read(None, vp, gp, 37, info2.ctypes.data_as(U), None, nodes.ctypes.data_as(U), ncap, tris.ctypes.data_as(U), tcap) == -1
        assert (nodes == 0xA5A5A5A5).all() and (tris == 0xA5A5A5A5).all() and (info2 == 0xA5A5A5A5).all()          # nothing is written
    nodes = np.zeros((nn, 8), np.uint32); tris = np.zeros((nt, 12), np.uint32)
    assert L.mi355rt_debug_bvh_read(None, vp, gp, 37, info.ctypes.data_as(U), None, nodes.ctypes.data_as(U), nn, None, nt) == -1      # one array without the other
    assert L.mi355rt_debug_bvh_read(None, vp, gp, 37, None, None, None, 0, None, 0) == -1
    assert L.mi355rt_debug_bvh_read(None, None, None, 37, info.ctypes.data_as(U), None, None, 0, None, 0) == -1
    t = pkg.debug_bvh(v, g); t0 = pkg.debug_bvh(v)
    assert np.array_equal(t["nodes"], t0["nodes"]) and np.array_equal(t["tris"][:, 7], g[t["tris"][:, 3]]) and not t0["tris"][:, 7].any()


# ---------------------------------------------------------------------------------------------------- the depth boundary
def test_chain_scenes_have_statement_heights_31_and_32():
    """The two scenes of the depth-limit tests (tests/test_gpu_lbvh_statement.py), chosen HERE from the statement so that the GPU test cannot
    drift off the boundary: one of statement height exactly 31 (the deepest tree the traversal stack serves: built on the device) and one of
    exactly 32 (refused by the device builder).  The construction is what it says: a scene box of exactly [0, 2]^3, the keys 0, the single
    bits 2^m in turn, and 2^63 - 1."""
    S = statement()
    v31, g31, t31 = chain_of_height(31)
    v32, g32, t32 = chain_of_height(32)
    assert t31["max_depth"] == 31 and t32["max_depth"] == 32
    assert v32.shape[0] == v31.shape[0] + 1 and np.array_equal(v32[:-1], v31)
    for v, t in ((v31, t31), (v32, t32)):
        n = v.shape[0]
        assert t["scene_min"].tolist() == [0, 0, 0] and t["scene_max"].tolist() == [2, 2, 2]
        keys = S.morton_keys(v, t["scene_min"], t["scene_max"])
        assert [int(k) for k in keys] == [0, 2 ** 63 - 1] + [1 << m for m in range(n - 2)]
        assert t["order"].tolist() == [0] + list(range(2, n)) + [1]
        facts = S.check_tree(t["nodes"], t["tris"], v, ((np.arange(n) * 7 + 1) % N_GEOM).astype(np.uint32), leaves=n, max_leaf=1)
        assert facts["path_inner"] == t["max_depth"]
    deep, depth = deepest_triangles(t31)
    assert deep.tolist() == [0, 2, 3, 4, 5, 6, 7, 8] and depth.tolist() == [31, 31, 30, 29, 28, 27, 26, 25]
    print("\nchain scenes: %d triangles give height 31, %d give height 32" % (v31.shape[0], v32.shape[0]))


def test_rays_of_the_cases_hit_and_miss(oracle, scenes):
    """the ray sets of the GPU tests do what they are for, by the brute-force oracle alone: at least 10 % hit and at least 10 % miss on every
    case, and at least 64 rays of each chain scene have one of the 8 deepest triangles as their answer"""
    for name in CASE_NAMES:
        orc = brute_oracle(oracle, case_scene(name, scenes))
        _, prim = orc.intersect(case_rays(name, scenes), brute=True)
        share = float((prim != MISS).mean())
        print("\n[%s] oracle hit share %.3f" % (name, share))
        assert 0.1 <= share <= 0.9, name
    for height in (31, 32):
        v, g, tree = chain_of_height(height)
        orc = brute_oracle(oracle, scene_with(scenes, v, g))
        _, prim = orc.intersect(chain_rays(height), brute=True)
        deep, _ = deepest_triangles(tree)
        print("\n[chain of height %d] oracle hit share %.3f, %d rays answer one of the 8 deepest triangles" % (height, float((prim != MISS).mean()), int(np.isin(prim, deep).sum())))
        assert np.isin(prim, deep).sum() >= 64
