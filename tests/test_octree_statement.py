"""The octree build held to an independent statement, without a GPU.

csrc/octree.cpp (the product) and oracle/oracle.c are two restatements of oct_tree_intersector.rs in C by one author; a
shared misreading passes every parity test.  Here a third statement (oracle/octree_statement.py: numpy, written from the
reference's text in another shape) is compared with both, node for node, and the SAT decisions themselves are compared
with exact rational geometry that uses no separating axes.  tests/test_gpu_octree_statement.py holds the device walk to
the same statement, with the rays built here."""
import importlib.util
import os
import sys
import time
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF


def statement():
    name = "octree_statement"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "oracle", "octree_statement.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- hand-made scenes
# Scenes no loader produces.  Each has at most 200 triangles and builds under 50 000 nodes at its leaf size (asserted below).
# The root cube is pinned by two "anchor" triangles that lie IN root faces (z = lo and z = hi), so every scene also has
# triangles in the outermost cube planes.

def _tri(*p):
    return [float(x) for v in p for x in v]


def _anchors(lo=-1.0, hi=1.0, s=0.5):
    return [_tri((lo, lo, lo), (lo + s, lo, lo), (lo, lo + s, lo)), _tri((hi, hi, hi), (hi - s, hi, hi), (hi, hi - s, hi))]


def _in_plane(axis, c, uv):
    """the 2-D points uv put into the plane coordinate[axis] = c"""
    other = [a for a in range(3) if a != axis]
    out = []
    for u, v in uv:
        p = [0.0, 0.0, 0.0]
        p[axis] = c; p[other[0]] = u; p[other[1]] = v
        out.append(tuple(p))
    return out


def scene_face_planes():
    """pairs of overlapping coplanar triangles in the root's mid planes (0), in its children's mid planes (+-0.5, the face planes
    of the grandchildren) and in its face planes (+-1); one pair per plane, so the split runs to level 9 over the overlap"""
    t = _anchors()
    k = 0
    for axis in range(3):
        for c in (0.0, 0.5, -0.5, 1.0, -1.0):
            u0, v0 = -0.83 + 0.11 * k, 0.71 - 0.097 * k
            k += 1
            for du in (0.0, 0.012):
                t.append(_tri(*_in_plane(axis, c, [(u0 + du, v0 + du), (u0 + du + 0.05, v0 + du), (u0 + du, v0 + du + 0.05)])))
    return np.array(t, np.float32), 1


def scene_mid_point_vertex():
    """fans of six triangles around a vertex that lies exactly on the root's mid point, on a child's mid point and on a
    grandchild's; the rim vertices are generic.  Also one fan whose rim lies on grid points too (every vertex a cube corner)."""
    t = _anchors()
    rim = [(0.31, 0.07, 0.12), (0.13, 0.29, -0.08), (-0.17, 0.23, 0.11), (-0.33, -0.05, -0.09), (-0.12, -0.27, 0.14), (0.19, -0.26, -0.13)]
    for c in ((0.0, 0.0, 0.0), (0.5, 0.5, 0.5), (-0.25, 0.25, -0.75)):
        for i in range(6):
            a, b = rim[i], rim[(i + 1) % 6]
            t.append(_tri(c, tuple(c[k] + 0.5 * a[k] for k in range(3)), tuple(c[k] + 0.5 * b[k] for k in range(3))))
    grid = [(0.25, 0.0, 0.0), (0.0, 0.25, 0.0), (-0.25, 0.0, 0.25), (0.0, -0.25, 0.0), (0.0, 0.0, -0.25), (0.25, -0.25, 0.0)]
    c = (-0.5, -0.5, 0.5)
    for i in range(6):
        a, b = grid[i], grid[(i + 1) % 6]
        t.append(_tri(c, tuple(c[k] + a[k] for k in range(3)), tuple(c[k] + b[k] for k in range(3))))
    return np.array(t, np.float32), 3


def scene_zero_area():
    """zero-area triangles, three coincident copies each (so that two per leaf force the split to level 9 around them): collinear
    along a generic direction, collinear along an axis inside a mid plane, two vertices coincident, all three coincident (a point,
    generic and on the root's mid point).  Their normal and some edge axes are the zero vector."""
    t = _anchors()
    t.append(_tri((-0.6, 0.1, 0.2), (0.2, 0.5, -0.3), (0.5, -0.7, 0.4)))           # one ordinary triangle through the middle
    deg = [
        _tri((0.125, 0.25, 0.375), (0.25, 0.3125, 0.328125), (0.375, 0.375, 0.28125)),   # collinear in a generic direction (dyadic: exactly so in f32)
        _tri((-0.7, 0.0, 0.3), (-0.5, 0.0, 0.3), (-0.3, 0.0, 0.3)),                # collinear along x, inside the mid plane y = 0
        _tri((0.4, -0.4, -0.2), (0.4, -0.4, -0.2), (0.62, -0.31, -0.05)),          # v0 == v1
        _tri((-0.3, 0.6, -0.6), (-0.12, 0.71, -0.52), (-0.12, 0.71, -0.52)),       # v1 == v2
        _tri((0.37, 0.61, -0.43), (0.37, 0.61, -0.43), (0.37, 0.61, -0.43)),       # a point, generic
        _tri((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),                   # a point on the root's mid point
        _tri((0.5, 0.5, -0.5), (0.5, 0.25, -0.5), (0.5, 0.75, -0.5)),              # collinear along y on a cube edge, middle vertex first
    ]
    for d in deg:
        t += [d, d, d]
    return np.array(t, np.float32), 2


def scene_nearly_collinear():
    """NOT one of the zero-area scenes, and compared tree against tree only: three vertices that are collinear in decimal and a hair
    off in f32.  The f32 cross product of the two edges is rounding noise, so the reference's normal-axis test separates the triangle
    from cubes it passes through (exact geometry calls those decisions wrong by far more than
    any band).  The product has to drop the triangle from those cubes too: the reference's arithmetic is the semantics."""
    t = _anchors()
    t.append(_tri((-0.6, 0.1, 0.2), (0.2, 0.5, -0.3), (0.5, -0.7, 0.4)))
    t += [_tri((0.11, 0.23, 0.37), (0.21, 0.28, 0.33), (0.31, 0.33, 0.29))] * 3
    return np.array(t, np.float32), 2


def scene_coincident_copies():
    """80 coincident copies of one triangle at 70 per leaf: every cube the triangle meets holds all 80, down to level 9.  A
    backdrop triangle behind it and the anchors in the root's faces give the rays something else to hit."""
    t = _anchors()
    t.append(_tri((-0.9, -0.8, 0.6), (0.9, -0.7, 0.7), (0.1, 0.9, 0.55)))
    one = _tri((0.13, 0.07, -0.11), (0.33, 0.12, -0.02), (0.19, 0.29, 0.05))
    t += [one] * 80
    return np.array(t, np.float32), 70


_PERMS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))


def scene_corner_slivers():
    """Triangles that pass a cube's edge outside it: they overlap the cube's bounding slabs, their plane cuts the cube, and only
    an edge axis separates them.  In the frame of the cube [0,1]^3 the edge (0.7, 1.5) - (1.5, 0.7) runs outside the cube edge
    x = y = 1; the third vertex is either far (a broad triangle: only that edge's axis rejects) or close (a sliver).  Every
    rotation of the vertex order (which of edge 1, 2, 3 it is), every cyclic permutation of the coordinates (which cube axis
    the edge axis is made with) and all 8 mirror images: the target cubes are the grandchildren of the root [-2, 2]^3 that touch
    its centre."""
    t = _anchors(-2.0, 2.0, 0.25)
    for mirror in range(8):
        sg = [(-1.0 if (mirror >> a) & 1 else 1.0) for a in range(3)]
        for perm in _PERMS:
            for rot in range(3):
                h = 0.31 + 0.07 * rot + 0.05 * perm[0]
                broad = [(1.5, 0.7, h), (0.7, 1.5, h + 0.02), (1.9, 1.85, h + 0.9)]
                sliver = [(1.46, 0.66, h + 0.3), (0.66, 1.46, h + 0.33), (1.42, 0.62, h + 0.36)]
                for tri3 in (broad, sliver):
                    tri3 = tri3[rot:] + tri3[:rot]
                    pts = []
                    for p in tri3:
                        q = [0.0, 0.0, 0.0]
                        for a in range(3):
                            q[perm[a]] = sg[perm[a]] * p[a]
                        pts.append(tuple(q))
                    t.append(_tri(*pts))
    return np.array(t, np.float32), 4


def scene_flat():
    """every vertex at z = 0.25: the root and all its descendants have zero thickness in z, the lower and the upper children
    are the same squares and both hold every triangle of their square"""
    t = []
    n = 6
    for i in range(n):
        for j in range(n):
            x0, y0 = -1.0 + 2.0 * i / n, -1.0 + 2.0 * j / n
            x1, y1 = -1.0 + 2.0 * (i + 1) / n, -1.0 + 2.0 * (j + 1) / n
            t.append(_tri((x0, y0, 0.25), (x1, y0, 0.25), (x0, y1, 0.25)))
            if (i + j) % 2:
                t.append(_tri((x1, y1, 0.25), (x0 + 0.07, y1, 0.25), (x1, y0 + 0.05, 0.25)))
    return np.array(t, np.float32), 12


def scene_far():
    """a unit-size scene centred 1 000 times its size from the origin; vertices on a 1/64 grid, so that they are f32 values"""
    rng = np.random.default_rng(20240611)
    c = np.array([1000.0, -1000.0, 1000.0])
    t = []
    for a in _anchors(-0.5, 0.5, 0.25):
        t.append(a)
    for _ in range(60):
        p = rng.integers(-28, 29, 3) / 64.0
        t.append(_tri(*[tuple(np.clip(p + rng.integers(-10, 11, 3) / 64.0, -0.5, 0.5)) for _ in range(3)]))
    v = np.array(t, np.float64).reshape(-1, 3) + c
    return v.reshape(-1, 9).astype(np.float32), 4


HANDMADE = {"face_planes": scene_face_planes, "mid_point_vertex": scene_mid_point_vertex, "zero_area": scene_zero_area,
            "coincident_copies": scene_coincident_copies, "corner_slivers": scene_corner_slivers, "flat": scene_flat, "far": scene_far, "nearly_collinear": scene_nearly_collinear}


def handmade_leaf_size(name):
    return HANDMADE[name]()[1]


def scene_of(name, scenes):
    """a golden scene, or a hand-made one with the materials, the light and the camera of 4boxes"""
    if name not in HANDMADE:
        return scenes(name)
    sc = dict(scenes("4boxes"))
    tv, _ = HANDMADE[name]()
    sc["tri_verts"] = tv
    sc["tri_geom"] = np.zeros(tv.shape[0], np.uint32)
    return sc


GOLDEN_CASES = [("4boxes", 70), ("4boxes", 5), ("4boxes", 1), ("ico2", 70), ("ico2", 8), ("ico2", 1), ("ico3_tex", 70), ("thai2", 70)]
CASES = GOLDEN_CASES + [(n, handmade_leaf_size(n)) for n in HANDMADE]
HANDMADE_C = [n for n in HANDMADE if n != "nearly_collinear"]      # the scenes the exact-geometry test runs on

_trees = {}


def _give_memory_back():
    """The builds of the big cases free some hundred MB in small pieces, which the C library keeps for reuse.  Hand them back to the system:
    tests that run later measure the size of child processes, and a child starts out with the size of the process that made it."""
    import ctypes
    import gc
    gc.collect()
    trim = getattr(ctypes.CDLL(None), "malloc_trim", None)
    if trim is not None:
        trim(0)


@pytest.fixture(scope="module", autouse=True)
def _shared_results_end_with_the_module():
    """the trees and walks that the tests of this module share are dropped when the module is done.  tests/test_gpu_octree_statement.py
    borrows them through statement_walk() / tie_walk(), which compute what is missing: in whichever order the two modules run, the results
    are the same, and only the sharing is lost"""
    yield
    _trees.clear(); _walks.clear(); del _tie_walk[:]
    _give_memory_back()


def statement_tree(name, tpl, scenes):
    """the statement's tree of a case, left unchanged.  Built once per session for the cases that several tests use; the others (the big
    trees of the node-for-node comparison) are not kept, so that the test process does not stay large for the rest of the suite."""
    if (name, tpl) in _trees:
        return _trees[(name, tpl)]
    tree = statement().build(scene_of(name, scenes)["tri_verts"], tpl, keep_decisions=(name, tpl) in SHARED_CASES)
    if (name, tpl) in SHARED_CASES:
        _trees[(name, tpl)] = tree
    return tree


# ---------------------------------------------------------------------------------------------------- (a) three trees
@pytest.mark.parametrize("name,tpl", CASES, ids=["%s-%d" % c for c in CASES])
def test_three_trees_node_for_node(pkg, oracle, scenes, name, tpl):
    """product (mi355rt_debug_octree), oracle (oracle_octree_dump) and statement: the same cubes bit for bit, the same child
    indices, the same leaf lists in order, the same parent links, and the counters of mi355rt_octree_stats as the statement counts them"""
    sc = scene_of(name, scenes)
    t0 = time.time()
    T = statement_tree(name, tpl, scenes)
    secs = time.time() - t0
    n = T.cubes.shape[0]
    print("\n[%s at %d] %d triangles, %d nodes, %d decisions, statement build %.2f s" % (name, tpl, sc["tri_verts"].shape[0], n, T.n_decisions, secs))
    if name in HANDMADE:
        assert sc["tri_verts"].shape[0] <= 200 and n < 50000
    inner = T.children[:, 0] >= 0
    assert np.array_equal(T.children[inner], T.children[inner, :1] + np.arange(8)), "children are not consecutive in the statement"
    st = T.stats()
    # the product: cubes by bit pattern; the flat form has the first child and promises first .. first + 7; leaf lists in order; parent links; counters
    P = pkg.debug_octree(sc["tri_verts"], tpl)
    assert P["cubes"].shape[0] == n
    assert np.array_equal(bits(P["cubes"]), bits(T.cubes)), "product cubes"
    assert np.array_equal(P["first_child"], T.children[:, 0]), "product first_child"
    assert np.array_equal(P["tri_count"][~inner], T.leaf_count[~inner])
    assert np.array_equal(P["leaf_tris"], T.leaf_tris), "product leaf lists"
    assert np.array_equal(P["tri_first"][~inner], T.leaf_first[~inner])
    assert np.array_equal(P["parent"], T.parent), "product parents"
    assert P["stats"] == {k: st[k] for k in ("nodes", "inner", "leaves", "empty", "depth", "tri_refs")}
    del P
    # the oracle: cubes by bit pattern, all 8 child indices, leaf lists in order, counters
    orc = oracle.Oracle(sc, 8, 8, tris_per_leaf=tpl)
    D = orc.octree_dump()
    assert D["cubes"].shape[0] == n
    assert np.array_equal(bits(D["cubes"]), bits(T.cubes)), "oracle cubes"
    assert np.array_equal(D["children"], T.children), "oracle children"
    assert np.array_equal(D["leaf_count"], T.leaf_count)
    assert np.array_equal(D["leaf_tris"], T.leaf_tris), "oracle leaf lists"
    assert np.array_equal(D["leaf_first"][~inner], T.leaf_first[~inner])
    assert orc.octree_stats() == st
    orc.close()
    del T, D
    _give_memory_back()


def test_debug_octree_size_query_and_short_buffers(pkg, scenes):
    """the size query writes the counters only; a buffer that is too small gets MI355RT_E_INVALID and nothing is written"""
    import ctypes as C
    v = np.ascontiguousarray(scenes("4boxes")["tri_verts"], np.float32)
    L = pkg.lib()
    F, U, I = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    counts = np.zeros(8, np.uint32)
    assert L.mi355rt_debug_octree(v.ctypes.data_as(F), v.shape[0], 5, counts.ctypes.data_as(U), None, None, None, None, None, 0, None, 0) == 0
    n, refs = int(counts[0]), int(counts[5])
    assert (n, refs) == (161, 372)
    for ncap, lcap in ((n - 1, refs), (n, refs - 1)):
        counts2 = np.full(8, 77, np.uint32)
        cubes = np.full((n, 6), 7.0, np.float32); fc = np.full(n, 7, np.int32)
        a = [np.full(n, 7, np.uint32) for _ in range(3)]; lt = np.full(refs, 7, np.uint32)
        code = L.mi355rt_debug_octree(v.ctypes.data_as(F), v.shape[0], 5, counts2.ctypes.data_as(U), cubes.ctypes.data_as(F), fc.ctypes.data_as(I),
                                      a[0].ctypes.data_as(U), a[1].ctypes.data_as(U), a[2].ctypes.data_as(U), ncap, lt.ctypes.data_as(U), lcap)
        assert code == -1
        assert (counts2 == 77).all() and (cubes == 7.0).all() and (fc == 7).all() and all((x == 7).all() for x in a) and (lt == 7).all()
    assert L.mi355rt_debug_octree(v.ctypes.data_as(F), v.shape[0], 5, None, None, None, None, None, None, 0, None, 0) == -1
    # some arrays but not all: refused
    cubes = np.zeros((n, 6), np.float32)
    assert L.mi355rt_debug_octree(v.ctypes.data_as(F), v.shape[0], 5, counts.ctypes.data_as(U), cubes.ctypes.data_as(F), None, None, None, None, n, None, refs) == -1


# ---------------------------------------------------------------------------------------------------- (b) exact geometry
def classify_against_exact_geometry(T, tv, sample=None, seed=0):
    """Every (triangle, child cube) decision of the build against exact closed overlap, with delta = 1e-5 x the scene's diagonal.
    Returns dict(decisions, checked, outside, wrong_outside: [(tri, node, member)], band_differ).  Identical (triangle
    coordinates, cube) pairs are decided once.  The cube is shrunk along the axes in which it has extent: a cube of zero thickness
    (every cube of the flat scene) shrunk along that axis would be empty, and no member of such a cube would ever be checked.  Along
    such an axis the inner cube keeps the plane itself."""
    S = statement()
    tri, node, member = T.decisions
    lo, hi = T.cubes[0, :3].astype(np.float64), T.cubes[0, 3:].astype(np.float64)
    diag = Fraction(float(np.sqrt(((hi - lo) ** 2).sum())))
    delta = diag / 100000
    idx = np.arange(tri.size)
    if sample is not None and sample < tri.size:
        idx = np.sort(np.random.default_rng(seed).choice(tri.size, sample, replace=False))
    seen = {}
    outside = 0; wrong = []; band_differ = 0
    for i in idx:
        key = (tv[tri[i]].tobytes(), T.cubes[node[i]].tobytes())
        if key not in seen:
            c = T.cubes[node[i]]
            cmin = [Fraction(float(x)) for x in c[:3]]; cmax = [Fraction(float(x)) for x in c[3:]]
            thick = [cmax[a] > cmin[a] for a in range(3)]
            inner = S.exact_overlap([x + delta if k else x for x, k in zip(cmin, thick)], [x - delta if k else x for x, k in zip(cmax, thick)],
                                    tv[tri[i]])                                                       # a shrunk cube that is empty overlaps nothing
            outer = inner or S.exact_overlap([x - delta for x in cmin], [x + delta for x in cmax], tv[tri[i]])
            exact = inner or (outer and S.exact_overlap(cmin, cmax, tv[tri[i]]))
            seen[key] = (inner, outer, exact)
        inner, outer, exact = seen[key]
        if inner or not outer:
            outside += 1
            if bool(member[i]) != inner:
                wrong.append((int(tri[i]), int(node[i]), bool(member[i])))
        elif bool(member[i]) != exact:
            band_differ += 1
    return dict(decisions=int(tri.size), checked=int(idx.size), outside=outside, wrong_outside=wrong, band_differ=band_differ)


# (scene, leaf size, required share outside the band, sample): every decision is checked except on ico2, where a fixed-seed sample is
EXACT_CASES = [("4boxes", 5, 0.75, None), ("ico2", 70, 0.95, 6000)] + [(n, handmade_leaf_size(n), None, None) for n in HANDMADE_C]
SHARED_CASES = set(c[:2] for c in EXACT_CASES) | {("4boxes", 5), ("ico2", 8), ("ico2", 70)}      # with WALK_CASES below: the trees more than one test uses


@pytest.mark.parametrize("name,tpl,share,sample", EXACT_CASES, ids=["%s-%d" % c[:2] for c in EXACT_CASES])
def test_sat_decisions_against_exact_geometry(scenes, name, tpl, share, sample):
    """A triangle that overlaps the child cube shrunk by delta must be a member; one that does not overlap the cube grown by delta
    must not be; in between f32 rounding may decide.  The share of decisions outside that band is asserted where the issue sets it
    (4boxes at 5: at least 75 %, ico2 at 70: at least 95 %).

    Every decision of the build is checked, except on ico2 at 70, where a fixed-seed sample of 6 000 of the 19 656 is.  The remark
    that the shrunk cube is never empty does not hold for the flat scene, whose cubes have no thickness in z: there the cube is shrunk
    in x and y only (classify_against_exact_geometry), so that its members are checked too.

    Outside the band: 4boxes at 5: 1 239 of 1 552; ico2 at 70: 5 860 of the 6 000 sampled; face_planes 8 547 of 13 032;
    mid_point_vertex 9 874 of 11 576; zero_area 25 916 of 31 368; coincident_copies 645 875 of 654 760; corner_slivers 16 386 of
    16 432; flat 1 586 of 1 824; far 1 989 of 2 064.  No decision outside the band contradicts geometry on any of them.
    In-band decisions that differ from exact closed overlap: 29 on mid_point_vertex, 1 on zero_area, 0 on 4boxes, ico2 (in the
    sample) and the other hand-made scenes - a fact about the reference's arithmetic on these scenes, not a requirement.
    (A triangle that is only NEARLY collinear is decided against geometry far outside the band: scene_nearly_collinear, which is
    why that scene is not one of the zero-area scenes here.)"""
    sc = scene_of(name, scenes)
    T = statement_tree(name, tpl, scenes)
    tv = np.ascontiguousarray(sc["tri_verts"], np.float32).reshape(-1, 9)
    t0 = time.time()
    r = classify_against_exact_geometry(T, tv, sample=sample, seed=1)
    print("\n[%s at %d] decisions %d, checked %d, outside the band %d, in the band %d, in-band decisions that differ from exact overlap %d (%.1f s)"
          % (name, tpl, r["decisions"], r["checked"], r["outside"], r["checked"] - r["outside"], r["band_differ"], time.time() - t0))
    assert r["checked"] == (r["decisions"] if sample is None else sample) and r["checked"] >= min(r["decisions"], 5000)
    assert not r["wrong_outside"], "SAT decisions that contradict exact geometry outside the band (triangle, node, member): %r" % r["wrong_outside"][:10]
    if share is not None:
        assert r["outside"] >= share * r["checked"]


def test_corner_slivers_hang_on_each_edge_axis(scenes):
    """the corner-sliver scene does what it was made for: for each of the nine edge axes there are decisions of its build in which
    that axis alone separates triangle and cube (so leaving it out, or taking it with a wrong operand, changes the tree), and
    non-members that overlap all three bounding slabs of the cube"""
    S = statement()
    name = "corner_slivers"
    T = statement_tree(name, handmade_leaf_size(name), scenes)
    tv = scene_of(name, scenes)["tri_verts"]
    tri, node, member = T.decisions
    sep = S.triangle_cube_intersection(T.cubes[node, :3], T.cubes[node, 3:], tv[tri], per_axis=True)
    assert np.array_equal(~sep.any(axis=1), member)
    alone = sep.sum(axis=1) == 1
    counts = [int((alone & sep[:, 4 + k]).sum()) for k in range(9)]
    print("\n[corner_slivers] decisions where one edge axis alone separates:", counts, "; rejected by edge axes only:", int((~sep[:, :4].any(axis=1) & ~member).sum()))
    assert min(counts) >= 4
    assert (~sep[:, :4].any(axis=1) & ~member).sum() >= 100


# ---------------------------------------------------------------------------------------------------- the rays of the walk tests
def _feature_points(cube):
    """the 26 corners, edge mid points and face centres of a cube, f32; the mid coordinate as the build computes it"""
    lo, hi = cube[:3], cube[3:]
    mid = np.float32(0.5) * (hi + lo)
    g = np.stack([lo, mid, hi])
    pts = [(g[i, 0], g[j, 1], g[k, 2]) for i in range(3) for j in range(3) for k in range(3) if (i, j, k) != (1, 1, 1)]
    return np.array(pts, np.float32)


def statement_rays(T, tri_verts, seed, budget=4096, tags=None):
    """At most `budget` rays built from the statement's own cubes:
      A  origins and targets on faces, edges and corners of cubes of every level that exists;
      B  rays along the space diagonals through a node's centre (several children have the same t: only the stable order decides);
      C  origins inside leaves, towards points of the root and away from it;
      D  origins on triangle vertices;
      E  one or two zero direction components, the origin on no cube plane of that axis;
      F  targets where a triangle's edge crosses a face of its leaf's cube (the hit point lies on a cube face);
      G  targets on the root's faces where triangles touch them: the vertices that pin the extents, and points of edges that lie
         in a root face.  The f32 hit point pos + dir * t falls a last bit outside the root for about half of these, no leaf
         contains it, and the octree answer is not the true closest hit (the only way the two differ in a closed scene);
      H  rays from outside the root that enter it through a triangle lying in a root face, at a point that also lies on a cube
         plane of a descendant.  The children on both sides of that plane then have the same t, the f32 hit point lies in one of
         them only, and where the other holds a farther triangle only the STABLE order of the sort gives the reference's answer.
    No ray has a zero direction component with its origin on a cube plane of that axis (0 * inf: the NaN rule)."""
    rng = np.random.default_rng(seed)
    tv = np.ascontiguousarray(tri_verts, np.float32).reshape(-1, 9)
    cubes = T.cubes
    lo, hi = cubes[0, :3].astype(np.float64), cubes[0, 3:].astype(np.float64)
    ext = np.where(hi > lo, hi - lo, 1.0)
    leafm = T.children[:, 0] < 0
    full = np.nonzero(leafm & (T.leaf_count > 0))[0]
    levels = np.unique(T.level)
    q = budget // 8
    rays = []
    kinds = []

    def pick(pool, k):
        return pool[rng.integers(0, pool.size, k)]

    def root_point(k):
        return lo + (hi - lo) * rng.random((k, 3))

    def inside(nodes):
        c = cubes[nodes].astype(np.float64)
        return c[:, :3] + (c[:, 3:] - c[:, :3]) * (0.05 + 0.9 * rng.random((nodes.size, 3)))

    def add(org, tgt=None, dir_=None, tag="?"):
        org = np.asarray(org, np.float32).reshape(-1, 3)
        kinds.append(np.full(org.shape[0], tag))
        d = (np.asarray(tgt, np.float32).reshape(-1, 3) - org) if dir_ is None else np.asarray(dir_, np.float32).reshape(-1, 3)
        rays.append(np.concatenate([org, d.astype(np.float32)], axis=1))

    # A: per level the same number of rays; the other end on a cube of any level (the root included)
    per = max(q // levels.size, 8)
    for l in levels:
        pool = np.nonzero(T.level == l)[0]
        a = pick(pool, per); b = pick(np.arange(cubes.shape[0]), per); b[::3] = 0
        pa = np.stack([_feature_points(cubes[n])[rng.integers(26)] for n in a])
        pb = np.stack([_feature_points(cubes[n])[rng.integers(26)] for n in b])
        stretch = np.where(rng.random(per) < 0.5, 1.0, 2.5)[:, None].astype(np.float32)      # a target on the cube, or the cube half way
        add(pa, dir_=(pb - pa) * stretch, tag="A")
    # B: the four space diagonals of nodes of every level, from outside the cube, from its boundary, from half way and from the centre
    nodes = np.concatenate([pick(np.nonzero(T.level == l)[0], max(q // (8 * levels.size), 2)) for l in levels])
    for n in nodes:
        c = cubes[n]
        mid = np.float32(0.5) * (c[3:] + c[:3]); half = c[3:] - mid
        for s in range(8):
            sg = np.array([(-1.0 if (s >> a) & 1 else 1.0) for a in range(3)], np.float32)
            d = half * sg
            k = np.float32((2.0, 1.0, 0.5, 0.0)[(s + n) % 4])
            add(mid - d * k, dir_=d * np.float32(2.0), tag="B")
    # C: origins inside leaves
    lv = pick(np.nonzero(leafm)[0], q // 2)
    add(inside(lv), tgt=root_point(lv.size), tag="C")
    lv = pick(full if full.size else np.nonzero(leafm)[0], q // 2)
    o = inside(lv)
    add(o, tgt=np.where(rng.random((lv.size, 1)) < 0.5, o + (o - 0.5 * (lo + hi)) * 4.0 + ext * (rng.random((lv.size, 3)) - 0.5), inside(pick(full, lv.size)) if full.size else root_point(lv.size)), tag="C")
    # D: origins on triangle vertices
    t = rng.integers(0, tv.shape[0], q)
    v = tv[t].reshape(-1, 3, 3)[np.arange(q), rng.integers(0, 3, q)]
    other = tv[rng.integers(0, tv.shape[0], q)].reshape(-1, 3, 3)[np.arange(q), rng.integers(0, 3, q)]
    add(v, tgt=np.where(rng.random((q, 1)) < 0.5, other.astype(np.float64), root_point(q)), tag="D")
    # E: zero direction components
    o = root_point(q).astype(np.float32)
    d = ((rng.random((q, 3)) - 0.5) * ext * 3.0).astype(np.float32)
    zero = np.zeros((q, 3), bool)
    zero[np.arange(q), rng.integers(0, 3, q)] = True
    second = rng.random(q) < 0.5
    zero[np.arange(q)[second], rng.integers(0, 3, int(second.sum()))] = True
    d[zero] = 0.0
    d[np.arange(q)[::7], :] = np.where(zero[::7], np.float32(-0.0), d[::7])                  # some of the zeros are -0: 1 / -0 = -inf
    add(o, dir_=d, tag="E")
    # F: hit points on cube faces
    tgt = []
    for n in (pick(full, 4 * q) if full.size else []):
        if len(tgt) == q:
            break
        lst = T.leaf(n)
        tri3 = tv[lst[rng.integers(lst.size)]].reshape(3, 3).astype(np.float64)
        e = rng.integers(3)
        p0, p1, third = tri3[e], tri3[(e + 1) % 3], tri3[(e + 2) % 3]
        c = cubes[n].astype(np.float64)
        crossed = [(a, plane) for a in range(3) for plane in (c[a], c[3 + a]) if (p0[a] - plane) * (p1[a] - plane) < 0]
        if not crossed:
            continue
        a, plane = crossed[rng.integers(len(crossed))]
        p = p0 + (plane - p0[a]) / (p1[a] - p0[a]) * (p1 - p0)
        p[a] = plane
        tgt.append(p if rng.random() < 0.5 else p + (0.02 + 0.3 * rng.random()) * (third - p))      # on the edge, or a little way into the triangle
    if tgt:
        tgt = np.array(tgt); k = tgt.shape[0]
        o = np.where(rng.random((k, 1)) < 0.7, root_point(k), 0.5 * (lo + hi) + (rng.random((k, 3)) - 0.5) * ext * 2.6)
        add(o, dir_=(tgt - o) * np.where(rng.random((k, 1)) < 0.7, 2.0, 0.75), tag="F")
    # G: hit points on the root's faces
    tri3 = tv.reshape(-1, 3, 3)
    tgt = []
    on = [(t, k, a) for a in range(3) for plane in (cubes[0, a], cubes[0, 3 + a]) for t, k in zip(*np.nonzero(tri3[:, :, a] == plane))]
    for i in rng.integers(0, len(on), q):
        t, k, a = on[i]
        p = tri3[t, k].astype(np.float64)
        mates = [m for m in range(3) if m != k and tri3[t, m, a] == tri3[t, k, a]]
        if mates and rng.random() < 0.7:                                                        # along an edge that lies in the face
            p = p + rng.random() * (tri3[t, mates[rng.integers(len(mates))]].astype(np.float64) - p)
        tgt.append(p)
    tgt = np.array(tgt)
    o = np.where(rng.random((q, 1)) < 0.7, root_point(q), 0.5 * (lo + hi) + (rng.random((q, 3)) - 0.5) * ext * 2.6)
    add(o, dir_=(tgt - o) * np.where(rng.random((q, 1)) < 0.7, 2.0, 0.75), tag="G")
    # H: entering the root through a triangle in a root face, on a descendant's cube plane
    org, tgt = [], []
    flat_in = [(t, a, side) for a in range(3) for side in (0, 1) for t in np.nonzero((tri3[:, :, a] == cubes[0, 3 * side + a]).all(axis=1))[0]]
    planes = [np.unique(np.concatenate([cubes[:, a], cubes[:, 3 + a]])).astype(np.float64) for a in range(3)]
    for i in (rng.integers(0, len(flat_in), 6 * q) if flat_in and (hi > lo).all() else []):
        if len(tgt) == q:
            break
        t, a, side = flat_in[i]
        w = rng.dirichlet((1.0, 1.0, 1.0))
        p = (w[:, None] * tri3[t].astype(np.float64)).sum(axis=0)
        b = [x for x in range(3) if x != a][rng.integers(2)]
        near = planes[b][np.argsort(np.abs(planes[b] - p[b]))[:4]]                               # onto one of the nearest planes of that axis
        p[b] = near[rng.integers(near.size)]; p[a] = cubes[0, 3 * side + a]
        e = tri3[t].astype(np.float64)
        m = np.linalg.solve(np.stack([e[1] - e[0], e[2] - e[0], np.eye(3)[a]], axis=1), p - e[0])
        if m[0] < 0.02 or m[1] < 0.02 or m[0] + m[1] > 0.98:
            continue                                                                            # the moved point left the triangle
        out = np.zeros(3); out[a] = 1.0 if side else -1.0
        org.append(p + out * ext[a] * (0.2 + rng.random()) + (rng.random(3) - 0.5) * ext * 1.5 * (1.0 - np.abs(out)))
        tgt.append(p)
    if tgt:
        org = np.array(org); tgt = np.array(tgt)
        add(org, dir_=(tgt - org) * 2.0, tag="H")
    rays = np.concatenate(rays).astype(np.float32)
    # the NaN rule: no zero direction component with the origin on a cube plane of that axis; and no null direction
    keep = np.ones(rays.shape[0], bool)
    for a in range(3):
        planes = np.unique(np.concatenate([cubes[:, a], cubes[:, 3 + a]]))
        keep &= ~((rays[:, 3 + a] == 0) & np.isin(rays[:, a], planes))
    keep &= (rays[:, 3:] != 0).any(axis=1)
    rays = rays[keep]; kinds = np.concatenate(kinds)[keep]
    if rays.shape[0] > budget:
        sel = np.sort(rng.choice(rays.shape[0], budget, replace=False))
        rays = rays[sel]; kinds = kinds[sel]
    if tags is not None:
        tags.extend(kinds)
    return np.ascontiguousarray(rays)


WALK_CASES = [("4boxes", 5), ("ico2", 8), ("ico2", 70), ("coincident_copies", 70), ("corner_slivers", 4)]
WALK_BUDGET = {"coincident_copies": 2048}      # rays per case, 4 096 unless listed: the statement's walk of a case is to take a few seconds
_walks = {}


def statement_walk(name, tpl, scenes):
    """(rays, tuv, prim, blocked, seconds) of a walk case: the statement's answers, computed once per session"""
    if (name, tpl) not in _walks:
        S = statement()
        sc = scene_of(name, scenes)
        T = statement_tree(name, tpl, scenes)
        rays = statement_rays(T, sc["tri_verts"], seed=1000 + tpl, budget=WALK_BUDGET.get(name, 4096))
        t0 = time.time()
        tuv, prim = S.intersect(T, sc["tri_verts"], rays)            # raises where the reference would panic
        secs = time.time() - t0
        _walks[(name, tpl)] = (rays, tuv, prim, S.occluded_from_hits(tuv, prim), secs)
    return _walks[(name, tpl)]


@pytest.mark.parametrize("name,tpl", WALK_CASES, ids=["%s-%d" % c for c in WALK_CASES])
def test_walk_rays_cover_what_they_are_for(scenes, name, tpl):
    """the rays of the GPU walk tests, checked where no GPU is needed: at most 4 096, the statement raises on none of them, hits and
    misses and occluded and free rays are at least 5 % each, and occluded() is the predicate on intersect()'s hit"""
    S = statement()
    rays, tuv, prim, blocked, secs = statement_walk(name, tpl, scenes)
    n = rays.shape[0]
    hit = prim != MISS
    print("\n[%s at %d] %d rays, %d hits, %d occluded, statement walk %.1f s" % (name, tpl, n, int(hit.sum()), int(blocked.sum()), secs))
    budget = WALK_BUDGET.get(name, 4096)
    assert 0.7 * budget <= n <= budget
    assert min(hit.sum(), (~hit).sum()) >= 0.05 * n
    assert min(blocked.sum(), (blocked == 0).sum()) >= 0.05 * n
    zeros = (rays[:, 3:] == 0).sum(axis=1)
    assert (zeros == 1).sum() >= budget // 40 and (zeros == 2).sum() >= budget // 40
    sub = rays[::16]
    assert np.array_equal(S.occluded(statement_tree(name, tpl, scenes), scene_of(name, scenes)["tri_verts"], sub), blocked[::16])


# ---------------------------------------------------------------------------------------------------- (d) statement walk == oracle walk
@pytest.mark.parametrize("name,tpl", [("4boxes", 5), ("ico2", 8)], ids=["4boxes-5", "ico2-8"])
def test_statement_walk_equals_oracle_walk(oracle, scenes, name, tpl):
    """triangle, t, u and v bit for bit on the rays of the GPU walk tests: a disagreement found on the GPU is then the device's"""
    rays, tuv, prim, blocked, _ = statement_walk(name, tpl, scenes)
    orc = oracle.Oracle(scene_of(name, scenes), 8, 8, tris_per_leaf=tpl)
    otuv, oprim = orc.intersect(rays)
    assert np.array_equal(oprim, prim), "triangles differ for %d rays, first %r" % (int((oprim != prim).sum()), np.nonzero(oprim != prim)[0][:8])
    m = prim != MISS
    assert np.array_equal(bits(otuv[m]), bits(tuv[m]))
    # and the rays exercise the semantics: the true closest hit differs somewhere
    _, bprim = orc.intersect(rays, brute=True)
    print("\n[%s at %d] rays whose octree answer is not the true closest hit: %d of %d" % (name, tpl, int((bprim != prim).sum()), rays.shape[0]))
    assert (bprim != prim).sum() > 0


# ---------------------------------------------------------------------------------------------------- the stable order
# Children of equal t are tied only where a ray enters their parent on the boundary between them, and the order among them changes the
# answer only where the f32 hit point falls into one of them and the other holds a farther triangle: about one ray in 3 000 of
# statement_rays() on 4boxes at 5, none found on ico2.  So the rays on which the order decides are recorded: tests/golden/
# octree_tie_rays_4boxes_5.npy holds 48 of them; tests/golden/make_octree_tie_rays.py is its generator.
TIE_RAYS = os.path.join(ROOT, "tests", "golden", "octree_tie_rays_4boxes_5.npy")


_tie_walk = []


def tie_walk(scenes):
    """(rays, tuv, prim) of the recorded rays: the statement's answers, computed once per session"""
    if not _tie_walk:
        rays = np.load(TIE_RAYS)
        sc = scenes("4boxes")
        _tie_walk.append((rays,) + statement().intersect(statement_tree("4boxes", 5, scenes), sc["tri_verts"], rays))
    return _tie_walk[0]


def test_stable_order_decides_on_the_recorded_rays(oracle, scenes):
    """on every recorded ray a walk that takes children of equal t in the other order answers differently, and the oracle's walk
    equals the statement's stable one bit for bit"""
    S = statement()
    rays, tuv, prim = tie_walk(scenes)
    sc = scenes("4boxes")
    assert rays.shape == (48, 6) and not (rays[:, 3:] == 0).any()
    r_tuv, r_prim = S.intersect(statement_tree("4boxes", 5, scenes), sc["tri_verts"], rays, reverse_ties=True)
    assert ((r_prim != prim) | (bits(r_tuv) != bits(tuv)).any(axis=1)).all()
    otuv, oprim = oracle.Oracle(sc, 8, 8, tris_per_leaf=5).intersect(rays)
    assert np.array_equal(oprim, prim)
    m = prim != MISS
    assert m.sum() >= 40 and np.array_equal(bits(otuv[m]), bits(tuv[m]))
