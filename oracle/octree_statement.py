"""octree_statement.py — a third statement of the reference's OctTreeIntersector, in numpy.

TEST INFRASTRUCTURE ONLY, like the rest of oracle/: nothing under raytracer-rs_amd/ (the product) and not
bench.py may import this file.  numpy only: no ctypes, and nothing here looks at oracle.c or at the product.

Why it exists: csrc/octree.cpp and oracle.c are two restatements of oct_tree_intersector.rs in C with the
same structure; a shared misreading passes every parity test.  This one is written from the reference's text
in another shape:
  - the build works on whole LEVELS (all (triangle, child cube) decisions of a level in one array) and
    numbers the nodes afterwards;
  - the walk works on whole RAY SETS per node, not on one ray at a time;
  - every f32 rounding is explicit: all arithmetic is on np.float32 arrays, one numpy operation per reference
    operation, so each product, sum and difference rounds once to f32 and nothing is fused.

Citations are relative to raytracer_lib/src of the reference:
  OCT = raytracer/accel_intersect/oct_tree_intersector.rs, INT = raytracer/intersect.rs,
  MOD = raytracer/mod.rs, VEC = vecmath.rs.

exact_overlap() is independent of all of the above: closed triangle/box overlap in exact rational
arithmetic by clipping, with no separating axes.
"""
from fractions import Fraction

import numpy as np

F32 = np.float32
F32_MAX = F32(np.finfo(np.float32).max)      # std::f32::MAX
F32_MIN = F32(-np.finfo(np.float32).max)     # std::f32::MIN (the most negative finite value)
F32_EPSILON = F32(np.finfo(np.float32).eps)  # std::f32::EPSILON
MISS = 0xFFFFFFFF
MAX_SPLIT_LEVEL = 8                          # OCT:108: a leaf is split while recurse_level <= 8
_CHUNK = 1 << 16                             # decisions per SAT call (bounds the temporaries)


# ------------------------------------------------------------------------------------------- VEC
def _dot(a, b):
    """VEC:74-76: v0.x*v1.x + v0.y*v1.y + v0.z*v1.z, left to right; a, b: (x, y, z) tuples of f32 arrays"""
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    """VEC:79-85"""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _project(points, axis):
    """OCT:460-469 project_points_on_axis.  Starts from f32::MAX / f32::MIN; Rust's f32::min / f32::max return the
    other operand when one is NaN: np.fmin / np.fmax (np.minimum would hand the NaN on)."""
    lo = np.full(np.shape(_dot(axis, points[0])), F32_MAX, F32)
    hi = np.full(lo.shape, F32_MIN, F32)
    for p in points:
        val = _dot(axis, p)
        lo = np.fmin(lo, val)
        hi = np.fmax(hi, val)
    return lo, hi


# ------------------------------------------------------------------------------------------- SAT
def triangle_cube_intersection(cmin, cmax, tri, per_axis=False):
    """OCT:393-458 for n (cube, triangle) pairs at once.  cmin, cmax: (n, 3) f32; tri: (n, 9) f32.  Returns bool (n,).
    The reference returns at the first separating axis; evaluating all 13 and combining them is the same decision.
    per_axis=True: returns instead bool (n, 13), which axes separate, in the reference's order (x, y, z, the normal, then
    edge 1 x X, Y, Z, edge 2 x X, Y, Z, edge 3 x X, Y, Z) - for tests that ask which axis a decision hangs on."""
    cmin = np.asarray(cmin, F32); cmax = np.asarray(cmax, F32); tri = np.asarray(tri, F32)
    n = tri.shape[0]
    one = np.ones(n, F32); zero = np.zeros(n, F32)
    x_axis, y_axis, z_axis = (one, zero, zero), (zero, one, zero), (zero, zero, one)           # OCT:397-399
    tv = [(tri[:, 3 * k], tri[:, 3 * k + 1], tri[:, 3 * k + 2]) for k in range(3)]
    with np.errstate(all="ignore"):
        sep = []
        for a, axis in enumerate((x_axis, y_axis, z_axis)):                                    # OCT:401-412
            tmin, tmax = _project(tv, axis)
            sep.append((tmax < cmin[:, a]) | (tmin > cmax[:, a]))
        mn = (cmin[:, 0], cmin[:, 1], cmin[:, 2]); mx = (cmax[:, 0], cmax[:, 1], cmax[:, 2])
        cube_vertices = [mn,                                                                    # OCT:415-424
                         (mx[0], mn[1], mn[2]), (mn[0], mx[1], mn[2]), (mn[0], mn[1], mx[2]),
                         (mn[0], mx[1], mx[2]), (mx[0], mn[1], mx[2]), (mx[0], mx[1], mn[2]),
                         mx]
        e1 = _sub(tv[0], tv[1])                                                                 # OCT:425
        e2 = _sub(tv[1], tv[2])                                                                 # OCT:426
        normal = _cross(e1, e2)                                                                 # OCT:427
        offset = _dot(normal, tv[0])                                                            # OCT:428
        cube_min, cube_max = _project(cube_vertices, normal)
        sep.append((cube_max < offset) | (cube_min > offset))                                   # OCT:430
        e3 = _sub(tv[2], tv[0])                                                                 # OCT:434
        for e in (e1, e2, e3):                                                                  # OCT:437-447, this order
            for cube_axis in (x_axis, y_axis, z_axis):
                axis = _cross(e, cube_axis)
                cube_min, cube_max = _project(cube_vertices, axis)
                tmin, tmax = _project(tv, axis)
                sep.append((cube_max < tmin) | (cube_min > tmax))                               # OCT:451
    sep = np.stack(sep, axis=1)
    return sep if per_axis else ~sep.any(axis=1)


# ------------------------------------------------------------------------------------------- build
def calc_extents(tri_verts):
    """OCT:315-330: running f32::min / f32::max over every vertex, from f32::MAX / f32::MIN"""
    v = np.asarray(tri_verts, F32).reshape(-1, 3)
    lo = np.full(3, F32_MAX, F32); hi = np.full(3, F32_MIN, F32)
    if v.shape[0]:
        lo = np.fmin(lo, np.fmin.reduce(v, axis=0))
        hi = np.fmax(hi, np.fmax.reduce(v, axis=0))
    return lo, hi


def child_cubes(cmin, cmax):
    """OCT:274-313 for s cubes: (s, 8, 3) minima and maxima, children in the reference's order.  mid = 0.5 * (max + min).
    Child i takes the upper half in x when i & 1, in y when i & 2, in z when i & 4 (read off the eight Cube::new lines)."""
    cmin = np.asarray(cmin, F32).reshape(-1, 3); cmax = np.asarray(cmax, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        mid = F32(0.5) * (cmax + cmin)                                                          # OCT:275
    kmin = np.empty((cmin.shape[0], 8, 3), F32); kmax = np.empty_like(kmin)
    for i in range(8):
        for a in range(3):
            upper = (i >> a) & 1
            kmin[:, i, a] = mid[:, a] if upper else cmin[:, a]
            kmax[:, i, a] = cmax[:, a] if upper else mid[:, a]
    return kmin, kmax


class Tree:
    """cubes (n, 6) f32 [min3, max3]; children (n, 8) int64, -1 in a leaf's row; level (n,); parent (n,) (root: 0);
    leaf_first / leaf_count (n,) into leaf_tris (global triangle ids, list order), zero for inner nodes;
    decisions: (tri, node, member) arrays, one entry per (triangle, child cube) SAT decision of the build."""

    def leaf(self, i):
        return self.leaf_tris[self.leaf_first[i]:self.leaf_first[i] + self.leaf_count[i]]

    def is_leaf(self, i):
        return self.children[i, 0] < 0

    def stats(self):
        """the counters of mi355rt_octree_stats / oracle_octree_stats, counted from the arrays"""
        leafm = self.children[:, 0] < 0
        return dict(nodes=int(self.cubes.shape[0]), inner=int((~leafm).sum()), leaves=int(leafm.sum()),
                    empty=int((leafm & (self.leaf_count == 0)).sum()), depth=int(self.level[leafm].max()),
                    tri_refs=int(self.leaf_count[leafm].sum()), max_leaf=int(self.leaf_count[leafm].max()))


def build(tri_verts, tris_per_leaf, keep_decisions=True):
    """OCT:66-146.  Level by level: every leaf of a level that holds more than tris_per_leaf triangles (and whose level
    is at most 8, OCT:108) is split; all SAT decisions of the level are taken in one array.  The reference's numbering
    follows afterwards: split_node appends the 8 children together (OCT:120-135), then splits them depth-first in
    order (OCT:136-145); node index == cube index (OCT:126-129).  keep_decisions=False leaves Tree.decisions None (a big tree's record is big);
    Tree.n_decisions counts them either way."""
    tv = np.ascontiguousarray(tri_verts, F32).reshape(-1, 9)
    ntri = tv.shape[0]
    lo, hi = calc_extents(tv)
    # per level: cubes, lists (CSR), parent slot in the previous level, and which nodes split
    lv_min = [lo.reshape(1, 3)]; lv_max = [hi.reshape(1, 3)]
    lv_first = [np.zeros(1, np.int64)]; lv_count = [np.array([ntri], np.int64)]; lv_tris = [np.arange(ntri, dtype=np.int32)]   # OCT:332-342
    lv_split = []            # per level: indices (within the level) of the nodes that split; their children are 8 * rank .. 8 * rank + 7 of the next level
    dec_tri, dec_slot, dec_member = [], [], []    # slot = (level + 1, index within that level)
    n_decisions = 0
    level = 0
    while True:
        count = lv_count[level]
        split = np.nonzero(count > tris_per_leaf)[0] if level <= MAX_SPLIT_LEVEL else np.zeros(0, np.int64)   # OCT:108
        lv_split.append(split)
        if split.size == 0:
            break
        kmin, kmax = child_cubes(lv_min[level][split], lv_max[level][split])
        scount = count[split]
        # decisions in the order (node, child, list position): OCT:120-125 with OCT:380
        per_child = np.repeat(scount, 8)                                    # list length of each (node, child)
        group = np.repeat(np.arange(split.size * 8, dtype=np.int32), per_child)
        start = np.repeat(lv_first[level][split], 8)                        # list start of each (node, child)
        gfirst = np.cumsum(per_child) - per_child
        src = (start - gfirst)[group]
        src += np.arange(group.size, dtype=np.int64)                        # list start + position in the list
        tri = lv_tris[level][src]
        del src
        gmin = kmin.reshape(-1, 3); gmax = kmax.reshape(-1, 3)
        member = np.empty(group.size, bool)
        for c0 in range(0, group.size, _CHUNK):
            s = slice(c0, c0 + _CHUNK)
            member[s] = triangle_cube_intersection(gmin[group[s]], gmax[group[s]], tv[tri[s]])
        n_decisions += group.size
        if keep_decisions:
            dec_tri.append(tri); dec_slot.append((level + 1, group)); dec_member.append(member)
        ncount = np.bincount(group[member], minlength=split.size * 8).astype(np.int64)
        lv_min.append(gmin); lv_max.append(gmax)
        lv_count.append(ncount); lv_first.append(np.cumsum(ncount) - ncount); lv_tris.append(tri[member])
        level += 1

    # numbering: the reference's depth-first order
    nlevels = len(lv_count)
    rank = []                 # per level: node -> rank among the splitting nodes, -1 for a leaf
    for l in range(nlevels):
        r = np.full(lv_count[l].size, -1, np.int64)
        r[lv_split[l]] = np.arange(lv_split[l].size)
        rank.append(r)
    # grown[l][k]: how many nodes the reference appends while split_node runs on node k of level l (0 for a node that stays a leaf)
    grown = [np.zeros(lv_count[l].size, np.int64) for l in range(nlevels)]
    for l in range(nlevels - 2, -1, -1):
        grown[l][lv_split[l]] = 8 + grown[l + 1].reshape(-1, 8).sum(axis=1)
    # length[l][k]: the length of the node vector when split_node is called on that node; its 8 children take the next 8 indices (OCT:126-135),
    # then child 0 is split with everything below it, then child 1, ... (OCT:136-145)
    index = [np.zeros(1, np.int64)]
    length = [np.ones(1, np.int64)]
    for l in range(nlevels - 1):
        at = length[l][lv_split[l]][:, None]
        below = grown[l + 1].reshape(-1, 8)
        index.append((at + np.arange(8)).reshape(-1))
        length.append((at + 8 + np.cumsum(below, axis=1) - below).reshape(-1))
    total = 1 + int(grown[0][0])
    t = Tree()
    t.cubes = np.zeros((total, 6), F32); t.children = np.full((total, 8), -1, np.int64)
    t.level = np.zeros(total, np.int64); t.parent = np.zeros(total, np.int64)
    counts = np.zeros(total, np.int64)
    for l in range(nlevels):
        idx = index[l]
        t.cubes[idx, :3] = lv_min[l]; t.cubes[idx, 3:] = lv_max[l]
        t.level[idx] = l
        leafm = rank[l] < 0
        counts[idx[leafm]] = lv_count[l][leafm]
        if lv_split[l].size:
            kids = index[l + 1].reshape(-1, 8)
            t.children[idx[lv_split[l]]] = kids
            t.parent[kids.reshape(-1)] = np.repeat(idx[lv_split[l]], 8)
    t.leaf_count = counts
    t.leaf_first = np.cumsum(counts) - counts
    t.leaf_tris = np.zeros(int(counts.sum()), np.int64)
    for l in range(nlevels):
        ks = np.nonzero((rank[l] < 0) & (lv_count[l] > 0))[0]
        if ks.size == 0:
            continue
        n = lv_count[l][ks]
        pos = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)         # position within each leaf's list
        t.leaf_tris[np.repeat(t.leaf_first[index[l][ks]], n) + pos] = lv_tris[l][np.repeat(lv_first[l][ks], n) + pos]
    t.n_decisions = n_decisions
    if not keep_decisions:
        t.decisions = None
    elif dec_tri:
        t.decisions = (np.concatenate(dec_tri).astype(np.int64), np.concatenate([index[l][g] for l, g in dec_slot]), np.concatenate(dec_member))
    else:
        t.decisions = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool))
    t.tris_per_leaf = tris_per_leaf
    return t


# ------------------------------------------------------------------------------------------- walk
def intersect_cube_inverse_ray(pos, inv_dir, cmin, cmax):
    """OCT:348-372, broadcasting; pos, inv_dir, cmin, cmax: (..., 3) f32.  Returns (hit, tmin).  f32::min / f32::max: np.fmin / np.fmax."""
    with np.errstate(all="ignore"):
        tx1 = (cmin[..., 0] - pos[..., 0]) * inv_dir[..., 0]
        tx2 = (cmax[..., 0] - pos[..., 0]) * inv_dir[..., 0]
        tmin = np.fmin(tx1, tx2)
        tmax = np.fmax(tx1, tx2)
        ty1 = (cmin[..., 1] - pos[..., 1]) * inv_dir[..., 1]
        ty2 = (cmax[..., 1] - pos[..., 1]) * inv_dir[..., 1]
        tmin = np.fmax(tmin, np.fmin(ty1, ty2))
        tmax = np.fmin(tmax, np.fmax(ty1, ty2))
        tz1 = (cmin[..., 2] - pos[..., 2]) * inv_dir[..., 2]
        tz2 = (cmax[..., 2] - pos[..., 2]) * inv_dir[..., 2]
        tmin = np.fmax(tmin, np.fmin(tz1, tz2))
        tmax = np.fmin(tmax, np.fmax(tz1, tz2))
        hit = (tmax >= tmin) & (tmax > F32(0.0))                                                # OCT:367
    return hit, tmin


def triangle_test(pos, dir_, tri):
    """INT:15-17 dispatches to moller_trumbore::intersect_late_out, INT:62-98.  pos, dir_: (r, 3); tri: (k, 9).
    Returns (some (r, k) bool, t, u, v (r, k) f32).  The rejections are written as the reference has them, so a NaN
    (which fails every comparison) is kept exactly where the reference keeps it."""
    p = tuple(pos[:, a][:, None] for a in range(3))
    d = tuple(dir_[:, a][:, None] for a in range(3))
    v0 = tuple(tri[:, a][None, :] for a in range(3))
    v1 = tuple(tri[:, 3 + a][None, :] for a in range(3))
    v2 = tuple(tri[:, 6 + a][None, :] for a in range(3))
    with np.errstate(all="ignore"):
        v0v1 = _sub(v1, v0)                                                                     # INT:65
        v0v2 = _sub(v2, v0)                                                                     # INT:66
        pvec = _cross(d, v0v2)                                                                  # INT:67
        det = _dot(v0v1, pvec)                                                                  # INT:68
        parallel = np.abs(det) < F32_EPSILON                                                    # INT:70
        inv_det = F32(1.0) / det                                                                # INT:75
        tvec = _sub(p, v0)                                                                      # INT:77
        u = _dot(tvec, pvec) * inv_det                                                          # INT:78
        qvec = _cross(tvec, v0v1)                                                               # INT:80
        v = _dot(d, qvec) * inv_det                                                             # INT:81
        t = _dot(v0v2, qvec) * inv_det                                                          # INT:84
        out = parallel | (u < F32(0.0)) | (u > F32(1.0))                                        # INT:87
        out = out | (v < F32(0.0)) | (u + v > F32(1.0))                                         # INT:90
        out = out | (t < F32(0.0))                                                              # INT:93
    shape = np.broadcast_shapes(pos[:, :1].shape, tri[:, :1].T.shape)
    return (np.broadcast_to(~out, shape), np.broadcast_to(t, shape), np.broadcast_to(u, shape), np.broadcast_to(v, shape))


class _Walk:
    def __init__(self, tree, tri_verts, rays6, reverse_ties=False):
        self.tree = tree
        self.reverse_ties = reverse_ties
        self.tv = np.ascontiguousarray(tri_verts, F32).reshape(-1, 9)
        rays = np.ascontiguousarray(rays6, F32).reshape(-1, 6)
        self.pos = rays[:, :3].copy(); self.dir = rays[:, 3:].copy()
        with np.errstate(all="ignore"):
            self.inv = F32(1.0) / self.dir                                                      # OCT:241-244
        n = rays.shape[0]
        self.tuv = np.zeros((n, 3), F32); self.prim = np.full(n, MISS, np.uint32)

    def leaf(self, node, rays):
        """OCT:156-171 with intersect_leaf_triangles, OCT:249-272, for the rays `rays` (indices).  Returns bool per ray: Some(hit)."""
        tris = self.tree.leaf(node)
        r = rays.size
        has = np.zeros(r, bool)
        if tris.size == 0:
            return has
        bt = np.zeros(r, F32); bu = np.zeros(r, F32); bv = np.zeros(r, F32); bp = np.zeros(r, np.int64)
        some, t, u, v = triangle_test(self.pos[rays], self.dir[rays], self.tv[tris])
        with np.errstate(invalid="ignore"):
            plain = not (some & ~np.isfinite(t)).any()
        if plain:
            # every Some(t) is finite: the loop below keeps the FIRST of the smallest t, which is what argmin returns
            key = np.where(some, t, F32(np.inf))
            k = np.argmin(key, axis=1)
            row = np.arange(r)
            has = some[row, k]
            bt = np.where(has, t[row, k], bt); bu = np.where(has, u[row, k], bu); bv = np.where(has, v[row, k], bv); bp = np.where(has, tris[k], bp)
        else:
            for k in range(tris.size):                   # list order; (None, Some): take it; (Some, Some): only if t is strictly smaller, OCT:258-268
                with np.errstate(invalid="ignore"):
                    take = some[:, k] & (~has | (t[:, k] < bt))
                bt = np.where(take, t[:, k], bt); bu = np.where(take, u[:, k], bu); bv = np.where(take, v[:, k], bv)
                bp = np.where(take, tris[k], bp)
                has |= take
        cube = self.tree.cubes[node]
        with np.errstate(all="ignore"):
            hp = self.pos[rays] + self.dir[rays] * bt[:, None]                                  # OCT:164: ray.pos + ray.dir * t
            outside = ((hp[:, 0] < cube[0]) | (hp[:, 0] > cube[3]) | (hp[:, 1] < cube[1]) | (hp[:, 1] > cube[4])      # OCT:34-44
                       | (hp[:, 2] < cube[2]) | (hp[:, 2] > cube[5]))
        ok = has & ~outside                                                                     # OCT:165-169
        got = rays[ok]
        self.tuv[got, 0] = bt[ok]; self.tuv[got, 1] = bu[ok]; self.tuv[got, 2] = bv[ok]
        self.prim[got] = bp[ok].astype(np.uint32)
        return ok

    def node(self, node, rays):
        """OCT:148-196 for a set of rays; returns bool per ray: Some(hit).  Rays are independent, so taking them through a
        node together changes nothing for any one of them."""
        if rays.size == 0:
            return np.zeros(0, bool)
        if self.tree.is_leaf(node):
            return self.leaf(node, rays)
        kids = self.tree.children[node]
        cubes = self.tree.cubes[kids]
        passes, tmin = intersect_cube_inverse_ray(self.pos[rays][:, None, :], self.inv[rays][:, None, :],
                                                  cubes[None, :, :3], cubes[None, :, 3:])     # (r, 8), child order: OCT:177
        if np.isnan(tmin[passes]).any():
            raise FloatingPointError("a NaN slab distance enters the sort: the reference panics here (OCT:183, partial_cmp().unwrap())")
        # OCT:183: sort_by is a STABLE sort on t; the children that failed the slab test are not in the list (sent to the end here)
        key = np.where(passes, tmin, F32(np.inf))
        if self.reverse_ties:          # NOT the reference: equal t in descending child order, for tests that ask whether their rays tell the two apart
            order = 7 - np.argsort(key[:, ::-1], axis=1, kind="stable")
        else:
            order = np.argsort(key, axis=1, kind="stable")
        # a passing child whose t is +inf must still precede the children that failed: stable order keeps lower child index first, and a failed child
        # with a lower index would overtake it; so sort the failed ones out explicitly
        failed = ~np.take_along_axis(passes, order, axis=1)
        order = np.take_along_axis(order, np.argsort(failed, axis=1, kind="stable"), axis=1)
        npass = passes.sum(axis=1)
        done = np.zeros(rays.size, bool)
        leaf_count = self.tree.leaf_count[kids]; kids_leaf = self.tree.children[kids, 0] < 0
        for k in range(8):                                                                      # OCT:188-192: the first child that returns a hit wins
            active = np.nonzero(~done & (npass > k))[0]
            if active.size == 0:
                break
            choice = order[active, k]
            for c in np.unique(choice):
                if leaf_count[c] == 0 and kids_leaf[c]:
                    continue                                                                    # an empty leaf returns None: OCT:157-158
                sel = active[choice == c]
                done[sel] = self.node(int(kids[c]), rays[sel])
        return done


def intersect(tree, tri_verts, rays6, reverse_ties=False):
    """Intersector::intersect_ray, OCT:240-246: (tuv (n, 3) f32, prim (n,) uint32).  A miss leaves tuv zero and prim 0xFFFFFFFF.
    Raises FloatingPointError where the reference would panic (a NaN slab distance in the sort).
    reverse_ties=True is a deliberately WRONG walk (children of equal t in descending order, an unstable sort's other choice)."""
    w = _Walk(tree, tri_verts, rays6, reverse_ties)
    w.node(0, np.arange(w.pos.shape[0]))
    return w.tuv, w.prim


def occluded(tree, tri_verts, rays6):
    """the shadow predicate of shade(), MOD:226-227: the intersector's hit has 0.01 < t < 1.0.  uint8 (n,)."""
    tuv, prim = intersect(tree, tri_verts, rays6)
    return occluded_from_hits(tuv, prim)


def occluded_from_hits(tuv, prim):
    with np.errstate(invalid="ignore"):
        return ((prim != MISS) & (tuv[:, 0] > F32(0.01)) & (tuv[:, 0] < F32(1.0))).astype(np.uint8)


# ------------------------------------------------------------------------------------------- exact geometry
def _frac(x):
    return Fraction(float(x))            # an f32 is a dyadic rational: exact


def exact_overlap(cmin, cmax, tri):
    """Closed triangle / closed box overlap in exact rational arithmetic (fractions.Fraction of the f32 inputs; cmin / cmax may
    also be Fractions already).  The triangle is clipped against the six closed half-spaces of the box (Sutherland-Hodgman); it
    overlaps iff the clipped polygon is non-empty.  Touching counts.  A triangle is convex, also a degenerate one (a segment or
    a point), and clipping a convex polygon by a closed half-space keeps exactly its intersection with it, so no point is lost.
    Written from the geometry: no separating axes."""
    lo = [x if isinstance(x, Fraction) else _frac(x) for x in cmin]
    hi = [x if isinstance(x, Fraction) else _frac(x) for x in cmax]
    t = [_frac(x) for x in np.asarray(tri).reshape(9)]
    poly = [(t[0], t[1], t[2]), (t[3], t[4], t[5]), (t[6], t[7], t[8])]
    for a in range(3):
        for bound, sign in ((lo[a], 1), (hi[a], -1)):          # keep sign * (p[a] - bound) >= 0
            if not poly:
                return False
            out = []
            m = len(poly)
            for i in range(m):
                p, q = poly[i], poly[(i + 1) % m]
                dp, dq = sign * (p[a] - bound), sign * (q[a] - bound)
                if dp >= 0:
                    out.append(p)
                if (dp > 0 and dq < 0) or (dp < 0 and dq > 0):
                    s = dp / (dp - dq)
                    out.append(tuple(p[c] + s * (q[c] - p[c]) for c in range(3)))
            poly = out
    return bool(poly)
