"""bvh_statement.py — an independent statement of the BVH the device builds (csrc/lbvh.hip), in numpy.

TEST INFRASTRUCTURE ONLY, like the rest of oracle/: nothing under raytracer-rs_amd/ (the product) and not
bench.py may import this file.  numpy only: no ctypes, and nothing here looks at the product.

Why it exists: the device build (Morton keys, a stable sort, Karras' hierarchy, an atomic bottom-up refit, outward
rounded half-precision boxes) is fully deterministic — a leaf holds one triangle, so every inner node survives and
keeps Karras' number — and so the tree can be stated exactly, word for word, not only checked for validity.  It is
written from the header comments of lbvh.hip, from bvh.hpp and from T. Karras, "Maximizing Parallelism in the
Construction of BVHs, Octrees, and k-d Trees" (HPG 2012), in another shape than the kernels:
  - the hierarchy is built TOP DOWN: a range of sorted positions is split at the highest bit in which its first and
    its last (key, position) pair differ.  Karras' bottom-up searches (direction, range end, split) do not appear;
  - the key is assembled bit by bit in Python-sized steps, not with magic masks;
  - the directed half rounding is "round to nearest, then one step outward when on the wrong side", on whole arrays;
  - every f32 operation is one numpy operation on np.float32 arrays, so each rounds once and nothing is fused.

check_tree() is independent of all of the above: a plain walk from the root of ANY builder's tree that decodes the
halves with np.float16 and compares boxes with the vertices in float64.

THE CONVENTIONS STATED HERE
  scene bounds   min / max over all vertices
  pad            max(diag * 2e-5f, 1e-6f), diag = sqrt((dx*dx + dy*dy) + dz*dz) in f32, d = max - min
  key            box centre c = 0.5f * (mn + mx); q = (c - smin) * sinv, sinv = 1.0f / extent (0 where the extent is 0);
                 q * 2^21, negative or NaN -> 0, clamped to 2097151, truncated; bit b of qx, qy, qz goes to bit
                 3b + 2, 3b + 1, 3b of the 63-bit key
  order          stable sort by key: ties in ascending triangle index
  hierarchy      the binary radix tree over (key, sorted position); root 0; a range split after position gamma has its
                 inner children numbered gamma (left) and gamma + 1 (right)
  boxes          exact min / max unions of the triangles' boxes
  height         0 for a leaf, 1 + max over the children for an inner node: a node over two leaves has height 1.  The
                 root's height is the reported max_depth: the greatest number of inner nodes on a root-to-leaf path
  node           8 words { h0[3], child0, h1[3], child1 }: h[a] = half_down(mn[a] - pad) | half_up(mx[a] + pad) << 16,
                 an inner child is its number, a leaf is ~(position << 3)
  triangle       12 words { v0[3], prim, e1[3], geom, e2[3], 0 } at its sorted position, e1 = v1 - v0, e2 = v2 - v0
"""
import bisect

import numpy as np

F32 = np.float32
KEY_MAX = 2097151            # 2^21 - 1
MAX_DEPTH = 31               # bvh.hpp: kBvhMaxDepth


# ------------------------------------------------------------------------------------------- scalars of the scene
def scene_bounds(tri_verts):
    v = np.asarray(tri_verts, F32).reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)


def padding(smin, smax):
    d = np.asarray(smax, F32) - np.asarray(smin, F32)
    sq = d * d
    diag = np.sqrt((sq[0] + sq[1]) + sq[2])
    return max(diag * F32(2e-5), F32(1e-6))


# ------------------------------------------------------------------------------------------- keys
def quantised_centres(tri_verts, smin, smax):
    """(n, 3) integers in [0, 2097151]: where the box centre of each triangle lies in the scene box, per axis"""
    v = np.asarray(tri_verts, F32).reshape(-1, 3, 3)
    smin = np.asarray(smin, F32); smax = np.asarray(smax, F32)
    mn = v.min(axis=1); mx = v.max(axis=1)
    centre = F32(0.5) * (mn + mx)
    with np.errstate(all="ignore"):
        extent = smax - smin
        sinv = np.where(smax > smin, F32(1.0) / extent, F32(0.0)).astype(F32)
        q = (centre - smin) * sinv
        q = q * F32(2097152.0)
        q = np.where(q > F32(0.0), q, F32(0.0)).astype(F32)                 # negative, NaN -> 0
        q = np.where(q < F32(KEY_MAX), q, F32(KEY_MAX)).astype(F32)         # the scene's max corner -> the last cell
    return q.astype(np.int64)                                               # truncation (q >= 0)


def morton_keys(tri_verts, smin, smax):
    """(n,) uint64: x at bit 2, y at bit 1, z at bit 0 of each triple of the 63-bit key"""
    q = quantised_centres(tri_verts, smin, smax).astype(np.uint64)
    key = np.zeros(q.shape[0], np.uint64)
    for b in range(21):
        for axis, place in ((0, 2), (1, 1), (2, 0)):
            key |= ((q[:, axis] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + place)
    return key


# ------------------------------------------------------------------------------------------- hierarchy
def radix_tree(sorted_keys):
    """The binary radix tree over the (key, position) pairs of a sorted key list, top down.  Returns per inner node
    (n - 1 of them, Karras' numbers) lo, hi (its range of positions), and left, right: a child >= 0 is an inner node,
    a child < 0 is the leaf ~child (a position).  Needs n >= 2."""
    keys = [int(k) for k in sorted_keys]
    n = len(keys)
    assert n >= 2 and all(keys[i] <= keys[i + 1] for i in range(n - 1))
    lo = np.full(n - 1, -1, np.int64); hi = np.full(n - 1, -1, np.int64)
    left = np.zeros(n - 1, np.int64); right = np.zeros(n - 1, np.int64)
    todo = [(0, 0, n - 1)]
    while todo:
        node, a, b = todo.pop()
        assert lo[node] < 0, "node number %d given twice" % node
        if keys[a] != keys[b]:
            bit = (keys[a] ^ keys[b]).bit_length() - 1                  # the highest bit in which the range's keys differ
            first_with_bit = ((keys[a] >> bit) | 1) << bit              # keys[a] has the bit clear, keys[b] has it set
            gamma = bisect.bisect_left(keys, first_with_bit, a, b + 1) - 1
        else:                                                           # one key: the positions tell the pairs apart
            bit = (a ^ b).bit_length() - 1
            gamma = ((b >> bit) << bit) - 1
        assert a <= gamma < b
        lo[node], hi[node] = a, b
        for side, (ca, cb, number) in enumerate(((a, gamma, gamma), (gamma + 1, b, gamma + 1))):
            ref = ~ca if ca == cb else number
            (left if side == 0 else right)[node] = ref
            if ca != cb:
                todo.append((number, ca, cb))
    assert (lo >= 0).all()
    return lo, hi, left, right


def _bottom_up_order(left, right):
    """inner nodes, every node after its children"""
    order = []
    todo = [0]
    while todo:
        i = todo.pop()
        order.append(i)
        for c in (int(left[i]), int(right[i])):
            if c >= 0:
                todo.append(c)
    return order[::-1]


# ------------------------------------------------------------------------------------------- directed half rounding
def half_bits_directed(x, up):
    """f32 array -> binary16 bit patterns (uint32 array), rounded toward +inf (up) or -inf: round to nearest first, then one
    representable value outward where the result lies on the wrong side.  +-0 steps to the smallest denormal of the right
    sign; a finite value beyond the half range gives +-inf on the outward side and +-65504 on the inward side; +-inf stays;
    NaN gives the widest bound (+inf up, -inf down)."""
    x = np.atleast_1d(np.asarray(x, F32))
    with np.errstate(all="ignore"):
        h = x.astype(np.float16)
        back = h.astype(F32)
        wrong = (back < x) if up else (back > x)
    b = h.view(np.uint16).astype(np.uint32)
    is_zero = (b & 0x7FFF) == 0
    away_from_zero = ((b & 0x8000) == 0) == bool(up)
    stepped = np.where(is_zero, np.uint32(0x0001 if up else 0x8001), np.where(away_from_zero, b + np.uint32(1), b - np.uint32(1)))
    out = np.where(wrong, stepped, b)
    return np.where(np.isnan(x), np.uint32(0x7C00 if up else 0xFC00), out).astype(np.uint32)


def pack_box(mn, mx, pad):
    """(k, 3) f32 boxes -> (k, 3) words: the padded minimum rounded down in the low half, the padded maximum rounded up in the high half"""
    with np.errstate(all="ignore"):
        lo = (np.asarray(mn, F32) - F32(pad)).astype(F32)
        hi = (np.asarray(mx, F32) + F32(pad)).astype(F32)
    shape = lo.shape
    return (half_bits_directed(lo.reshape(-1), False) | half_bits_directed(hi.reshape(-1), True) << np.uint32(16)).reshape(shape)


# ------------------------------------------------------------------------------------------- the tree
def build(tri_verts, tri_geom):
    """The tree of the device builder for n >= 2 triangles, as the read-out gives it: dict(order, keys (sorted), nodes (n - 1, 8) uint32,
    tris (n, 12) uint32, root, leaves, max_depth, max_leaf, scene_min, scene_max, pad, lo, hi, left, right, height (per node))."""
    verts = np.ascontiguousarray(tri_verts, F32).reshape(-1, 9)
    geom = np.ascontiguousarray(tri_geom, np.uint32).reshape(-1)
    n = verts.shape[0]
    assert n >= 2 and geom.shape[0] == n
    smin, smax = scene_bounds(verts)
    pad = padding(smin, smax)
    keys = morton_keys(verts, smin, smax)
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    lo, hi, left, right = radix_tree(skeys)

    v = verts.reshape(n, 3, 3)[order]
    leaf_mn = v.min(axis=1); leaf_mx = v.max(axis=1)
    node_mn = np.zeros((n - 1, 3), F32); node_mx = np.zeros((n - 1, 3), F32)
    height = np.zeros(n - 1, np.int64)

    def child_box(c):
        return (leaf_mn[~c], leaf_mx[~c], 0) if c < 0 else (node_mn[c], node_mx[c], int(height[c]))

    for i in _bottom_up_order(left, right):
        a_mn, a_mx, a_h = child_box(int(left[i])); b_mn, b_mx, b_h = child_box(int(right[i]))
        node_mn[i] = np.minimum(a_mn, b_mn); node_mx[i] = np.maximum(a_mx, b_mx)
        height[i] = 1 + max(a_h, b_h)

    nodes = np.zeros((n - 1, 8), np.uint32)
    for side, refs in enumerate((left, right)):
        is_leaf = refs < 0
        pos = np.where(is_leaf, ~refs, 0); num = np.where(is_leaf, 0, refs)
        mn = np.where(is_leaf[:, None], leaf_mn[pos], node_mn[num])
        mx = np.where(is_leaf[:, None], leaf_mx[pos], node_mx[num])
        nodes[:, 4 * side:4 * side + 3] = pack_box(mn, mx, pad)
        link = np.where(is_leaf, ~(pos << 3), num)                        # a leaf of one triangle: ~(position << 3 | 1 - 1)
        nodes[:, 4 * side + 3] = link.astype(np.int32).view(np.uint32)

    tris = np.zeros((n, 12), np.uint32)
    with np.errstate(all="ignore"):
        v0 = v[:, 0]; e1 = v[:, 1] - v[:, 0]; e2 = v[:, 2] - v[:, 0]
    tris[:, 0:3] = np.ascontiguousarray(v0, F32).view(np.uint32)
    tris[:, 3] = order.astype(np.uint32)
    tris[:, 4:7] = np.ascontiguousarray(e1, F32).view(np.uint32)
    tris[:, 7] = geom[order]
    tris[:, 8:11] = np.ascontiguousarray(e2, F32).view(np.uint32)
    return dict(order=order.astype(np.uint32), keys=skeys, nodes=nodes, tris=tris, root=0, leaves=n, max_depth=int(height[0]), max_leaf=1,
                scene_min=smin, scene_max=smax, pad=pad, lo=lo, hi=hi, left=left, right=right, height=height)


def first_difference(nodes, other):
    """None, or a sentence naming the first node whose words differ, with both sides' words"""
    nodes = np.asarray(nodes, np.uint32).reshape(-1, 8); other = np.asarray(other, np.uint32).reshape(-1, 8)
    if nodes.shape != other.shape:
        return "%d nodes against the statement's %d" % (nodes.shape[0], other.shape[0])
    bad = np.nonzero((nodes != other).any(axis=1))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    fmt = lambda w: " ".join("%08x" % int(x) for x in w)
    return "%d of %d nodes differ; first: node %d has [%s], the statement [%s]" % (bad.size, nodes.shape[0], i, fmt(nodes[i]), fmt(other[i]))


# ------------------------------------------------------------------------------------------- any builder's tree, checked by a walk
def _half(words):
    return words.astype(np.uint16).view(np.float16).astype(np.float64)


def check_tree(nodes, tris, tri_verts, tri_geom, root=0, leaves=None, max_leaf=None):
    """A plain walk from `root` over nodes (k, 8) and tris (n, 12) of ANY builder.  Raises AssertionError naming what is wrong:
    a triangle in no leaf or in two, prim not a permutation, geom / v0 / e1 / e2 not right on the bits, a child box (decoded with
    np.float16) that fails to hold a vertex below it (float64 compare), an inner node reached twice, `leaves` or `max_leaf` not
    what the walk counts.  Returns dict(inner, leaves, max_leaf, path_inner): path_inner is the greatest number of inner nodes on
    any root-to-leaf path — what the traversal stack has to serve; the caller compares it with the builder's max_depth."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 12)
    verts = np.ascontiguousarray(tri_verts, F32).reshape(-1, 3, 3)
    geom = np.ascontiguousarray(tri_geom, np.uint32).reshape(-1)
    n = verts.shape[0]
    assert tris.shape[0] == n, "%d triangle slots for %d triangles" % (tris.shape[0], n)
    # the triangle words
    prim = tris[:, 3].astype(np.int64)
    assert prim.max() < n and np.array_equal(np.sort(prim), np.arange(n)), "prim is not a permutation of the triangles"
    src = verts[prim]
    assert np.array_equal(tris[:, 7], geom[prim]), "geom differs"
    assert np.array_equal(tris[:, 0:3], np.ascontiguousarray(src[:, 0]).view(np.uint32)), "v0 differs"
    with np.errstate(all="ignore"):
        e1 = src[:, 1] - src[:, 0]; e2 = src[:, 2] - src[:, 0]
    assert np.array_equal(tris[:, 4:7], np.ascontiguousarray(e1).view(np.uint32)), "e1 differs"
    assert np.array_equal(tris[:, 8:11], np.ascontiguousarray(e2).view(np.uint32)), "e2 differs"
    assert not tris[:, 11].any(), "pad word not 0"
    slot_mn = src.astype(np.float64).min(axis=1); slot_mx = src.astype(np.float64).max(axis=1)      # exact box per triangle slot

    # the walk: depth (inner nodes above) of every inner node, the leaves
    child = nodes[:, [3, 7]].view(np.int32).astype(np.int64)
    depth = np.full(nodes.shape[0], -1, np.int64)
    seen = np.zeros(n, np.int64)
    n_leaves = 0; biggest = 0; path_inner = 0
    todo = [(int(np.int32(root)), 0)]
    while todo:
        ref, above = todo.pop()
        if ref < 0:
            code = ~ref; first, count = code >> 3, (code & 7) + 1
            assert first + count <= n, "leaf %d + %d beyond the %d triangles" % (first, count, n)
            seen[first:first + count] += 1
            n_leaves += 1; biggest = max(biggest, count); path_inner = max(path_inner, above)
        else:
            assert ref < nodes.shape[0], "child %d beyond the %d nodes" % (ref, nodes.shape[0])
            assert depth[ref] < 0, "inner node %d reached twice" % ref
            depth[ref] = above
            todo.append((int(child[ref, 0]), above + 1)); todo.append((int(child[ref, 1]), above + 1))
    lost = np.nonzero(seen == 0)[0]; twice = np.nonzero(seen > 1)[0]
    assert lost.size == 0, "%d triangle slots in no leaf, first %d (triangle %d)" % (lost.size, lost[0], prim[lost[0]])
    assert twice.size == 0, "%d triangle slots in more than one leaf, first %d (triangle %d)" % (twice.size, twice[0], prim[twice[0]])

    # boxes: level by level from the deepest, the exact float64 box of everything below each child against the child's halves
    reached = np.nonzero(depth >= 0)[0]
    below_mn = np.zeros((nodes.shape[0], 3)); below_mx = np.zeros((nodes.shape[0], 3))
    for level in range(int(depth.max()) if reached.size else -1, -1, -1):
        idx = reached[depth[reached] == level]
        acc_mn = np.full((idx.size, 3), np.inf); acc_mx = np.full((idx.size, 3), -np.inf)
        for side in range(2):
            c = child[idx, side]
            leaf = c < 0
            code = np.where(leaf, ~c, 0); first = code >> 3; count = (code & 7) + 1
            mn = below_mn[np.where(leaf, 0, c)].copy(); mx = below_mx[np.where(leaf, 0, c)].copy()
            lmn = np.full((idx.size, 3), np.inf); lmx = np.full((idx.size, 3), -np.inf)
            for k in range(8):
                use = leaf & (k < count)
                at = np.where(use, first + k, 0)
                lmn = np.where(use[:, None], np.minimum(lmn, slot_mn[at]), lmn); lmx = np.where(use[:, None], np.maximum(lmx, slot_mx[at]), lmx)
            mn = np.where(leaf[:, None], lmn, mn); mx = np.where(leaf[:, None], lmx, mx)
            words = nodes[idx][:, 4 * side:4 * side + 3]
            box_lo = _half(words & np.uint32(0xFFFF)); box_hi = _half(words >> np.uint32(16))
            ok = (box_lo <= mn).all(axis=1) & (box_hi >= mx).all(axis=1)            # a NaN half fails here too
            if not ok.all():
                j = int(np.nonzero(~ok)[0][0])
                raise AssertionError("child %d of node %d: box [%r, %r] does not hold [%r, %r] below it (%d such boxes at this level)"
                                     % (side, idx[j], box_lo[j].tolist(), box_hi[j].tolist(), mn[j].tolist(), mx[j].tolist(), int((~ok).sum())))
            acc_mn = np.minimum(acc_mn, mn); acc_mx = np.maximum(acc_mx, mx)
        below_mn[idx] = acc_mn; below_mx[idx] = acc_mx
    if leaves is not None:
        assert n_leaves == leaves, "%d leaves reached, %d reported" % (n_leaves, leaves)
    if max_leaf is not None:
        assert biggest == max_leaf, "largest leaf %d, reported %d" % (biggest, max_leaf)
    return dict(inner=int(reached.size), leaves=n_leaves, max_leaf=biggest, path_inner=path_inner)
