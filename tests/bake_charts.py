"""Hand-made UV charts and atlas masks shared by tests/test_bake_abi.py (host twin against the statement) and tests/test_gpu_bake.py (kernels against the
statement).  A chart set is a float32 (ntri, 3, 2) array for a scene of ntri triangles: the first rows are the case, the rest lie off the atlas."""
from fractions import Fraction

import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
OFF = [[2.0, 2.0], [3.0, 2.0], [2.0, 3.0]]          # a chart wholly outside the atlas


def _pad(rows, ntri):
    uv = np.empty((ntri, 3, 2), F)
    uv[:] = np.asarray(OFF, F)
    uv[:len(rows)] = np.asarray(rows, F)
    return uv


def charts(ntri):
    """name -> (uv, width, height): the hand-made cases for a scene of ntri >= 2 triangles"""
    nan, inf = np.nan, np.inf
    c = {
        # a quad split along the diagonal x == y, which passes through every texel centre (i + 0.5, i + 0.5): each centre owned once, by triangle 0
        "diagonal": (_pad([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], ntri), 8, 8),
        "diagonal_swapped": (_pad([[[0, 0], [1, 1], [0, 1]], [[0, 0], [1, 0], [1, 1]]], ntri), 8, 8),
        "mirrored": (_pad([[[0, 0], [1, 1], [1, 0]], [[0, 0], [0, 1], [1, 1]]], ntri), 8, 8),
        "zero_area": (_pad([[[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]], [[0.3, 0.3], [0.3, 0.3], [0.3, 0.3]]], ntri), 8, 8),
        "outside": (_pad([OFF, [[-3, -3], [-2, -3], [-3, -2]]], ntri), 8, 8),
        "half_outside": (_pad([[[-0.5, -0.5], [1.0, -0.5], [-0.5, 1.0]], [[0.5, 0.5], [1.5, 0.5], [0.5, 1.5]]], ntri), 8, 8),
        "nan_inf": (_pad([[[nan, 0], [1, 0], [1, 1]], [[0, 0], [inf, 0], [0, 1]], ], ntri), 8, 8),
        "neg_inf": (_pad([[[0, 0], [1, -inf], [1, 1]], [[0.25, 0.25], [0.75, 0.25], [0.25, 0.75]]], ntri), 8, 8),
        "overlap": (_pad([[[0.1, 0.1], [0.9, 0.1], [0.1, 0.9]], [[0, 0], [1, 0], [0, 1]]], ntri), 16, 16),
        "overlap_swapped": (_pad([[[0, 0], [1, 0], [0, 1]], [[0.1, 0.1], [0.9, 0.1], [0.1, 0.9]]], ntri), 16, 16),
        # smaller than a texel, around the corner between four texels: contains no centre
        "sub_texel": (_pad([[[0.49, 0.49], [0.51, 0.49], [0.49, 0.51]], [[0.26, 0.26], [0.27, 0.26], [0.26, 0.27]]], ntri), 8, 8),
        "odd_atlas": (_pad([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], ntri), 65, 9),
        "tiny_atlas": (_pad([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], ntri), 1, 1),
        "narrow_atlas": (_pad([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], ntri), 3, 5),
    }
    if ntri >= 48:
        # the LAST triangle covers the whole atlas (x + y <= 2 holds on the unit square); the others are small charts on top of it, which win
        rows = []
        for i in range(ntri - 1):
            x, y = (i % 8) / 8.0 + 0.02, (i // 8) / 8.0 + 0.02
            rows.append([[x, y], [x + 0.06, y], [x, y + 0.06]])
        rows.append([[0, 0], [2, 0], [0, 2]])
        c["whole_atlas_under_small_ones"] = (np.asarray(rows, F), 64, 64)
    return c


def crowd(ntri):
    """ntri copies of one small chart inside one tile: a bin far longer than any fixed staging"""
    return _pad([[[0.30, 0.30], [0.36, 0.30], [0.30, 0.36]]] * ntri, ntri), 64, 64


def masks():
    """name -> (ids, values, width, height, dilate): hand-made atlases"""
    rng = np.random.default_rng(11)
    val = lambda n: rng.uniform(0.0, 4.0, (n, 3)).astype(F)
    island = np.array([y * 9 + x for y in range(2, 5) for x in range(3, 6) if (x, y) != (4, 3)], np.uint32)       # a ring: its hole is filled from 8 sides
    out = {
        "one_texel": (np.array([2 * 7 + 3], np.uint32), val(1), 7, 5, 2),
        "corner_texel": (np.array([0], np.uint32), val(1), 4, 4, 3),
        "island": (island, val(island.size), 9, 7, 2),
        "full": (np.arange(6 * 4, dtype=np.uint32), val(24), 6, 4, 2),
        "empty": (np.zeros(0, np.uint32), np.zeros((0, 3), F), 5, 3, 2),
        "dilate_0": (island, val(island.size), 9, 7, 0),
        "dilate_beyond_the_atlas": (np.array([5 * 12 + 1, 2 * 12 + 9], np.uint32), val(2), 12, 7, 300),
        "two_blocks": (rng.permutation(40 * 33)[:300].astype(np.uint32), val(300), 40, 33, 4),
        "negative_zero": (np.array([0, 2], np.uint32), np.array([[-0.0, -0.0, 1.0], [-0.0, 2.0, -0.0]], F), 3, 1, 1),
    }
    return out


# ---- exact coverage ------------------------------------------------------------------------------------------------------------------------------------
def jittered_mesh(seed, quads=8, size=32):
    """(uv (2 * quads^2, 3, 2), size): a quads x quads grid of quads over the whole atlas of size x size texels, inner vertices jittered, every quad split
    along a random diagonal, every triangle with a random winding; on odd seeds a third of the inner vertices are snapped onto texel centres and another
    third onto texel edges.  size is a power of two, so px = uv * size is exact."""
    rng = np.random.default_rng(seed)
    step = size / quads
    gx, gy = np.meshgrid(np.arange(quads + 1) * step, np.arange(quads + 1) * step)
    p = np.stack([gx, gy], axis=-1).astype(np.float64)
    p[1:-1, 1:-1] += rng.uniform(-0.45 * step, 0.45 * step, (quads - 1, quads - 1, 2))
    if seed & 1:
        kind = rng.integers(0, 3, (quads - 1, quads - 1))
        inner = p[1:-1, 1:-1]
        inner[kind == 1] = np.floor(inner[kind == 1]) + 0.5
        inner[kind == 2] = np.round(inner[kind == 2])
    p = (p / size).astype(F)
    tris = []
    for j in range(quads):
        for i in range(quads):
            a, b, c, d = p[j, i], p[j, i + 1], p[j + 1, i + 1], p[j + 1, i]
            pair = [[a, b, c], [a, c, d]] if rng.integers(0, 2) else [[a, b, d], [b, c, d]]
            for t in pair:
                tris.append(t[::-1] if rng.integers(0, 2) else t)
    return np.asarray(tris, F), size


def exactly_inside(uv3, size, x, y):
    """the centre of texel (x, y) lies in the closed triangle, in rational arithmetic on the f32 coordinates; a zero-area triangle holds nothing"""
    px = [Fraction(float(F(u) * F(size))) for u in uv3[:, 0]]
    py = [Fraction(float(F(v) * F(size))) for v in uv3[:, 1]]
    cx, cy = Fraction(2 * x + 1, 2), Fraction(2 * y + 1, 2)
    e = []
    for p, q in ((1, 2), (2, 0), (0, 1)):
        e.append((px[p] - cx) * (py[q] - cy) - (py[p] - cy) * (px[q] - cx))
    if sum(e) == 0:
        return False
    return all(v >= 0 for v in e) or all(v <= 0 for v in e)
