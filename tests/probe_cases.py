"""Hand-made probe grids and queries that no gather produces (include/mi355rt.h "PROBES"), shared by tests/test_probes_abi.py (the host side
of csrc/sh9.hpp against the numpy statement) and tests/test_gpu_probes.py (the lookup kernel against the same statement).  Not a test module."""
import numpy as np

F = np.float32
COUNTS = [(1, 1, 1), (2, 1, 3), (4, 3, 2), (5, 5, 5)]
# dyadic origins and spacings make "exactly on a probe" exact in f32; (4, 3, 2) has neither
GRIDS = {(1, 1, 1): ([0.5, -1.0, 2.0], [1.0, 1.0, 1.0]), (2, 1, 3): ([-1.5, 0.25, 0.0], [2.0, 0.5, 0.75]),
         (4, 3, 2): ([0.3, -0.7, 1.1], [0.7, 1.3, 0.9]), (5, 5, 5): ([-2.0, -2.0, -2.0], [1.0, 0.5, 0.25])}


def grid(counts):
    o, s = GRIDS[tuple(counts)]
    return dict(origin=np.array(o, F), spacing=np.array(s, F), counts=np.array(counts, np.uint32))


def values(counts, seed=1, empty=True):
    """dict(n, sh) with negative values, denormals and (empty) some probes with n == 0"""
    rng = np.random.default_rng(seed)
    nprobes = int(np.prod(counts))
    n = rng.integers(1, 400, nprobes).astype(np.uint32)
    sh = (rng.normal(size=(nprobes, 9, 3)) * 40.0).astype(F)
    sh.reshape(-1)[::11] = F(1e-40)                       # denormals, which the weights make smaller still
    sh.reshape(-1)[5::17] = F(-3e-42)
    if empty and nprobes > 1:
        n[rng.random(nprobes) < 0.1] = 0
        n[1::4] = 0
        n[0] = 7
    return dict(n=n, sh=sh)


def probe_positions(g):
    """origin + float32(i) * spacing in index order, written out here (probes.grid_points is held to it by the host test)"""
    nx, ny, nz = (int(c) for c in g["counts"])
    out = np.empty((nz, ny, nx, 3), F)
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                out[iz, iy, ix] = [g["origin"][0] + F(ix) * g["spacing"][0], g["origin"][1] + F(iy) * g["spacing"][1], g["origin"][2] + F(iz) * g["spacing"][2]]
    return out.reshape(-1, 3)


def queries(g, m=257, seed=3):
    """(points, dirs) float32 (m, 3): every prefix mixes interior points, points exactly on probes, on faces, on edges between probes, outside, far outside
    (1e30, infinity) and points with a NaN coordinate; the first query is interior.  dirs are unit vectors, a few of them not (used as given)."""
    rng = np.random.default_rng(seed)
    cnt = np.array([int(c) for c in g["counts"]])
    lo = g["origin"].astype(np.float64)
    hi = lo + (cnt - 1) * g["spacing"].astype(np.float64)
    size = np.maximum(hi - lo, g["spacing"].astype(np.float64))
    pts = lo + rng.random((m, 3)) * (hi - lo)
    gp = probe_positions(g).astype(np.float64)
    kind = np.arange(m) % 8
    for q in range(m):
        a = int(rng.integers(0, 3))
        if kind[q] == 1:
            pts[q] = gp[rng.integers(0, len(gp))]
        elif kind[q] == 2:
            pts[q, a] = (lo, hi)[int(rng.integers(0, 2))][a]
        elif kind[q] == 3:
            pts[q] = pts[q] + size * rng.choice([-1.5, 1.5], 3)
        elif kind[q] == 4:
            pts[q, a] = rng.choice([1e30, -1e30, np.inf, -np.inf])
        elif kind[q] == 5:
            pts[q, a] = np.nan
        elif kind[q] == 6:
            on = gp[rng.integers(0, len(gp))]
            keep = pts[q, a]
            pts[q] = on; pts[q, a] = keep
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[3::29] *= 1.7
    return np.ascontiguousarray(pts.astype(F)), np.ascontiguousarray(d.astype(F))


def cases():
    """(name, grid, res, usable or None, points, dirs) for every hand-made grid: all values with and without a usable mask, a mask that leaves nothing
    (ok 0, rgb exactly 0), and an infinite coefficient in a probe that queries reach with zero weight only"""
    out = []
    for counts in COUNTS:
        g = grid(counts)
        nprobes = int(np.prod(counts))
        pts, dirs = queries(g)
        res = values(counts)
        out.append(("plain %s" % (counts,), g, res, None, pts, dirs))
        mask = (np.random.default_rng(9).random(nprobes) < 0.6).astype(np.uint8)
        out.append(("masked %s" % (counts,), g, values(counts, seed=2, empty=False), mask, pts, dirs))
        out.append(("nothing usable %s" % (counts,), g, res, np.zeros(nprobes, np.uint8), pts, dirs))
        if tuple(counts) != (4, 3, 2) and nprobes > 1:
            # the queries sit exactly on the probes, so each uses its own probe alone and every neighbour has weight 0 — the last probe holds an infinity
            # and is not itself queried
            inf = values(counts, seed=4, empty=False)
            inf["sh"][nprobes - 1, 4, 1] = np.inf
            on = probe_positions(g)[:nprobes - 1]
            d = np.tile(np.array([[0.48, -0.6, 0.64]], F), (len(on), 1))
            out.append(("infinity at zero weight %s" % (counts,), g, inf, None, np.ascontiguousarray(on), np.ascontiguousarray(d)))
    return out
