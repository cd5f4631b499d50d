"""Hand-made depth films, directions and lookup cases that no gather produces (include/mi355rt.h "PROBE VISIBILITY"), shared by
tests/test_probes_vis_abi.py (the host side of csrc/oct_vis.hpp against the numpy statement) and tests/test_gpu_probes_vis.py (the kernels against the same
statement).  The grids, SH values and queries are those of tests/probe_cases.py.  Not a test module."""
import itertools

import numpy as np

import probe_cases as pc

F = np.float32
RES = (2, 3, 8, 16)


def film(R, nprobes, seed, empty=0.25, D=3.0):
    """dict(res, max_distance, count (nprobes, R * R), moments (nprobes, R * R, 2)): random counts with a share of empty texels, whose moments hold an
    infinity — a skipped texel is never read into a sum, and one that were would show"""
    rng = np.random.default_rng(seed)
    count = rng.integers(1, 60, (nprobes, R * R)).astype(np.uint32)
    count[rng.random((nprobes, R * R)) < empty] = 0
    mean = rng.uniform(0.05, D, (nprobes, R * R))
    var = rng.uniform(0.0, 0.6, (nprobes, R * R)) ** 2
    m = np.empty((nprobes, R * R, 2), F)
    m[..., 0] = (count * mean).astype(F)
    m[..., 1] = (count * (mean * mean + var)).astype(F)
    m[count == 0] = np.inf
    return dict(res=R, max_distance=F(D), count=count, moments=m)


def flat_film(R, nprobes, mean=2.0 ** -6, count=4):
    """every texel holds `count` samples of exactly `mean` (powers of two): every bilinear mean is `mean` exactly and the variance exactly 0, so the weight is
    0 for every r > mean and 1 for every r <= mean"""
    c = np.full((nprobes, R * R), count, np.uint32)
    m = np.empty((nprobes, R * R, 2), F)
    m[..., 0] = F(count * mean); m[..., 1] = F(count * mean * mean)
    return dict(res=R, max_distance=F(3.0), count=c, moments=m)


def unit_directions():
    """float32 (k, 3): the six axes, the eight diagonals, components of +0 and -0, z just below and above 0, directions on the fold lines |x| + |y| = s (z = 0)
    and on the map's corners and edges (x = 0 or y = 0 with z < 0)"""
    d = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    d += [list(s) for s in itertools.product((1.0, -1.0), repeat=3)]
    d += [[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0], [-0.0, -0.0, -1.0], [1.0, -0.0, -0.0], [-0.0, 1.0, 0.0], [0.3, -0.0, -0.4], [-0.0, -0.7, -0.1]]
    tiny = float(np.nextafter(F(0), F(1)))
    for z in (tiny, -tiny, 1e-30, -1e-30, 1e-7, -1e-7, 0.0, -0.0):
        d += [[0.6, 0.8, z], [-0.25, 0.75, z], [0.5, -0.5, z], [-1.0, -3.0, z], [1.0, 0.0, z], [0.0, -1.0, z]]
    d += [[0.0, 0.5, -0.5], [0.5, 0.0, -0.5], [0.0, -0.2, -0.9], [-0.9, 0.0, -0.2], [1e-7, 1e-7, -1.0], [-1e-7, 1e-7, -1.0], [1e-7, -1e-7, -1.0], [-1e-7, -1e-7, -1.0]]
    return np.array(d, F)


def directions(seed=11, n=3000):
    """unit_directions at several lengths (denormal to 1e30), and n fixed-seed directions of mixed lengths; none is the zero vector, none holds a NaN"""
    u = unit_directions()
    rng = np.random.default_rng(seed)
    r = rng.normal(size=(n, 3))
    r *= (10.0 ** rng.uniform(-3, 3, n))[:, None]
    out = [u, u * F(1e-41), u * F(1e-20), u * F(0.37), u * F(7.5), u * F(1e19), u * F(1e30), r.astype(F)]
    d = np.ascontiguousarray(np.concatenate(out).astype(F))
    return d[(d != 0).any(axis=1)]


def odd_vectors():
    """vectors whose length is not a positive finite number, or nearly: the zero vectors, NaN and infinite components, an overflowing and an underflowing square"""
    return np.array([[0, 0, 0], [-0.0, 0.0, -0.0], [np.nan, 1, 0], [0, 0, np.nan], [np.inf, 0, 1], [1, -np.inf, 0], [3e19, 0, 0], [1e30, -1e30, 1e30],
                     [1e-30, 0, 0], [1e-23, 1e-23, -1e-23], [1.8e19, 0.0, 1.0], [1e-20, 0, 0], [0.5, -0.5, 0.0]], F)


def normals(m, seed=21):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(m, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    return np.ascontiguousarray(n.astype(F))


FLAGS = [(False, False), (True, False), (False, True), (True, True)]          # (chebyshev, facing)


def lookup_cases():
    """(name, grid, res, depth, usable or None, points, dirs, normals) on every case of probe_cases.cases() — negative SH values, masked probes, probes with
    n == 0, queries inside, on probes, outside and with a NaN coordinate — with a random depth film (R cycling through 2, 3, 8, 16), and for the grids with more
    than one probe a flat film whose visibility is 0 beyond 2^-6: with it only queries within that of a probe (those on probes) keep a corner, and under a mask
    that hides those probes nothing is left (ok 0)"""
    out = []
    for k, (name, g, res, usable, pts, dirs) in enumerate(pc.cases()):
        nprobes = len(res["n"])
        R = RES[k % 4]
        out.append((name + " R%d" % R, g, res, film(R, nprobes, 30 + k), usable, pts, dirs, normals(len(pts), 40 + k)))
        if name.startswith("masked") and nprobes > 1:
            out.append((name + " flat", g, res, flat_film(RES[(k + 1) % 4], nprobes), usable, pts, dirs, normals(len(pts), 60 + k)))
    return out
