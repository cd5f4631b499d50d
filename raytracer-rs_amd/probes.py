"""The statement of RayTracer.probes_gather / probes_lookup (include/mi355rt.h, "PROBES") in numpy.

Host code, float32 with every rounding explicit, no GPU.  A probe is a film of its own: per point n and 9 x 3 sums (and hits, near), accumulated in sample
order over gather's sphere-mode samples; the lookup is a read-out of such a film laid out as a grid:

    basis(d)                                              the nine real spherical harmonics up to band 2 of a direction, used as given
    project(rgb, t, hit, d, npoints, near_distance, prev) the per-point sums from the traced rays' results            (what probes_project_kernel does)
    lookup(grid, res, points, dirs, mode, usable)         trilinear interpolation of the grid, evaluated for dirs     (what probes_lookup_kernel does)
    grid_points(grid), grid_over(lo, hi, counts)          the probes' positions in index order; a grid over a box
    usable(res, max_near_share)                           a mask of the probes that are not buried in geometry

A grid is a dict(origin=(3,), spacing=(3,), counts=(3,)): probe (ix, iy, iz) has index (iz * ny + iy) * nx + ix and sits at origin + float32(i) * spacing.  A
result is a dict with n uint32 (npoints,) and sh float32 (npoints, 9, 3) (and hits, near), as project() returns it.  Layout of the samples: sample-major, row
s * npoints + i is sample s of point i, as gather.rays(normals=None) makes them.  Every expression below is f32, unfused, in the order written: csrc/sh9.hpp
and the kernels of csrc/probes.hip evaluate the same expressions.  The basis is polynomial in the direction, so nothing here needs a transcendental function.
"""
import numpy as np

_F = np.float32
C0, C1, C2, C3, C4 = _F(0.282094792), _F(0.488602512), _F(1.092548431), _F(0.315391565), _F(0.546274215)
A_BAND = (_F(3.14159265), _F(2.09439510), _F(0.785398163))      # the cosine lobe per band: pi, 2 pi / 3, pi / 4
A = tuple(A_BAND[0 if k == 0 else 1 if k < 4 else 2] for k in range(9))
SPHERE = _F(12.566370614)                                       # 4 pi
MODES = {"radiance": 0, "irradiance": 1}                        # MI355RT_SH_*


def basis(d):
    """b_0 .. b_8 of directions d float32 (..., 3) -> float32 (..., 9)"""
    d = np.asarray(d, _F)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = np.empty(d.shape[:-1] + (9,), _F)
    with np.errstate(all="ignore"):
        out[..., 0] = C0
        out[..., 1] = C1 * y
        out[..., 2] = C1 * z
        out[..., 3] = C1 * x
        out[..., 4] = C2 * (x * y)
        out[..., 5] = C2 * (y * z)
        out[..., 6] = C3 * (_F(3.0) * (z * z) - _F(1.0))
        out[..., 7] = C2 * (x * z)
        out[..., 8] = C4 * (x * x - y * y)
    return out


def project(rgb, t, hit, d, npoints, near_distance=np.inf, prev=None):
    """Per point, in sample order: sh[k][c] += b_k(d) * rgb_c; n += 1; hits += hit; near += hit and t < near_distance.  rgb, d: float32 (spp * npoints, 3);
    t: float32 (spp * npoints,) (read where hit); hit: bool (spp * npoints,).  prev: a dict of earlier results to add to (the accumulate of
    mi355rt_probes_gather), None: from 0; it is not written.  Returns dict(n, hits, near uint32 (npoints,); sh float32 (npoints, 9, 3))."""
    npts = int(npoints)
    rgb = np.ascontiguousarray(rgb, _F).reshape(-1, npts, 3)
    spp = rgb.shape[0]
    d = np.ascontiguousarray(d, _F).reshape(spp, npts, 3)
    t = np.ascontiguousarray(t, _F).reshape(spp, npts)
    hit = np.asarray(hit).reshape(spp, npts).astype(bool)
    nd = _F(near_distance)
    res = {}
    for k, shape, dt in (("n", (npts,), np.uint32), ("hits", (npts,), np.uint32), ("near", (npts,), np.uint32), ("sh", (npts, 9, 3), _F)):
        res[k] = np.zeros(shape, dt) if prev is None or prev.get(k) is None else np.array(prev[k], dt).reshape(shape)
    with np.errstate(all="ignore"):
        for s in range(spp):
            b = basis(d[s])
            res["sh"] = res["sh"] + b[:, :, None] * rgb[s][:, None, :]
            res["n"] += np.uint32(1)
            res["hits"][hit[s]] += np.uint32(1)
            res["near"][hit[s] & (t[s] < nd)] += np.uint32(1)
    return res


def _grid(grid):
    origin = np.ascontiguousarray(grid["origin"], _F).reshape(3)
    spacing = np.ascontiguousarray(grid["spacing"], _F).reshape(3)
    counts = [int(c) for c in np.asarray(grid["counts"]).reshape(3)]
    if min(counts) < 1 or counts[0] * counts[1] * counts[2] >= 2**31:
        raise ValueError("grid counts: each >= 1, the product < 2^31")
    if not (np.isfinite(spacing).all() and (spacing > 0).all() and np.isfinite(origin).all()):
        raise ValueError("grid: spacing finite and positive, origin finite")
    return origin, spacing, counts


def _axis(p, origin, spacing, count):
    """one axis of the queries: (i uint32, f float32)"""
    with np.errstate(all="ignore"):
        g = (p - origin) / spacing
        g = np.where(g >= _F(0.0), g, _F(0.0)).astype(_F)        # a NaN becomes 0: no index is ever made from a NaN
        top = _F(count - 1)
        g = np.where(g <= top, g, top).astype(_F)
        i = g.astype(np.uint32)
        if count >= 2:
            i = np.where(i > np.uint32(count - 2), np.uint32(count - 2), i).astype(np.uint32)
        f = g - i.astype(_F)
    if count == 1:
        i = np.zeros_like(i); f = np.zeros_like(f)
    return i, f


def lookup(grid, res, points, dirs, mode="irradiance", usable=None):
    """The grid interpolated at points float32 (m, 3) and evaluated for dirs float32 (m, 3): mode "radiance" (arriving from dir) or "irradiance" (at normal
    dir).  res: dict with n uint32 (nprobes,) and sh float32 (nprobes, 9, 3); usable: uint8 (nprobes,) or None.  A corner is skipped when its weight is 0, its
    n is 0 or it is not usable, and a skipped corner is never read into a sum.  Returns (rgb float32 (m, 3), ok uint8 (m,)); no corner used: rgb 0, ok 0.
    Nothing is clamped."""
    if mode not in MODES:
        raise ValueError("mode: one of %s, not %r" % (tuple(MODES), mode))
    origin, spacing, counts = _grid(grid)
    nprobes = counts[0] * counts[1] * counts[2]
    n = np.ascontiguousarray(res["n"], np.uint32).reshape(nprobes)
    sh = np.ascontiguousarray(res["sh"], _F).reshape(nprobes, 27)
    use = None if usable is None else np.ascontiguousarray(usable, np.uint8).reshape(nprobes)
    points = np.ascontiguousarray(points, _F).reshape(-1, 3)
    dirs = np.ascontiguousarray(dirs, _F).reshape(points.shape[0], 3)
    m = points.shape[0]
    i, f = zip(*(_axis(points[:, a], origin[a], spacing[a], counts[a]) for a in range(3)))
    Cq = np.zeros((m, 27), _F); wsum = np.zeros(m, _F); ok = np.zeros(m, bool)
    with np.errstate(all="ignore"):
        for j in range(8):
            c, w = [], []
            for a in range(3):
                up = (j >> a) & 1
                c.append(np.minimum(i[a].astype(np.int64) + 1, counts[a] - 1) if up else i[a].astype(np.int64))
                w.append(f[a] if up else _F(1.0) - f[a])
            t = (w[0] * w[1]) * w[2]
            probe = (c[2] * counts[1] + c[1]) * counts[0] + c[0]
            nj = n[probe]
            used = (t != _F(0.0)) & (nj != 0)
            if use is not None:
                used &= use[probe] != 0
            s = t * (SPHERE / nj.astype(_F))
            wsum = np.where(used, wsum + t, wsum)
            Cq = np.where(used[:, None], Cq + s[:, None] * sh[probe], Cq)
            ok |= used
        b = basis(dirs)
        r = np.zeros((m, 3), _F)
        for k in range(9):
            ck = Cq[:, 3 * k:3 * k + 3]
            r = r + ((A[k] * ck) if mode == "irradiance" else ck) * b[:, k, None]
        rgb = np.where(ok[:, None], r / wsum[:, None], _F(0.0)).astype(_F)
    return rgb, ok.astype(np.uint8)


def grid_points(grid):
    """the probes' positions in index order: float32 (nx * ny * nz, 3), origin_a + float32(i_a) * spacing_a"""
    origin, spacing, counts = _grid(grid)
    ax = [origin[a] + np.arange(counts[a], dtype=np.uint32).astype(_F) * spacing[a] for a in range(3)]
    out = np.empty((counts[2], counts[1], counts[0], 3), _F)
    out[..., 0] = ax[0][None, None, :]
    out[..., 1] = ax[1][None, :, None]
    out[..., 2] = ax[2][:, None, None]
    return out.reshape(-1, 3)


def grid_over(lo, hi, counts):
    """A grid whose outermost probes sit on the box lo .. hi: spacing (hi - lo) / (count - 1) in f32.  An axis with one probe puts it at the middle of the
    box (spacing 1: the lookup never uses it); an axis on which the box is flat gets spacing 1 too."""
    lo, hi = np.asarray(lo, _F).reshape(3), np.asarray(hi, _F).reshape(3)
    counts = [int(c) for c in counts]
    origin, spacing = lo.copy(), np.ones(3, _F)
    for a in range(3):
        if counts[a] == 1:
            origin[a] = lo[a] + (hi[a] - lo[a]) * _F(0.5)
        elif hi[a] > lo[a]:
            spacing[a] = (hi[a] - lo[a]) / _F(counts[a] - 1)
    return dict(origin=origin, spacing=spacing, counts=np.array(counts, np.uint32))


def usable(res, max_near_share=0.25):
    """uint8 (nprobes,): 1 for a probe with samples of which at most max_near_share hit geometry nearer than the gather's near_distance; a probe buried in
    geometry (or one without samples) is 0 and the lookup leaves it out"""
    n = np.asarray(res["n"]).astype(np.float64)
    near = np.asarray(res["near"]).astype(np.float64)
    return ((n > 0) & (near <= float(max_near_share) * n)).astype(np.uint8)
