"""The statement of RayTracer.probes_gather / probes_lookup (include/mi355rt.h, "PROBES") in numpy.

Host code, float32 with every rounding explicit, no GPU.  A probe is a film of its own: per point n and 9 x 3 sums (and hits, near), accumulated in sample
order over gather's sphere-mode samples; the lookup is a read-out of such a film laid out as a grid:

    basis(d)                                              the nine real spherical harmonics up to band 2 of a direction, used as given
    project(rgb, t, hit, d, npoints, near_distance, prev) the per-point sums from the traced rays' results            (what probes_project_kernel does)
    lookup(grid, res, points, dirs, mode, usable)         trilinear interpolation of the grid, evaluated for dirs     (what probes_lookup_kernel does)
    grid_points(grid), grid_over(lo, hi, counts)          the probes' positions in index order; a grid over a box
    usable(res, max_near_share)                           a mask of the probes that are not buried in geometry

and of RayTracer.probes_gather_depth / probes_lookup_vis (include/mi355rt.h, "PROBE VISIBILITY"): per probe a depth film over an octahedral
map of R x R texels, and a lookup that trusts a probe less where the query lies farther than the probe usually sees that way (csrc/oct_vis.hpp and the
kernels of csrc/probes_vis.hip evaluate the same expressions; only + - x / sqrt, comparisons and integer conversions):

    oct_encode(v), oct_texel(v, R)                        a direction, used as given, on the unit square; the texel (ix, iy) of a sample
    project_depth(t, hit, d, npoints, R, max_distance, prev)   count and the sums of dist, dist^2 per (point, texel)   (what probes_depth_*_kernel do)
    visibility(count, moments, R, v)                      the Chebyshev weight of one probe for v = query - probe position
    lookup_vis(grid, res, depth, points, dirs, normals, mode, usable, chebyshev, facing, normal_bias)     lookup with corner weight (t * vis) * face
    grid_max_distance(grid)                               1.5 x the length of the spacing vector, the usual max_distance

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


# ---- probe visibility (include/mi355rt.h, "PROBE VISIBILITY") ----------------------------------------------------------------------------
VIS_CHEBYSHEV, VIS_FACING = 1, 2                                # MI355RT_VIS_*
RES_MIN, RES_MAX = 2, 16
MAX_DISTANCE_TOP = 1e12                                         # D^2 times 2^32 samples stays finite in f32


def _res(R):
    if int(R) != R or not RES_MIN <= int(R) <= RES_MAX:
        raise ValueError("res: an integer %d .. %d, not %r" % (RES_MIN, RES_MAX, R))
    return int(R)


def _max_distance(D):
    D = float(D)
    if not (np.isfinite(D) and 0.0 < D <= MAX_DISTANCE_TOP):
        raise ValueError("max_distance: finite, > 0 and <= 1e12, not %r" % D)
    return _F(D)


def oct_encode(v):
    """A direction v float32 (..., 3), used as given (not normalised), on the unit square: (u, w) float32 (...).  s = (|x| + |y|) + |z|; px = x / s,
    py = y / s; with z < 0 the lower half folds outwards: (px, py) = ((1 - |py|) * sx, (1 - |px|) * sy) from the old values, sx = x >= 0 ? 1 : -1;
    u = px * 0.5 + 0.5, w = py * 0.5 + 0.5."""
    v = np.asarray(v, _F)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(all="ignore"):
        s = (np.abs(x) + np.abs(y)) + np.abs(z)
        px, py = x / s, y / s
        sx = np.where(x >= _F(0.0), _F(1.0), _F(-1.0)).astype(_F)
        sy = np.where(y >= _F(0.0), _F(1.0), _F(-1.0)).astype(_F)
        fx = (_F(1.0) - np.abs(py)) * sx
        fy = (_F(1.0) - np.abs(px)) * sy
        px = np.where(z < _F(0.0), fx, px).astype(_F)
        py = np.where(z < _F(0.0), fy, py).astype(_F)
        u = px * _F(0.5) + _F(0.5)
        w = py * _F(0.5) + _F(0.5)
    return u, w


def _texel_axis(u, R):
    with np.errstate(all="ignore"):
        g = u * _F(R)
        g = np.where(g >= _F(0.0), g, _F(0.0)).astype(_F)       # a NaN becomes 0: no index is ever made from a NaN
        return np.minimum(g.astype(np.uint32), np.uint32(R - 1)).astype(np.uint32)


def oct_texel(v, R):
    """The bin of a sample with direction v: (ix, iy) uint32 (...); per axis g = u * (float)R, 0 where !(g >= 0), i = min((uint32)g, R - 1).  The texel's
    index is iy * R + ix."""
    R = _res(R)
    u, w = oct_encode(v)
    return _texel_axis(u, R), _texel_axis(w, R)


def project_depth(t, hit, d, npoints, R, max_distance, prev=None):
    """The depth film of the samples project() takes (same sample-major layout).  Per point, in sample order: dist = hit ? (t < D ? t : D) : D (a NaN t
    becomes D); k = oct_texel(d); count[k] += 1; m[k][0] += dist; m[k][1] += dist * dist.  Every sample goes into exactly one texel.  prev: a dict with count
    and moments to add to (None: from 0); it is not written.  Returns dict(count uint32 (npoints, R * R), moments float32 (npoints, R * R, 2))."""
    R, D = _res(R), _max_distance(max_distance)
    npts = int(npoints)
    d = np.ascontiguousarray(d, _F).reshape(-1, npts, 3)
    spp = d.shape[0]
    t = np.ascontiguousarray(t, _F).reshape(spp, npts)
    hit = np.asarray(hit).reshape(spp, npts).astype(bool)
    count = np.zeros((npts, R * R), np.uint32) if prev is None else np.array(prev["count"], np.uint32).reshape(npts, R * R)
    m = np.zeros((npts, R * R, 2), _F) if prev is None else np.array(prev["moments"], _F).reshape(npts, R * R, 2)
    at = np.arange(npts)
    with np.errstate(all="ignore"):
        for s in range(spp):
            ix, iy = oct_texel(d[s], R)
            k = (iy * np.uint32(R) + ix).astype(np.int64)
            dist = np.where(hit[s], np.where(t[s] < D, t[s], D), D).astype(_F)
            count[at, k] += np.uint32(1)
            m[at, k, 0] = m[at, k, 0] + dist
            m[at, k, 1] = m[at, k, 1] + dist * dist
    return dict(count=count, moments=m)


def oct_wrap(i, j, R):
    """An index pair outside [0, R - 1]^2 on the texel the octahedral map puts there: the x rule, then the y rule applied to its result.  i, j: int64 arrays."""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    lo, hi = i < 0, i >= R
    j = np.where(lo | hi, R - 1 - j, j)
    i = np.where(lo, 0, np.where(hi, R - 1, i))
    lo, hi = j < 0, j >= R
    i = np.where(lo | hi, R - 1 - i, i)
    j = np.where(lo, 0, np.where(hi, R - 1, j))
    return i, j


def _length(v):
    """(r, fine): r = sqrt((x * x + y * y) + z * z); fine where r is a positive finite number"""
    with np.errstate(all="ignore"):
        x, y, z = v[..., 0], v[..., 1], v[..., 2]
        r = np.sqrt((x * x + y * y) + z * z).astype(_F)
        return r, (r > _F(0.0)) & np.isfinite(r)


def _visibility(count, moments, R, v, r, fine):
    """visibility() for m vectors at once: count uint32 (m, R * R) and moments float32 (m, R * R, 2) are the films of the probes the vectors belong to"""
    m = v.shape[0]
    at = np.arange(m)
    with np.errstate(all="ignore"):
        u, w = oct_encode(np.where(fine[:, None], v, _F(1.0)).astype(_F))        # where not fine the answer is 1 and nothing here is used
        i1, f = [], []
        for c in (u, w):
            g = c * _F(R) + _F(0.5)
            i = g.astype(np.uint32)
            i1.append(i.astype(np.int64)); f.append(g - i.astype(_F))
        ws = np.zeros(m, _F); a = np.zeros(m, _F); b = np.zeros(m, _F)
        for dj in (0, 1):
            for di in (0, 1):
                wt = (f[0] if di else _F(1.0) - f[0]) * (f[1] if dj else _F(1.0) - f[1])
                i, j = oct_wrap(i1[0] - 1 + di, i1[1] - 1 + dj, R)
                k = j * R + i
                cnt = count[at, k]
                used = (wt != _F(0.0)) & (cnt != 0)
                cf = np.where(used, cnt, 1).astype(_F)
                ws = np.where(used, ws + wt, ws)
                a = np.where(used, a + wt * (moments[at, k, 0] / cf), a)
                b = np.where(used, b + wt * (moments[at, k, 1] / cf), b)
        some = fine & (ws != _F(0.0))
        wss = np.where(some, ws, _F(1.0)).astype(_F)
        mean, mean2 = a / wss, b / wss
        var = np.abs(mean2 - mean * mean)
        dd = r - mean
        c = var / (var + dd * dd)
        return np.where(some & ~(r <= mean), (c * c) * c, _F(1.0)).astype(_F)


def visibility(count, moments, R, v):
    """The Chebyshev weight of ONE probe with film count uint32 (R * R,), moments float32 (R * R, 2) for v = p_b - probe position -> float32.
    r = sqrt((x * x + y * y) + z * z); not a positive finite number: 1.  The texel means are fetched bilinearly at oct_encode(v), per axis without a floor:
    g = u * (float)R + 0.5, i1 = (uint32)g, f = g - (float)i1, texels i1 - 1 and i1 with weights 1 - f and f, out-of-range pairs wrapped by oct_wrap; the
    four in the order (dj, di) = (0,0), (0,1), (1,0), (1,1) with wt = wx * wy; one with wt == 0 or count == 0 is skipped, else ws += wt,
    a += wt * (m0 / (float)count), b += wt * (m1 / (float)count).  ws == 0: 1.  mean = a / ws, mean2 = b / ws; r <= mean: 1; else var = |mean2 - mean * mean|,
    dd = r - mean, c = var / (var + dd * dd), and the weight is (c * c) * c."""
    R = _res(R)
    v = np.ascontiguousarray(v, _F).reshape(1, 3)
    r, fine = _length(v)
    out = _visibility(np.ascontiguousarray(count, np.uint32).reshape(1, R * R), np.ascontiguousarray(moments, _F).reshape(1, R * R, 2), R, v, r, fine)
    return _F(out[0])


def lookup_vis(grid, res, depth, points, dirs, normals=None, mode="irradiance", usable=None, chebyshev=True, facing=True, normal_bias=0.0):
    """lookup() with the weight of corner j wj = (t * vis) * face in the place of t: in the == 0 skip, in wsum += and in s = wj * (4 pi / n).  depth:
    dict(res, count uint32 (nprobes, R * R), moments float32 (nprobes, R * R, 2)) as project_depth fills it at the grid's probes.  p_b = p + normal_bias *
    normal (p without normals); v = p_b - probe position; vis = visibility(v) when chebyshev, else 1; face = q * q + 0.2 when facing, normals are given and
    |v| is positive and finite, else 1, with q = (dot(-v, normal) / r + 1) * 0.5 made 0.0001 where !(q >= 0.0001) and the dot (x * nx + y * ny) + z * nz of
    the negated components.  The cell and the fractions come from p.  As in lookup a corner with t == 0, n == 0 or usable == 0 is skipped before anything of
    it is read; one whose wj is 0 is skipped like them.  Returns (rgb float32 (m, 3), ok uint8 (m,)).  Nothing is clamped."""
    if mode not in MODES:
        raise ValueError("mode: one of %s, not %r" % (tuple(MODES), mode))
    origin, spacing, counts = _grid(grid)
    nprobes = counts[0] * counts[1] * counts[2]
    R = _res(depth["res"])
    count = np.ascontiguousarray(depth["count"], np.uint32).reshape(nprobes, R * R)
    moments = np.ascontiguousarray(depth["moments"], _F).reshape(nprobes, R * R, 2)
    n = np.ascontiguousarray(res["n"], np.uint32).reshape(nprobes)
    sh = np.ascontiguousarray(res["sh"], _F).reshape(nprobes, 27)
    use = None if usable is None else np.ascontiguousarray(usable, np.uint8).reshape(nprobes)
    points = np.ascontiguousarray(points, _F).reshape(-1, 3)
    dirs = np.ascontiguousarray(dirs, _F).reshape(points.shape[0], 3)
    m = points.shape[0]
    bias = _F(normal_bias)
    if not np.isfinite(bias):
        raise ValueError("normal_bias must be finite")
    nrm = None if normals is None else np.ascontiguousarray(normals, _F).reshape(m, 3)
    with np.errstate(all="ignore"):
        pb = points if nrm is None else (points + bias * nrm).astype(_F)
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
            v = np.stack([pb[:, a] - (origin[a] + c[a].astype(np.uint32).astype(_F) * spacing[a]) for a in range(3)], axis=1).astype(_F)
            r, fine = _length(v)
            vis = _visibility(count[probe], moments[probe], R, v, r, fine) if chebyshev else np.ones(m, _F)
            face = np.ones(m, _F)
            if facing and nrm is not None:
                dot = ((-v[:, 0]) * nrm[:, 0] + (-v[:, 1]) * nrm[:, 1]) + (-v[:, 2]) * nrm[:, 2]
                q = (dot / np.where(fine, r, _F(1.0)).astype(_F) + _F(1.0)) * _F(0.5)
                q = np.where(q >= _F(0.0001), q, _F(0.0001)).astype(_F)
                face = np.where(fine, q * q + _F(0.2), _F(1.0)).astype(_F)
            wj = (t * vis) * face
            nj = n[probe]
            used = (t != _F(0.0)) & (nj != 0) & (wj != _F(0.0))
            if use is not None:
                used &= use[probe] != 0
            s = wj * (SPHERE / nj.astype(_F))
            wsum = np.where(used, wsum + wj, wsum)
            Cq = np.where(used[:, None], Cq + s[:, None] * sh[probe], Cq)
            ok |= used
        b = basis(dirs)
        rr = np.zeros((m, 3), _F)
        for k in range(9):
            ck = Cq[:, 3 * k:3 * k + 3]
            rr = rr + ((A[k] * ck) if mode == "irradiance" else ck) * b[:, k, None]
        rgb = np.where(ok[:, None], rr / wsum[:, None], _F(0.0)).astype(_F)
    return rgb, ok.astype(np.uint8)


def grid_max_distance(grid):
    """1.5 x the length of the grid's spacing vector: the usual max_distance of a depth film, a little more than the farthest a query can lie from a corner"""
    _, spacing, _ = _grid(grid)
    return float(_F(1.5 * float(np.sqrt((spacing.astype(np.float64) ** 2).sum()))))


# ---- probe placement (include/mi355rt.h, "PROBE PLACEMENT") -------------------------------------------------------------------------------
# and of RayTracer.probes_survey / probes_place / probes_lookup_placed: what a probe sees around itself, where it moves, the state it gets and the lookup that
# knows the moves (csrc/probe_place.hpp and the kernels of csrc/probes_place.hip evaluate the same expressions):
#
#     survey(t, prim, d, tri_normals, npoints, max_distance, flip, prev)   counts and three records per point from the samples' closest hits
#     place(survey, offsets, grid, back_share, max_offset, min_front)      the new offsets and a verdict per probe
#     classify(survey, back_share), usable_states(state)                   UNKNOWN / BURIED / IDLE / ACTIVE, and the lookups' usable mask
#     lookup_placed(..., offsets), corner_weights(...)                     lookup_vis with the probes at grid point + offset; the eight weights of a query
#     relocate(rt, grid, rounds, spp, ...), grid_min_front(grid)           rounds of survey and place from zero offsets, then survey and classify
MISS = 0xFFFFFFFF
SURVEY_FLIP = 1                                                 # MI355RT_SURVEY_FLIP
UNKNOWN, BURIED, IDLE, ACTIVE = 0, 1, 2, 3                      # MI355RT_PROBE_*
PLACE_UNSAMPLED, PLACE_THROUGH, PLACE_AWAY, PLACE_STAY, PLACE_BACK, PLACE_REST, PLACE_REFUSED = 0, 1, 2, 3, 4, 5, 8      # MI355RT_PLACE_*
BACK_SHARE, MAX_OFFSET = 0.25, 0.45                             # the published DDGI values
SURVEY_KEYS = ("n", "back", "front", "near_back", "near_front", "far")
_INF = _F(np.inf)


def survey_empty(npoints, max_distance):
    """the survey of npoints points without a sample: counts 0, near records (+inf, 0, 0, 0), far records (-inf, 0, 0, 0)"""
    npts = int(npoints)
    res = dict(n=np.zeros(npts, np.uint32), back=np.zeros(npts, np.uint32), front=np.zeros(npts, np.uint32), near_back=np.zeros((npts, 4), _F),
               near_front=np.zeros((npts, 4), _F), far=np.zeros((npts, 4), _F), max_distance=float(_max_distance(max_distance)))
    res["near_back"][:, 0] = np.inf; res["near_front"][:, 0] = np.inf; res["far"][:, 0] = -np.inf
    return res


def survey(t, prim, d, tri_normals, npoints, max_distance, flip=False, prev=None):
    """What each point sees, from the closest hits of the samples project() takes (same sample-major layout).  t float32 and prim uint32 (spp * npoints,) as
    intersect_rays answers (t is read where prim != MISS; a prim is MISS or a triangle index), d float32 (spp * npoints, 3) the rays' directions, used as given,
    tri_normals float32 (ntri, 3) (features.tri_normals(scene)), negated with flip.  A sample is a hit when prim != MISS and t is a positive finite number; a hit
    is a back hit when (dx * Nx + dy * Ny) + dz * Nz > 0, else (a NaN dot too) a front hit.  Per point, in sample order, with D = max_distance: n += 1; back hit:
    back += 1, and (t, d) replaces near_back where t < near_back.dist; front hit: front += 1, (t, d) replaces near_front where t < near_front.dist, and
    dist = t < D ? t : D; miss: dist = D; for a front hit or a miss (dist, d) replaces far where dist > far.dist.  Strict comparisons: the first sample of a
    distance keeps the record.  prev: a survey to continue (None: empty); it is not written.  Returns dict(n, back, front uint32 (npoints,); near_back,
    near_front, far float32 (npoints, 4) rows (dist, dx, dy, dz); max_distance)."""
    D = _max_distance(max_distance)
    npts = int(npoints)
    d = np.ascontiguousarray(d, _F).reshape(-1, npts, 3)
    spp = d.shape[0]
    t = np.ascontiguousarray(t, _F).reshape(spp, npts)
    prim = np.ascontiguousarray(prim, np.uint32).reshape(spp, npts)
    N = np.ascontiguousarray(tri_normals, _F).reshape(-1, 3)
    if N.shape[0] == 0:
        N = np.zeros((1, 3), _F)                                 # a scene without triangles: every sample is a miss and no normal is used
    res = survey_empty(npts, D)
    if prev is not None:
        if float(_F(prev["max_distance"])) != float(D):
            raise ValueError("prev: its max_distance is %r, not %r" % (prev["max_distance"], float(D)))
        for k in SURVEY_KEYS:
            res[k] = np.array(prev[k], res[k].dtype).reshape(res[k].shape)
    with np.errstate(all="ignore"):
        for s in range(spp):
            found = prim[s] != np.uint32(MISS)
            hit = found & (t[s] > _F(0.0)) & (t[s] <= _F(3.402823466e+38))
            nrm = N[np.where(found, prim[s], 0).astype(np.int64)]
            if flip:
                nrm = -nrm
            dot = (d[s][:, 0] * nrm[:, 0] + d[s][:, 1] * nrm[:, 1]) + d[s][:, 2] * nrm[:, 2]
            back = hit & (dot > _F(0.0))
            front = hit & ~back
            rec = np.concatenate([t[s][:, None], d[s]], axis=1).astype(_F)
            res["n"] += np.uint32(1)
            res["back"][back] += np.uint32(1)
            res["front"][front] += np.uint32(1)
            take = back & (t[s] < res["near_back"][:, 0])
            res["near_back"][take] = rec[take]
            take = front & (t[s] < res["near_front"][:, 0])
            res["near_front"][take] = rec[take]
            dist = np.where(front, np.where(t[s] < D, t[s], D), D).astype(_F)
            take = ~back & (dist > res["far"][:, 0])
            rec[:, 0] = dist
            res["far"][take] = rec[take]
    return res


def _survey_arrays(sv, nprobes):
    return tuple(np.ascontiguousarray(sv[k], np.uint32 if k in ("n", "back", "front") else _F).reshape((nprobes,) if k in ("n", "back", "front") else (nprobes, 4))
                 for k in SURVEY_KEYS)


def _place_config(back_share, max_offset, min_front=None):
    bs, mo = _F(back_share), _F(max_offset)
    if not (_F(0.0) <= bs <= _F(1.0)):
        raise ValueError("back_share: in [0, 1], not %r" % back_share)
    if not (np.isfinite(mo) and mo >= 0):
        raise ValueError("max_offset: finite and >= 0, not %r" % max_offset)
    if min_front is None:
        return bs, mo, None
    mf = _F(min_front)
    if not (np.isfinite(mf) and mf > 0):
        raise ValueError("min_front: finite and > 0, not %r" % min_front)
    return bs, mo, mf


def place(sv, offsets, grid, back_share=BACK_SHARE, max_offset=MAX_OFFSET, min_front=None, want_verdict=False):
    """Where every probe of the grid goes.  sv: the survey at grid_points(grid) + offsets; offsets float32 (nprobes, 3) or None (zero); min_front: a length
    (grid_min_front(grid) is the usual choice).  With share = (float)back / (float)n, o the probe's offset, nb / nf / far its records:
        n == 0: no candidate (PLACE_UNSAMPLED)
        share > back_share and nb.dist < +inf: len = nb.dist + 0.5 * min_front; c = o + nb.d * len                             (PLACE_THROUGH)
        else nf.dist < +inf and nf.dist < min_front: dot = (nf.x * far.x + nf.y * far.y) + nf.z * far.z, ln and lf the lengths sqrt((x * x + y * y) + z * z)
            of the two directions; dot <= (0.5 * ln) * lf: m = far.dist < min_front ? far.dist : min_front; c = o + (far.d * m) / lf        (PLACE_AWAY)
            otherwise no candidate                                                                                              (PLACE_STAY)
        else o != 0: lo = |o|, room = nf.dist - min_front; nf.dist < +inf and room < lo: c = o + ((-o) * room) / lo; else c = 0     (PLACE_BACK)
        else no candidate (PLACE_REST)
    The candidate becomes the offset only if every component has |c| < max_offset * spacing or c == 0, an axis with one probe having spacing 0; a component that
    is not finite fails both.  A refused candidate leaves the offset and adds PLACE_REFUSED to the verdict.  Returns offsets float32 (nprobes, 3), with
    want_verdict (offsets, verdict uint8 (nprobes,))."""
    origin, spacing, counts = _grid(grid)
    nprobes = counts[0] * counts[1] * counts[2]
    if min_front is None:
        raise ValueError("min_front: give one (probes.grid_min_front(grid) is the usual choice)")
    bs, mo, mf = _place_config(back_share, max_offset, min_front)
    n, back, front, nb, nf, far = _survey_arrays(sv, nprobes)
    o = np.zeros((nprobes, 3), _F) if offsets is None else np.ascontiguousarray(offsets, _F).reshape(nprobes, 3)
    if not np.isfinite(o).all():
        raise ValueError("offsets: holds a value that is not finite")
    with np.errstate(all="ignore"):
        share = back.astype(_F) / n.astype(_F)
        sampled = n != 0
        through = sampled & (share > bs) & (nb[:, 0] < _INF)
        near = sampled & ~through & (nf[:, 0] < _INF) & (nf[:, 0] < mf)
        dot = (nf[:, 1] * far[:, 1] + nf[:, 2] * far[:, 2]) + nf[:, 3] * far[:, 3]
        ln = np.sqrt((nf[:, 1] * nf[:, 1] + nf[:, 2] * nf[:, 2]) + nf[:, 3] * nf[:, 3]).astype(_F)
        lf = np.sqrt((far[:, 1] * far[:, 1] + far[:, 2] * far[:, 2]) + far[:, 3] * far[:, 3]).astype(_F)
        away = near & (dot <= (_F(0.5) * ln) * lf)
        stay = near & ~away
        moved = (o != _F(0.0)).any(axis=1)
        backw = sampled & ~through & ~near & moved
        rest = sampled & ~through & ~near & ~moved
        length = nb[:, 0] + _F(0.5) * mf
        c_through = o + nb[:, 1:4] * length[:, None]
        m = np.where(far[:, 0] < mf, far[:, 0], mf).astype(_F)
        c_away = o + (far[:, 1:4] * m[:, None]) / lf[:, None]
        lo = np.sqrt((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2]).astype(_F)
        room = nf[:, 0] - mf
        part = (nf[:, 0] < _INF) & (room < lo)
        c_back = np.where(part[:, None], o + ((-o) * room[:, None]) / lo[:, None], _F(0.0)).astype(_F)
        c = np.where(through[:, None], c_through, np.where(away[:, None], c_away, c_back)).astype(_F)
        bound = np.array([mo * (_F(0.0) if counts[a] == 1 else spacing[a]) for a in range(3)], _F)
        fits = ((np.abs(c) < bound[None, :]) | (c == _F(0.0))).all(axis=1)
    cand = through | away | backw
    out = np.where((cand & fits)[:, None], c, o).astype(_F)
    verdict = np.full(nprobes, PLACE_UNSAMPLED, np.uint8)
    for mask, code in ((through, PLACE_THROUGH), (away, PLACE_AWAY), (stay, PLACE_STAY), (backw, PLACE_BACK), (rest, PLACE_REST)):
        verdict[mask] = code
    verdict[cand & ~fits] |= PLACE_REFUSED
    return (out, verdict) if want_verdict else out


def classify(sv, back_share=BACK_SHARE):
    """uint8 (nprobes,): UNKNOWN where n == 0; BURIED where (float)back / (float)n > back_share; IDLE where not near_front.dist < the survey's max_distance (no
    front hit within reach: nothing there to light); ACTIVE everything else"""
    nprobes = int(np.asarray(sv["n"]).size)
    n, back, front, nb, nf, far = _survey_arrays(sv, nprobes)
    bs, _, _ = _place_config(back_share, MAX_OFFSET)
    D = _max_distance(sv["max_distance"])
    with np.errstate(all="ignore"):
        share = back.astype(_F) / n.astype(_F)
        state = np.where(n == 0, UNKNOWN, np.where(share > bs, BURIED, np.where(nf[:, 0] < D, ACTIVE, IDLE)))
    return state.astype(np.uint8)


def usable_states(state):
    """uint8: 1 for ACTIVE and IDLE probes, the shape of the usable= mask the lookups take (a numpy array or a torch tensor)"""
    if isinstance(state, np.ndarray):
        return ((state == ACTIVE) | (state == IDLE)).astype(np.uint8)
    return ((state == ACTIVE) | (state == IDLE)).to(state.dtype)


def grid_min_front(grid):
    """a fifth of the smallest spacing among the axes with more than one probe (of all axes when every axis has one): the usual min_front"""
    _, spacing, counts = _grid(grid)
    s = [spacing[a] for a in range(3) if counts[a] > 1] or list(spacing)
    return float(_F(0.2) * min(s))


def _placed(grid, res, depth, points, normals, usable, chebyshev, facing, normal_bias, offsets):
    """the corners of lookup_placed: (m, per corner (used, wj, probe))"""
    origin, spacing, counts = _grid(grid)
    nprobes = counts[0] * counts[1] * counts[2]
    R = _res(depth["res"])
    count = np.ascontiguousarray(depth["count"], np.uint32).reshape(nprobes, R * R)
    moments = np.ascontiguousarray(depth["moments"], _F).reshape(nprobes, R * R, 2)
    n = np.ascontiguousarray(res["n"], np.uint32).reshape(nprobes)
    use = None if usable is None else np.ascontiguousarray(usable, np.uint8).reshape(nprobes)
    off = None if offsets is None else np.ascontiguousarray(offsets, _F).reshape(nprobes, 3)
    if off is not None and not np.isfinite(off).all():
        raise ValueError("offsets: holds a value that is not finite")
    points = np.ascontiguousarray(points, _F).reshape(-1, 3)
    m = points.shape[0]
    bias = _F(normal_bias)
    if not np.isfinite(bias):
        raise ValueError("normal_bias must be finite")
    nrm = None if normals is None else np.ascontiguousarray(normals, _F).reshape(m, 3)
    with np.errstate(all="ignore"):
        pb = points if nrm is None else (points + bias * nrm).astype(_F)
    i, f = zip(*(_axis(points[:, a], origin[a], spacing[a], counts[a]) for a in range(3)))
    corners = []
    with np.errstate(all="ignore"):
        for j in range(8):
            c, w = [], []
            for a in range(3):
                up = (j >> a) & 1
                c.append(np.minimum(i[a].astype(np.int64) + 1, counts[a] - 1) if up else i[a].astype(np.int64))
                w.append(f[a] if up else _F(1.0) - f[a])
            t = (w[0] * w[1]) * w[2]
            probe = (c[2] * counts[1] + c[1]) * counts[0] + c[0]
            pos = [origin[a] + c[a].astype(np.uint32).astype(_F) * spacing[a] for a in range(3)]
            if off is not None:
                pos = [pos[a] + off[probe, a] for a in range(3)]
            v = np.stack([pb[:, a] - pos[a] for a in range(3)], axis=1).astype(_F)
            r, fine = _length(v)
            vis = _visibility(count[probe], moments[probe], R, v, r, fine) if chebyshev else np.ones(m, _F)
            face = np.ones(m, _F)
            if facing and nrm is not None:
                dot = ((-v[:, 0]) * nrm[:, 0] + (-v[:, 1]) * nrm[:, 1]) + (-v[:, 2]) * nrm[:, 2]
                q = (dot / np.where(fine, r, _F(1.0)).astype(_F) + _F(1.0)) * _F(0.5)
                q = np.where(q >= _F(0.0001), q, _F(0.0001)).astype(_F)
                face = np.where(fine, q * q + _F(0.2), _F(1.0)).astype(_F)
            wj = (t * vis) * face
            nj = n[probe]
            used = (t != _F(0.0)) & (nj != 0) & (wj != _F(0.0))
            if use is not None:
                used &= use[probe] != 0
            corners.append((used, wj.astype(_F), probe))
    return m, corners


def corner_weights(grid, res, depth, points, normals=None, usable=None, chebyshev=True, facing=True, normal_bias=0.0, offsets=None):
    """The weights lookup_placed gives the eight corners of each query: float32 (m, 8), corner j in column j, 0 for a corner that is skipped; and the corners'
    probe indices int64 (m, 8)"""
    m, corners = _placed(grid, res, depth, points, normals, usable, chebyshev, facing, normal_bias, offsets)
    w = np.stack([np.where(used, wj, _F(0.0)) for used, wj, _ in corners], axis=1).astype(_F)
    return w, np.stack([probe for _, _, probe in corners], axis=1)


def lookup_placed(grid, res, depth, points, dirs, normals=None, mode="irradiance", usable=None, chebyshev=True, facing=True, normal_bias=0.0, offsets=None):
    """lookup_vis() for probes that have moved: offsets float32 (nprobes, 3), and the probe position that enters v = p_b - position is
    (origin_a + float32(i_a) * spacing_a) + offset_a.  The cell, the fractions and the trilinear factor still come from the grid.  offsets None is lookup_vis on
    every bit; with chebyshev and facing off no position is used and it is lookup on every bit.  Returns (rgb float32 (m, 3), ok uint8 (m,))."""
    if mode not in MODES:
        raise ValueError("mode: one of %s, not %r" % (tuple(MODES), mode))
    m, corners = _placed(grid, res, depth, points, normals, usable, chebyshev, facing, normal_bias, offsets)
    nprobes = np.asarray(res["n"]).size
    n = np.ascontiguousarray(res["n"], np.uint32).reshape(nprobes)
    sh = np.ascontiguousarray(res["sh"], _F).reshape(nprobes, 27)
    dirs = np.ascontiguousarray(dirs, _F).reshape(m, 3)
    Cq = np.zeros((m, 27), _F); wsum = np.zeros(m, _F); ok = np.zeros(m, bool)
    with np.errstate(all="ignore"):
        for used, wj, probe in corners:
            s = wj * (SPHERE / n[probe].astype(_F))
            wsum = np.where(used, wsum + wj, wsum)
            Cq = np.where(used[:, None], Cq + s[:, None] * sh[probe], Cq)
            ok |= used
        b = basis(dirs)
        rr = np.zeros((m, 3), _F)
        for k in range(9):
            ck = Cq[:, 3 * k:3 * k + 3]
            rr = rr + ((A[k] * ck) if mode == "irradiance" else ck) * b[:, k, None]
        rgb = np.where(ok[:, None], rr / wsum[:, None], _F(0.0)).astype(_F)
    return rgb, ok.astype(np.uint8)


def relocate(rt, grid, rounds=4, spp=64, back_share=BACK_SHARE, max_offset=MAX_OFFSET, min_front=None, max_distance=None, flip=False, ids=None, device=None):
    """Move the probes of a grid out of geometry and say what became of each.  rt: a RayTracer (anything with its probes_survey and probes_place).  From zero
    offsets, per round r: survey at grid_points(grid) + offsets (one f32 addition per component) with the sample numbers r * spp .. r * spp + spp - 1, then
    place; after the last round one more survey (first_sample rounds * spp) and classify.  min_front None: grid_min_front(grid); max_distance None:
    grid_max_distance(grid).  device: a torch device of the handle's GPU — then every array is a tensor there and nothing leaves the GPU between the rounds.
    Returns dict(offsets float32 (nprobes, 3), state uint8 (nprobes,), usable uint8 (nprobes,), points float32 (nprobes, 3), verdict uint8 (nprobes,) of the
    last round, survey: the last survey)."""
    min_front = grid_min_front(grid) if min_front is None else min_front
    max_distance = grid_max_distance(grid) if max_distance is None else max_distance
    gp = grid_points(grid)
    offsets, verdict = np.zeros_like(gp), np.zeros(len(gp), np.uint8)
    if device is not None:
        import torch
        gp, offsets, verdict = torch.from_numpy(gp).to(device), torch.from_numpy(offsets).to(device), torch.from_numpy(verdict).to(device)
        if ids is not None and isinstance(ids, np.ndarray):
            ids = torch.from_numpy(np.ascontiguousarray(ids, np.uint32).view(np.int32)).to(device)
    kw = dict(back_share=back_share, max_offset=max_offset, min_front=min_front)
    for r in range(int(rounds) + 1):
        points = gp + offsets
        sv = rt.probes_survey(points, ids, spp=spp, first_sample=r * int(spp), max_distance=max_distance, flip=flip)
        if r < int(rounds):
            offsets, verdict = rt.probes_place(grid, sv, offsets, want=("offsets", "verdict"), **kw)
    state = rt.probes_place(grid, sv, None, want=("state",), **kw)[0]
    return dict(offsets=offsets, state=state, usable=usable_states(state), points=points, verdict=verdict, survey=sv)
