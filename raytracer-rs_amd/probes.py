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
