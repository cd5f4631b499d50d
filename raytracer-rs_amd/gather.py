"""The statement of RayTracer.gather / mi355rt_gather (include/mi355rt.h, "GATHER") in numpy.

Host code, float32 with every rounding explicit, no GPU.  The points are a film of their own: per point n, sum, sumsq (and hits, near), accumulated in
sample order over rays the renderer's own hemisphere sampler makes:

    rays(table, seed, points, normals, ids, first, spp)   the rays, keys, validity and weights of the samples     (what gather_rays_kernel makes)
    reduce(rgb, t, hit, valid, w, near_distance, prev)    the per-point sums from the traced rays' results         (what gather_reduce_kernel does)
    shadow_rays(points, lights), direct(...)              the unshadowed point-light term                          (gather_shadow_rays / gather_direct)
    mean(res), irradiance(res)                            sum / n, and pi * mean under weight "cosine"

Layout: sample-major, row s * npoints + i is sample s of point i (key (id_i, first + s)); rays() returns valid and w shaped (spp, npoints), reduce()
takes rgb / t / hit in that row order.  Every expression below is f32, unfused, in the order written: csrc/gather_walk.hpp and the gather kernels of
csrc/kernels.hip evaluate the same expressions.
"""
import numpy as np

from .cameras import pcg4d

_F = np.float32
SAMPLE_MAX = 65535            # the walk's modulus (sample_generator.rs:27): entries 0 .. 65534
STREAM = 0xFFFFFFFE           # hash word 2 of a gather sample: 0 is the jitter, 1 + child the tree, 0xFFFFFFFF the table
WEIGHTS = {"mean": 0, "cosine": 1}      # MI355RT_GATHER_*
_STEPS = 64                   # walk steps taken for all samples together before the stragglers are settled against the whole table


def table_index(h):
    """a hash word -> a table index in [0, 65534], as the bounce rays scale theirs (sample_generator.rs:32)"""
    return ((np.asarray(h, np.uint32).astype(np.uint64) * np.uint64(SAMPLE_MAX)) >> np.uint64(32)).astype(np.uint32)


def _dot(d, n):
    return d[..., 0] * n[..., 0] + d[..., 1] * n[..., 1] + d[..., 2] * n[..., 2]


def rays(table, seed, points, normals, ids, first, spp, weight="mean"):
    """The samples first .. first + spp - 1 of every point.  table: float32 (65536, 3) (RayTracer.sample_table()); points: (n, 3); normals: (n, 3) or None
    (sphere mode: no walk); ids: uint32 (n,) or None (i).  Returns (rays6 float32 (spp * n, 6), keys uint32 (spp * n, 2), valid uint8 (spp, n),
    w float32 (spp, n)).  The walk is reflection_ray's (mod.rs:187-189) from the hashed start entry, bounded to one full turn: a sample no entry
    satisfies is VOID (valid 0) and keeps the start entry as a harmless direction.  w: 1 ("mean") or 2 * dot(d, normal) ("cosine")."""
    if weight not in WEIGHTS:
        raise ValueError("weight: one of %s, not %r" % (tuple(WEIGHTS), weight))
    table = np.ascontiguousarray(table, _F).reshape(65536, 3)
    points = np.ascontiguousarray(points, _F).reshape(-1, 3)
    npts, spp = points.shape[0], int(spp)
    if normals is None and weight == "cosine":
        raise ValueError('weight "cosine" needs normals')
    ids = np.arange(npts, dtype=np.uint32) if ids is None else np.ascontiguousarray(ids, np.uint32).reshape(npts)
    with np.errstate(over="ignore"):
        sampleno = (np.uint32(int(first) & 0xFFFFFFFF) + np.arange(spp, dtype=np.uint32))[:, None]
    idb, snb = np.broadcast_arrays(ids[None, :], sampleno)
    start = table_index(pcg4d(idb, snb, np.uint32(STREAM), np.uint32(int(seed) & 0xFFFFFFFF))[0])
    valid = np.ones((spp, npts), np.uint8)
    jx = start.copy()
    if normals is not None:
        normals = np.ascontiguousarray(normals, _F).reshape(npts, 3)
        nb = np.broadcast_to(normals[None, :, :], (spp, npts, 3))
        jf, vf = jx.reshape(-1), valid.reshape(-1)             # views: sample e = s * npts + i
        with np.errstate(invalid="ignore", under="ignore"):
            act = np.nonzero((_dot(table[jf], nb.reshape(-1, 3)) <= _F(0.0)))[0]      # the samples still walking
            for _ in range(_STEPS):
                if act.size == 0:
                    break
                j = (jf[act] + np.uint32(1)) % np.uint32(SAMPLE_MAX)
                jf[act] = j
                act = act[_dot(table[j], normals[act % npts]) <= _F(0.0)]
            # the stragglers, one by one: the first accepted entry of the walk's cycle behind where they stand, or none on the whole turn: void
            for e in act:
                order = (np.arange(SAMPLE_MAX, dtype=np.int64) + int(jf[e])) % SAMPLE_MAX
                ok = np.nonzero(~(_dot(table[order], normals[e % npts]) <= _F(0.0)))[0]
                if ok.size:
                    jf[e] = order[ok[0]]
                else:
                    jf[e] = start.reshape(-1)[e]; vf[e] = 0
    d = table[jx]
    pb = np.broadcast_to(points[None, :, :], (spp, npts, 3))
    out = np.empty((spp, npts, 6), _F)
    for k in range(3):
        out[..., k] = pb[..., k] + _F(0.00001) * d[..., k]          # mod.rs:192-193
        out[..., 3 + k] = d[..., k]
    keys = np.stack([idb, snb], axis=-1).astype(np.uint32).reshape(-1, 2)
    if weight == "cosine":
        with np.errstate(invalid="ignore", under="ignore"):
            w = _F(2.0) * _dot(d, nb)
    else:
        w = np.ones((spp, npts), _F)
    return out.reshape(-1, 6), np.ascontiguousarray(keys), valid, np.ascontiguousarray(w, _F)


def reduce(rgb, t, hit, valid, w, near_distance=np.inf, prev=None):
    """Per point, in sample order, for every sample that is not void: v = w * rgb; sum += v; sumsq += v * v; n += 1; hits += hit; near += hit and
    t < near_distance.  rgb: float32 (spp * n, 3); t: float32 (spp * n,) (read where hit); hit: bool (spp * n,); valid, w: (spp, n) as rays() returns
    them.  prev: a dict of earlier results to add to (the accumulate of mi355rt_gather), None: from 0.  Returns dict(n, hits, near uint32 (n,); sum,
    sumsq float32 (n, 3))."""
    valid = np.asarray(valid)
    spp, npts = valid.shape
    rgb = np.ascontiguousarray(rgb, _F).reshape(spp, npts, 3)
    t = np.ascontiguousarray(t, _F).reshape(spp, npts)
    hit = np.asarray(hit).reshape(spp, npts).astype(bool)
    w = np.ascontiguousarray(w, _F).reshape(spp, npts)
    nd = _F(near_distance)
    res = {}
    for k, shape, dt in (("n", (npts,), np.uint32), ("hits", (npts,), np.uint32), ("near", (npts,), np.uint32), ("sum", (npts, 3), _F), ("sumsq", (npts, 3), _F)):
        res[k] = np.zeros(shape, dt) if prev is None or prev.get(k) is None else np.array(prev[k], dt).reshape(shape)
    with np.errstate(all="ignore"):
        for s in range(spp):
            m = valid[s] != 0
            v = w[s][:, None] * rgb[s]
            res["sum"][m] = res["sum"][m] + v[m]
            res["sumsq"][m] = res["sumsq"][m] + (v * v)[m]
            res["n"][m] += np.uint32(1)
            h = m & hit[s]
            res["hits"][h] += np.uint32(1)
            res["near"][h & (t[s] < nd)] += np.uint32(1)
    return res


def shadow_rays(points, lights):
    """The shadow rays of direct(): float32 (nlights * n, 6), row li * n + i = (p + l * 0.01, l) with l = light_li - p_i (mod.rs:215, 224-225), for every
    pair, whether or not the light lies behind the surface.  lights: float32 (nlights, 6) rows (pos3, color3), as scene["lights"]."""
    points = np.ascontiguousarray(points, _F).reshape(-1, 3)
    lights = np.ascontiguousarray(lights, _F).reshape(-1, 6)
    l = lights[:, None, 0:3] - points[None, :, :]
    out = np.empty((lights.shape[0], points.shape[0], 6), _F)
    out[..., 0:3] = points[None, :, :] + l * _F(0.01)
    out[..., 3:6] = l
    return out.reshape(-1, 6)


def direct(points, normals, lights, blocked):
    """The point-light term of shade() (mod.rs:207-261) without material and specular: over the lights in scene order, ndl = dot(normal, normalized(light - p));
    a light with ndl < 0 is skipped, a blocked one (blocked[li * n + i], mi355rt_occluded_rays of shadow_rays()) adds nothing, else direct += color * ndl.
    Returns float32 (n, 3)."""
    points = np.ascontiguousarray(points, _F).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, _F).reshape(-1, 3)
    lights = np.ascontiguousarray(lights, _F).reshape(-1, 6)
    blocked = np.asarray(blocked).reshape(lights.shape[0], points.shape[0]).astype(bool)
    acc = np.zeros((points.shape[0], 3), _F)
    with np.errstate(all="ignore"):
        for li in range(lights.shape[0]):
            l = lights[li, 0:3][None, :] - points
            length = np.sqrt(l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1] + l[:, 2] * l[:, 2])
            ln = l / length[:, None]
            ndl = normals[:, 0] * ln[:, 0] + normals[:, 1] * ln[:, 1] + normals[:, 2] * ln[:, 2]
            m = ~(ndl < _F(0.0)) & ~blocked[li]
            acc[m] = acc[m] + (lights[li, 3:6][None, :] * ndl[:, None])[m]
    return acc


def mean(res):
    """sum / n per point (NaN where n == 0): the reference's bounce estimator at the point under weight "mean" """
    with np.errstate(all="ignore"):
        return np.asarray(res["sum"], _F) / np.asarray(res["n"]).astype(_F)[:, None]


def irradiance(res):
    """pi * mean(res) of a gather under weight "cosine": the table is uniform on the sphere, the accepted half has density 1 / (2 pi), and
    w = 2 * dot(d, normal)"""
    return _F(np.pi) * mean(res)
