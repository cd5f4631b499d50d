"""The statement of RayTracer.probe_lit_points / probe_lit_rays / render_probe_lit (include/mi355rt.h, "PROBE-LIT") in numpy.

Host code, float32 with every rounding explicit, no GPU.  The reference's compute_radiance (mod.rs:132-176) returns shade() + (1 / num_sub) * the sum of the
children's radiance: the bounce term is the UNIFORM mean of the radiance arriving over the hemisphere of the triangle normal, not cosine-weighted and not
multiplied by albedo.  For a field held as SH coefficients that mean is a zonal convolution with the band factors 1, 1/2, 0, so a probe-lit sample is

    shade() at the closest hit, with shadow rays   +   the hemisphere mean of a probe volume there

and only coefficients 0 .. 3 of a probe are read:

    volume(grid, res, depth, usable, offsets, ...)        everything probes.lookup_placed takes of a grid, as one dict
    hemi(volume, points, normals, clamp)                  the hemisphere mean at surface points                    (what hemi_one of csrc/probe_lit_math.hpp does)
    shade(scene, rays6, tuv, prim, blocked)               the reference's shade() at the rays' hits                (shade_one)
    rays(scene, volume, rays6, tuv, prim, blocked, clamp) the whole call per ray, given the intersector's answers  (probe_lit_shade_kernel)
    frame_mean(rgb, npix)                                 the mean over a pixel's samples, layout s * npix + p

Every expression below is f32, unfused, in the order written: csrc/probe_lit_math.hpp and the kernels of csrc/probe_lit.hip evaluate the same expressions.
"""
import numpy as np

from . import features as _features
from . import gather as _gather
from . import probes as _probes

_F = np.float32
MISS = 0xFFFFFFFF
CLAMP = 1                                                       # MI355RT_PROBE_LIT_CLAMP
HALF = _F(0.5)                                                  # band 1 of the uniform hemisphere mean; band 0 is 1, band 2 is 0
OUTPUTS = ("rgb", "light", "indirect", "tuv", "prim", "ok")


def volume(grid, res, depth=None, usable=None, offsets=None, chebyshev=True, facing=True, normal_bias=0.0):
    """A probe volume: dict(grid, n, sh, usable, depth, offsets, chebyshev, facing, normal_bias).  res: a dict with n uint32 (nprobes,) and sh float32
    (nprobes, 9, 3) (probes_gather returns it).  depth: None, or a dict with count and moments and their resolution under "res" or "depth_res" (what
    probes_gather_depth returns serves: volume(grid, res, depth=res)).  usable: uint8 (nprobes,) or None.  offsets: float32 (nprobes, 3) or None, or the dict
    probes_relocate returns — then its "usable" is taken too unless one is given.  Without depth there is no visibility and no facing weight, and offsets must
    be None: the corner weights are the trilinear factors.  The arrays may be numpy arrays or torch tensors on the GPU, all alike."""
    if isinstance(offsets, dict):
        if usable is None:
            usable = offsets.get("usable")
        offsets = offsets["offsets"]
    d = None
    if depth is not None:
        R = depth["res"] if "res" in depth else depth["depth_res"]
        d = dict(res=_probes._res(R), count=depth["count"], moments=depth["moments"], max_distance=float(depth.get("max_distance", 1.0)))
    elif offsets is not None:
        raise ValueError("offsets: given without depth (without depth films no probe position is used)")
    return dict(grid=grid, n=res["n"], sh=res["sh"], usable=usable, depth=d, offsets=offsets, chebyshev=bool(chebyshev) and d is not None,
                facing=bool(facing) and d is not None, normal_bias=float(normal_bias) if d is not None else 0.0)


def _corners(vol, points, normals):
    """(m, corners) of probes._placed for the volume; without depth the weights are lookup's t_j (no visibility, no facing, no position)"""
    res = dict(n=vol["n"], sh=vol["sh"])
    depth = vol["depth"]
    if depth is None:
        nprobes = int(np.asarray(vol["n"]).size)
        depth = dict(res=2, count=np.zeros((nprobes, 4), np.uint32), moments=np.zeros((nprobes, 4, 2), _F))
        return _probes._placed(vol["grid"], res, depth, points, normals, vol["usable"], False, False, 0.0, None)
    return _probes._placed(vol["grid"], res, depth, points, normals, vol["usable"], vol["chebyshev"], vol["facing"], vol["normal_bias"], vol["offsets"])


def hemi(vol, points, normals, clamp=True):
    """The uniform mean over the hemisphere of `normals` of the field the volume holds, at points float32 (m, 3).  The corners, their skipping rules, wsum and
    the weight w_j are exactly those of probes.lookup_placed(points, dirs=normals, normals=normals) (of probes.lookup without depth).  Per used corner, in j
    order from 0: s_j = w_j * (4 pi / n_j); C[k][c] += s_j * sh_j[k][c] for k = 0 .. 3 only — coefficients 4 .. 8 are never read.  Then, the sum from 0 in k order,
    m_c = ((C[0][c] * b_0 + (0.5 * C[1][c]) * b_1(N)) + (0.5 * C[2][c]) * b_2(N)) + (0.5 * C[3][c]) * b_3(N); x_c = m_c / wsum; clamp: x_c >= 0 ? x_c : 0 (a NaN
    becomes 0).  Returns (indirect float32 (m, 3), ok uint8 (m,)); no corner used: indirect 0, ok 0."""
    points = np.ascontiguousarray(points, _F).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, _F).reshape(points.shape[0], 3)
    m, corners = _corners(vol, points, normals)
    nprobes = int(np.asarray(vol["n"]).size)
    n = np.ascontiguousarray(vol["n"], np.uint32).reshape(nprobes)
    sh = np.ascontiguousarray(vol["sh"], _F).reshape(nprobes, 27)[:, :12]
    Cq = np.zeros((m, 12), _F); wsum = np.zeros(m, _F); ok = np.zeros(m, bool)
    with np.errstate(all="ignore"):
        for used, wj, probe in corners:
            s = wj * (_probes.SPHERE / n[probe].astype(_F))
            wsum = np.where(used, wsum + wj, wsum)
            Cq = np.where(used[:, None], Cq + s[:, None] * sh[probe], Cq)
            ok |= used
        b = _probes.basis(normals)
        r = np.zeros((m, 3), _F)
        r = r + Cq[:, 0:3] * b[:, 0, None]
        for k in (1, 2, 3):
            r = r + (HALF * Cq[:, 3 * k:3 * k + 3]) * b[:, k, None]
        x = r / wsum[:, None]
        if clamp:
            x = np.where(x >= _F(0.0), x, _F(0.0))
        out = np.where(ok[:, None], x, _F(0.0)).astype(_F)
    return out, ok.astype(np.uint8)


def pow32(x):
    """x.powf(32.0) as the library has it (mod.rs:255): five squarings in f64 and one rounding"""
    d = np.asarray(x, _F).astype(np.float64)
    with np.errstate(all="ignore"):
        for _ in range(5):
            d = d * d
        return d.astype(_F)


def hit_points(rays6, tuv):
    """P = pos + t * dir per ray: one multiply and one add per axis (mod.rs:212)"""
    rays6 = np.ascontiguousarray(rays6, _F).reshape(-1, 6)
    t = np.ascontiguousarray(tuv, _F).reshape(-1, 3)[:, 0]
    with np.errstate(all="ignore"):
        return (rays6[:, 0:3] + t[:, None] * rays6[:, 3:6]).astype(_F)


def shade(scene, rays6, tuv, prim, blocked):
    """The reference's shade() (mod.rs:207-261) at the hits of rays6 float32 (n, 6): the root light sum.  tuv float32 (n, 3) and prim uint32 (n,) as
    mi355rt_intersect_rays answers (a miss, prim 0xFFFFFFFF, gives 0); blocked: (nlights * n,) verdicts of mi355rt_occluded_rays for
    gather.shadow_rays(P, lights), entry li * n + i.  P = pos + t * dir; N and the diffuse colour are features.hit_attributes.  Per light, in scene order, from
    0: l = light - P; ln = normalized(l); ndl = dot(N, ln); ndl < 0: skipped; blocked: skipped; else refl = (2 * ndl) * N - ln,
    spec = pow32(dot(normalized(dir), refl)), accum += (diffuse * ndl + spec) * colour.  vecmath.rs operation order: dot = x * x' + y * y' + z * z' left to
    right, normalized = three divisions by sqrt(dot(v, v)).  Returns float32 (n, 3)."""
    rays6 = np.ascontiguousarray(rays6, _F).reshape(-1, 6)
    n = rays6.shape[0]
    tuv = np.ascontiguousarray(tuv, _F).reshape(n, 3)
    prim = np.ascontiguousarray(prim, np.uint32).reshape(n)
    lights = np.ascontiguousarray(scene["lights"], _F).reshape(-1, 6)
    blocked = np.asarray(blocked).reshape(lights.shape[0], n).astype(bool)
    hit = prim != np.uint32(MISS)
    out = np.zeros((n, 3), _F)
    if not hit.any():
        return out
    r, h = rays6[hit], tuv[hit]
    P = hit_points(r, h)
    N, diffuse = _features.hit_attributes(h, prim[hit], scene)

    def dot(a, b):
        return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]

    def normalized(a):
        return (a / np.sqrt(dot(a, a))[:, None]).astype(_F)

    acc = np.zeros((P.shape[0], 3), _F)
    with np.errstate(all="ignore"):
        view = normalized(r[:, 3:6])
        for li in range(lights.shape[0]):
            l = lights[li, 0:3][None, :] - P
            ln = normalized(l)
            ndl = dot(N, ln)
            lit = ~(ndl < _F(0.0)) & ~blocked[li][hit]
            refl = (_F(2.0) * ndl)[:, None] * N - ln
            spec = pow32(dot(view, refl))
            term = (diffuse * ndl[:, None] + spec[:, None]) * lights[li, 3:6][None, :]
            acc = np.where(lit[:, None], acc + term, acc).astype(_F)
    out[hit] = acc
    return out


def rays(scene, vol, rays6, tuv, prim, blocked, clamp=True, tuv_before=None):
    """The whole call per ray, given the intersector's answers: (tuv, prim) of mi355rt_intersect_rays for rays6 and blocked of mi355rt_occluded_rays for
    gather.shadow_rays(P, lights) (rows of misses are not read).  A miss: rgb = light = indirect = 0, ok = 0, tuv as it was (tuv_before, None: 0).  A hit:
    light = shade(), (indirect, ok) = hemi(volume, P, N) with N the triangle's normal, NOT flipped towards the viewer, rgb = light + indirect.  Returns
    dict(rgb, light, indirect, tuv float32 (n, 3); prim uint32 (n,); ok uint8 (n,); points, normals float32 (n, 3), 0 for a miss)."""
    rays6 = np.ascontiguousarray(rays6, _F).reshape(-1, 6)
    n = rays6.shape[0]
    tuv = np.ascontiguousarray(tuv, _F).reshape(n, 3)
    prim = np.ascontiguousarray(prim, np.uint32).reshape(n)
    hit = prim != np.uint32(MISS)
    light = shade(scene, rays6, tuv, prim, blocked)
    P = np.zeros((n, 3), _F); N = np.zeros((n, 3), _F)
    indirect = np.zeros((n, 3), _F); ok = np.zeros(n, np.uint8)
    if hit.any():
        P[hit] = hit_points(rays6[hit], tuv[hit])
        N[hit] = _features.tri_normals(scene)[prim[hit].astype(np.int64)]
        indirect[hit], ok[hit] = hemi(vol, P[hit], N[hit], clamp)
    out_tuv = np.zeros((n, 3), _F) if tuv_before is None else np.array(tuv_before, _F).reshape(n, 3)
    out_tuv[hit] = tuv[hit]
    with np.errstate(all="ignore"):
        rgb = (light + indirect).astype(_F)
    return dict(rgb=rgb, light=light, indirect=indirect, tuv=out_tuv, prim=prim.copy(), ok=ok, points=P, normals=N)


def shadow_rays(scene, rays6, tuv, prim):
    """gather.shadow_rays at the rays' hit points, unchanged, in the layout li * n + i; the rows of a miss are zeros (their verdict is never read)"""
    rays6 = np.ascontiguousarray(rays6, _F).reshape(-1, 6)
    n = rays6.shape[0]
    prim = np.ascontiguousarray(prim, np.uint32).reshape(n)
    hit = prim != np.uint32(MISS)
    lights = np.ascontiguousarray(scene["lights"], _F).reshape(-1, 6)
    out = np.zeros((lights.shape[0], n, 6), _F)
    if hit.any():
        P = hit_points(rays6[hit], np.ascontiguousarray(tuv, _F).reshape(n, 3)[hit])
        out[:, hit, :] = _gather.shadow_rays(P, lights).reshape(lights.shape[0], -1, 6)
    return out.reshape(-1, 6)


def frame_mean(rgb, npix):
    """The mean over each pixel's samples of rgb (spp * npix, c), layout s * npix + p: acc = 0; for s in order acc = acc + rgb[s * npix + p]; mean = acc /
    (float)spp.  One elementwise addition per sample and one division, so a numpy array and a torch tensor give the same bits.  Returns (npix, c)."""
    npix = int(npix)
    spp = rgb.shape[0] // npix
    if spp < 1 or spp * npix != rgb.shape[0]:
        raise ValueError("rgb: its rows must be a positive multiple of npix")
    if isinstance(rgb, np.ndarray):
        acc = np.zeros_like(rgb[:npix])
        with np.errstate(all="ignore"):
            for s in range(spp):
                acc = acc + rgb[s * npix:(s + 1) * npix]
            return (acc / _F(spp)).astype(rgb.dtype)
    import torch
    acc = torch.zeros_like(rgb[:npix])
    for s in range(spp):
        acc = acc + rgb[s * npix:(s + 1) * npix]
    return acc / torch.full_like(acc, float(spp))                 # a tensor, not a scalar: an elementwise IEEE division, never a multiplication by 1 / spp
