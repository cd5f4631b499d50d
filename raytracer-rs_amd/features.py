"""The feature film (include/mi355rt.h "FEATURE FILM") restated in numpy float32, with no device.

The library accumulates on the device (kernels.hip, features_kernel) and converts the sums into guides there (features_guides_kernel); this is the
same contract, operation for operation in f32 (numpy does not fuse), so the two must agree bit for bit:

    accumulate(planes, tuv, prim, scene, spp)   hits of the samples' rays -> the planes after the call
    guides(planes)                              the guide dict raytracer_rs_amd.denoise takes (MI355RT_GUIDES_FEATURES)
    alpha(planes)                               hits / n

The rays and their hits are the caller's business: RayTracer.lens_rays(spp) on a film whose n equals the feature film's gives the rays of
features.render(spp), and any intersector that answers as mi355rt_intersect_rays does (the CPU oracle in the tests) gives (tuv, prim)."""
import numpy as np

F = np.float32
MISS = 0xFFFFFFFF


def empty(npix):
    """the planes of a cleared feature film: dict(n, hits uint32[npix]; depth float32[npix]; normal, albedo float32[npix, 3])"""
    return dict(n=np.zeros(npix, np.uint32), hits=np.zeros(npix, np.uint32), depth=np.zeros(npix, np.float32),
                normal=np.zeros((npix, 3), np.float32), albedo=np.zeros((npix, 3), np.float32))


def tri_normals(scene):
    """calc_normal (mod.rs:198-205) in vecmath.rs order: cross(v1 - v0, v2 - v0), then normalized (sqrt((x*x + y*y) + z*z), three divisions)"""
    v = np.asarray(scene["tri_verts"], np.float32).reshape(-1, 9)
    a = v[:, 3:6] - v[:, 0:3]; b = v[:, 6:9] - v[:, 0:3]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    with np.errstate(all="ignore"):
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
        return np.stack([cx / ln, cy / ln, cz / ln], axis=1).astype(np.float32)


def fetch_texel(tex, u, v):
    """texture.rs:21-27 as the library restates it: `as usize` truncation (NaN and negatives -> 0), the index clamped to the last texel"""
    tex = np.asarray(tex, np.float32)
    th, tw = tex.shape[0], tex.shape[1]
    n = tw * th
    with np.errstate(all="ignore"):
        fx = np.asarray(u, np.float32) * F(tw); fy = np.asarray(v, np.float32) * F(th)
        x = np.where(fx > 0, np.minimum(fx, F(n + 1)), F(0)).astype(np.int64)
        y = np.where(fy > 0, np.minimum(fy, F(n + 1)), F(0)).astype(np.int64)
    i = np.minimum(np.minimum(y, n) * tw + np.minimum(x, n), n - 1)
    return tex.reshape(-1, 3)[i]


def hit_attributes(tuv, prim, scene):
    """(normal float32[k, 3], albedo float32[k, 3]) of k hits: the triangle normal shading uses and shade()'s diffuse colour (the material colour, or
    its texture at the hit's (u, v)): N and A of GUIDES"""
    pi = np.asarray(prim).astype(np.int64)
    tuv = np.asarray(tuv, np.float32).reshape(-1, 3)
    geom = np.asarray(scene["tri_geom"], np.int64)[pi]
    kind = np.asarray(scene["mat_kind"])[geom]
    alb = np.asarray(scene["mat_rgb"], np.float32).reshape(-1, 3)[geom].copy()
    for m in np.unique(geom[kind == 1]):
        sel = geom == m
        alb[sel] = fetch_texel(scene["textures"][int(scene["mat_tex"][m])], tuv[sel, 1], tuv[sel, 2])
    return tri_normals(scene)[pi], alb


def accumulate(planes, tuv, prim, scene, spp, owned=None):
    """The planes after spp more samples per pixel.  tuv float32[spp * npix, 3] and prim uint32[spp * npix] are the hits of the samples' rays in
    mi355rt_render_rays layout (row s * npix + p; prim 0xFFFFFFFF: a miss, its tuv is not read).  Per pixel, in sample order: n += 1, and on a hit
    only hits += 1, depth = depth + t, normal = normal + N[prim], albedo = albedo + A — one f32 addition each, the plane's value on the left.
    owned: bool[npix], the pixels of the rows a striped handle owns (None: all); the others stay as they are.  `planes` is not modified."""
    out = {k: np.array(v, copy=True) for k, v in planes.items()}
    npix = out["n"].size
    tuv = np.asarray(tuv, np.float32).reshape(spp, npix, 3)
    prim = np.asarray(prim).reshape(spp, npix)
    assert prim.dtype == np.uint32, prim.dtype
    own = np.ones(npix, bool) if owned is None else np.asarray(owned, bool).reshape(npix)
    for s in range(spp):
        hit = (prim[s] != np.uint32(MISS)) & own
        nrm, alb = hit_attributes(tuv[s][hit], prim[s][hit], scene)
        out["n"][own] += np.uint32(1)
        out["hits"][hit] += np.uint32(1)
        out["depth"][hit] = out["depth"][hit] + tuv[s][hit, 0]
        out["normal"][hit] = out["normal"][hit] + nrm
        out["albedo"][hit] = out["albedo"][hit] + alb
    return out


def guides(planes):
    """dict(depth, normal, albedo, prim) as raytracer_rs_amd.denoise takes it: the means over the samples that hit.  hits == 0 (which includes n == 0): a
    miss guide (prim 0xFFFFFFFF, zeros); else inv = 1 / (float)hits, depth = dsum * inv, m = nsum * inv, albedo = asum * inv,
    len = sqrt((m.x*m.x + m.y*m.y) + m.z*m.z), normal = len > 0 ? m / len : 0 (three divisions), prim = 0."""
    h = np.asarray(planes["hits"]).reshape(-1)
    assert h.dtype == np.uint32, h.dtype
    hit = h != 0
    npix = h.size
    dsum = np.asarray(planes["depth"], np.float32).reshape(npix)
    nsum = np.asarray(planes["normal"], np.float32).reshape(npix, 3)
    asum = np.asarray(planes["albedo"], np.float32).reshape(npix, 3)
    g = dict(depth=np.zeros(npix, np.float32), normal=np.zeros((npix, 3), np.float32), albedo=np.zeros((npix, 3), np.float32),
             prim=np.where(hit, np.uint32(0), np.uint32(MISS)).astype(np.uint32))
    with np.errstate(all="ignore"):
        inv = (F(1) / h.astype(np.float32)).astype(np.float32)
        m = nsum * inv[:, None]
        ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        nrm = np.where((ln > F(0))[:, None], m / ln[:, None], F(0)).astype(np.float32)
        g["depth"][hit] = (dsum * inv)[hit]
        g["normal"][hit] = nrm[hit]
        g["albedo"][hit] = (asum * inv[:, None])[hit]
    return g


def alpha(planes):
    """float32[npix]: n == 0 ? 0 : (float)hits / (float)n, one IEEE division"""
    n = np.asarray(planes["n"]).reshape(-1); h = np.asarray(planes["hits"]).reshape(-1)
    assert n.dtype == np.uint32 and h.dtype == np.uint32
    with np.errstate(all="ignore"):
        a = h.astype(np.float32) / n.astype(np.float32)
    return np.where(n == 0, F(0), a).astype(np.float32)
