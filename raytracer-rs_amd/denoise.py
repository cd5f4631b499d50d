"""The denoised read-out (include/mi355rt.h) restated in numpy float32.

The library filters on the device (kernels.hip, denoise_init_kernel / denoise_iter_kernel); this is the same contract evaluated on a film
read back with RayTracer.film.pixel_datas() and on guide buffers (RayTracer.guides(), or built by the caller), operation for operation in
f32 (numpy does not fuse), so the two must agree bit for bit.  Used by the tests and by tools that want the filter without a device."""
import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
K1 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], np.float32)
DEFAULTS = dict(iterations=5, normal_power_log2=7, sigma_luminance=1.0, sigma_depth=0.1, sigma_albedo=0.1)   # mi355rt_denoise_default_config


def pos(x):
    """x > 0 ? x : 0, elementwise (NaN -> 0)"""
    return np.where(x > F(0), x, F(0)).astype(np.float32)


def _f32(a, shape):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.reshape(shape)


def film_inputs(s, q, n):
    """(c float32[npix, 3], var float32[npix]) of the film sums s, squares q and counts n"""
    s = _f32(s, (-1, 3)); q = _f32(q, (-1, 3))
    n = np.asarray(n).reshape(-1)
    assert n.dtype == np.uint32, n.dtype
    fn = n.astype(np.float32)[:, None]
    with np.errstate(all="ignore"):
        c = s * (F(1) / fn)
        v = pos(fn * q - s * s) / ((fn * fn) * (fn - F(1)))
        var = (v[:, 0] + v[:, 1]) + v[:, 2]
    return c, np.where(n >= 2, var, F(0)).astype(np.float32)


def iterate(c, var, empty, unknown, hit, normal, depth, albedo, width, height, step, normal_power_log2, sigma_luminance, sigma_depth, sigma_albedo):
    """one a-trous iteration of step h = `step`: the next (c, var)"""
    npix = width * height
    p = np.arange(npix)
    y, x = np.divmod(p, width)
    sl2 = F(sigma_luminance) * F(sigma_luminance)
    sd, sa = F(sigma_depth), F(sigma_albedo)
    N, t, A = normal, depth, albedo
    W = np.zeros(npix, np.float32); S = np.zeros((npix, 3), np.float32); V = np.zeros(npix, np.float32)
    with np.errstate(all="ignore"):
        lp = (F(0.2126) * c[:, 0] + F(0.7152) * c[:, 1]) + F(0.0722) * c[:, 2]
        sz = sd * t
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qx, qy = x + dx * step, y + dy * step
                inb = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
                q = np.where(inb, qy * width + qx, p)
                ok = inb & ~empty[q] & ~empty
                k = K1[dx + 2] * K1[dy + 2]
                cq, vq = c[q], var[q]
                if dx == 0 and dy == 0:
                    w = np.full(npix, k, np.float32)
                else:
                    ok &= hit == hit[q]                                   # exactly one of p, q a miss: skipped
                    Nq, Aq = N[q], A[q]
                    wn = pos((N[:, 0] * Nq[:, 0] + N[:, 1] * Nq[:, 1]) + N[:, 2] * Nq[:, 2])
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    rz = np.abs(t - t[q]) / sz
                    wz = F(1) / (F(1) + rz * rz)
                    ra = ((np.abs(A[:, 0] - Aq[:, 0]) + np.abs(A[:, 1] - Aq[:, 1])) + np.abs(A[:, 2] - Aq[:, 2])) / sa
                    wa = F(1) / (F(1) + ra * ra)
                    g = np.where(hit, (wn * wz) * wa, F(1))               # both miss: 1
                    dl = lp - ((F(0.2126) * cq[:, 0] + F(0.7152) * cq[:, 1]) + F(0.0722) * cq[:, 2])
                    wl = F(1) / (F(1) + (dl * dl) / (sl2 * (var + vq) + F(1e-12)))
                    wl = np.where(unknown | unknown[q], F(1), wl)
                    w = pos((k * g) * wl)
                S = np.where(ok[:, None], S + w[:, None] * cq, S)
                W = np.where(ok, W + w, W)
                V = np.where(ok, V + (w * w) * vq, V)
        c2 = np.where(empty[:, None], c, S / W[:, None]).astype(np.float32)
        v2 = np.where(empty, var, V / (W * W)).astype(np.float32)
    return c2, v2


def pack(c):
    """uint32[npix] 0xAARRGGBB of film means c, as get_tonemapped_pixels maps them (c/(1+c); NaN -> 255)"""
    c = _f32(c, (-1, 3))
    with np.errstate(all="ignore"):
        m = c / (F(1) + c)
        u = (np.fmax(np.fmin(m, F(1)), F(0)) * F(255)).astype(np.uint32) & np.uint32(0xFF)
    return (u[:, 2] | (u[:, 1] << np.uint32(8)) | (u[:, 0] << np.uint32(16)) | np.uint32(0xFF000000)).astype(np.uint32)


def denoise(s, q, n, guides, width, height, iterations, normal_power_log2, sigma_luminance, sigma_depth, sigma_albedo):
    """(rgb float32[npix, 3], packed uint32[npix]) of the film (s, q, n) with guides = dict(depth, normal, albedo, prim)"""
    npix = width * height
    c, var = film_inputs(s, q, n)
    assert c.shape[0] == npix
    n = np.asarray(n).reshape(-1)
    prim = np.asarray(guides["prim"]).reshape(-1)
    assert prim.dtype == np.uint32, prim.dtype
    normal = _f32(guides["normal"], (-1, 3)); albedo = _f32(guides["albedo"], (-1, 3)); depth = _f32(guides["depth"], (-1,))
    empty, unknown, hit = n == 0, n == 1, prim != np.uint32(MISS)
    for i in range(iterations):
        c, var = iterate(c, var, empty, unknown, hit, normal, depth, albedo, width, height, 1 << i, normal_power_log2,
                         sigma_luminance, sigma_depth, sigma_albedo)
    return c, pack(c)


def denoise_split(s, q, n, d, guides, width, height, iterations, normal_power_log2, sigma_luminance, sigma_depth, sigma_albedo):
    """(rgb, packed) of the split read-out (mi355rt_get_denoised_pixels_split): d float32[npix, 3] is the direct film
    (RayTracer.film.direct_sums()); the indirect part (s - d) / n is filtered under the total's variance and d / n is added back"""
    npix = width * height
    c, var = film_inputs(s, q, n)
    assert c.shape[0] == npix
    if iterations == 0:
        return c, pack(c)                                                     # the film mean itself, not cd + (c - cd)
    d = _f32(d, (-1, 3))
    n = np.asarray(n).reshape(-1)
    prim = np.asarray(guides["prim"]).reshape(-1)
    assert prim.dtype == np.uint32, prim.dtype
    normal = _f32(guides["normal"], (-1, 3)); albedo = _f32(guides["albedo"], (-1, 3)); depth = _f32(guides["depth"], (-1,))
    empty, unknown, hit = n == 0, n == 1, prim != np.uint32(MISS)
    with np.errstate(all="ignore"):
        cd = d * (F(1) / n.astype(np.float32)[:, None])
        ci = np.where(empty[:, None], c, c - cd).astype(np.float32)            # an empty pixel keeps its mean as it stands
    for i in range(iterations):
        ci, var = iterate(ci, var, empty, unknown, hit, normal, depth, albedo, width, height, 1 << i, normal_power_log2,
                          sigma_luminance, sigma_depth, sigma_albedo)
    with np.errstate(all="ignore"):
        out = np.where(empty[:, None], ci, cd + ci).astype(np.float32)
    return out, pack(out)
