"""The relit read-out of the light films, stated in numpy (include/mi355rt.h, "LIGHT FILMS").  Usable without a GPU on arrays:
light float32[nlights, npix, 3] (RayTracer.light_films.get()), n uint32[npix] (the film's counts), weights [nlights] or [nlights, 3].

Every operation is one f32 operation, in the order the header writes it: per pixel and channel
    inv = 1 / (float)n;  c = +0;  for li ascending:  m = light[li] * inv;  c = c + weights[li] * m
Nothing is special for n == 0: 0 * inf is NaN, and a NaN packs to white.  The mapping of c to 0xAARRGGBB is display.py's."""
import numpy as np

from . import display

F = np.float32


def weights3(weights, nlights):
    """weights as float32[nlights, 3]: a scalar per light is its factor for all three channels"""
    w = np.asarray(weights, np.float32)
    if w.ndim == 1:
        w = np.repeat(w[:, None], 3, axis=1)
    w = np.ascontiguousarray(w.reshape(-1, 3), np.float32)
    if w.shape != (nlights, 3):
        raise ValueError("weights: shape must be (%d,) or (%d, 3), not %s" % (nlights, nlights, np.shape(weights)))
    return w


def relit(light, n, weights):
    """c float32[npix, 3]: the rgb of mi355rt_get_relit_pixels"""
    light = np.asarray(light)
    n = np.asarray(n).reshape(-1)
    assert light.dtype == np.float32 and light.ndim == 3 and light.shape[2] == 3, (light.dtype, light.shape)
    assert n.dtype == np.uint32 and light.shape[1] == n.size, (n.dtype, light.shape, n.size)
    w = weights3(weights, light.shape[0])
    c = np.zeros((n.size, 3), np.float32)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / n.astype(np.float32)).astype(np.float32)
        for li in range(light.shape[0]):
            m = (light[li] * inv[:, None]).astype(np.float32)
            c = (c + (w[li][None, :] * m).astype(np.float32)).astype(np.float32)
    return c


def relit_pixels(light, n, weights, thresholds=None, **display_cfg):
    """(rgb float32[npix, 3], packed uint32[npix], exposure_used float32) of mi355rt_get_relit_pixels.  display_cfg: display config fields; none given is
    display == NULL, the reference's tone map of c (display.py's default mapping).  auto_exposure=1 takes E from the histogram of c, with n deciding `empty`."""
    cfg = dict(display.DEFAULTS)
    unknown = set(display_cfg) - set(cfg)
    if unknown:
        raise ValueError("unknown display config fields: %s" % sorted(unknown))
    cfg.update(display_cfg)
    if cfg["source"] != display.SOURCE_FILM:
        raise ValueError("the relit image has no denoised source: source must be SOURCE_FILM")
    c = relit(light, n, weights)
    E = F(cfg["exposure"])
    if cfg["auto_exposure"]:
        E = display.auto_exposure(display.histogram(c, np.asarray(n).reshape(-1)), cfg["key"], cfg["low"], cfg["high"])
    packed = display.display(c, exposure=E, curve=cfg["curve"], transfer=cfg["transfer"], white=cfg["white"], thresholds=thresholds)
    return c, packed, F(E)
