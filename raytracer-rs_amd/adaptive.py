"""Adaptive sampling's tile verdict (include/mi355rt.h) restated in numpy float32.

The library decides on the device (kernels.hip, adaptive_tiles_kernel); this is the same contract evaluated on a film read back
with RayTracer.film.pixel_datas(), operation for operation in f32 (numpy does not fuse), so the two must agree bit for bit.  Used by
the tests and by tools that want to know which tiles the next round would render."""
import numpy as np

TILE = 8            # MI355RT_ADAPTIVE_TILE


def settled_pixels(s, q, n, min_spp, rel_error, abs_floor):
    """bool[npix]: the pixel is settled (s, q: [npix, 3] float32 sums and sums of squares; n: [npix] sample counts)"""
    s = np.asarray(s, np.float32).reshape(-1, 3)
    q = np.asarray(q, np.float32).reshape(-1, 3)
    n = np.asarray(n, np.uint32).reshape(-1)
    fn = n.astype(np.float32)[:, None]
    rel = np.float32(rel_error)
    with np.errstate(all="ignore"):
        lhs = fn * q - s * s
        m = np.maximum(s, np.float32(abs_floor) * fn)
        rhs = (rel * rel) * ((fn - np.float32(1.0)) * (m * m))
        ok = (lhs <= rhs).all(axis=1)             # a NaN fails the comparison
    return ok & (n >= 2) & (n >= min_spp)


def tile_mask(s, q, n, width, height, min_spp, max_spp, batch_spp, rel_error, abs_floor, owned_rows=None, **_ignored):
    """uint8[tiles_y, tiles_x]: 1 where the tile is active (owned_rows: the handle's rows; None = every row)"""
    tx, ty = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    n = np.asarray(n, np.uint32).reshape(-1)
    owned = np.zeros(height, bool)
    owned[np.arange(height) if owned_rows is None else np.asarray(owned_rows, np.int64)] = True
    own = np.broadcast_to(owned[:, None], (height, width))
    unsettled = (~settled_pixels(s, q, n, min_spp, rel_error, abs_floor)).reshape(height, width) & own
    nn = np.where(own, n.reshape(height, width).astype(np.uint64), np.uint64(0))
    ph, pw = ty * TILE, tx * TILE
    pad_u = np.zeros((ph, pw), bool); pad_u[:height, :width] = unsettled
    pad_n = np.zeros((ph, pw), np.uint64); pad_n[:height, :width] = nn
    busy = pad_u.reshape(ty, TILE, tx, TILE).any(axis=(1, 3))
    max_n = pad_n.reshape(ty, TILE, tx, TILE).max(axis=(1, 3))
    return (busy & (max_n + np.uint64(batch_spp) <= np.uint64(max_spp))).astype(np.uint8)


def pixel_tiles(width, height):
    """int[height, width]: the tile index ty * tiles_x + tx of every pixel"""
    tx = (width + TILE - 1) // TILE
    y, x = np.mgrid[0:height, 0:width]
    return (y // TILE) * tx + x // TILE


def region_mask(width, height, x0, y0, x1, y1):
    """uint8[tiles_y, tiles_x]: 1 for the tiles the half-open pixel rectangle [x0, x1) x [y0, y1) touches, clipped to the image; an empty rectangle
    gives an all-zero mask (the mask of RayTracer.render_tiles: a crop or a region of interest)"""
    tx, ty = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    out = np.zeros((ty, tx), np.uint8)
    x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), width), min(int(y1), height)
    if x0 < x1 and y0 < y1:
        out[y0 // TILE:(y1 - 1) // TILE + 1, x0 // TILE:(x1 - 1) // TILE + 1] = 1
    return out


def refine(rt, **cfg):
    """The loop of mi355rt_render_adaptive run on the caller's side, from two calls that work under any lens (include/mi355rt.h, RENDER TILES): take the
    verdict with rt.adaptive_tile_mask(**cfg); stop when no tile is active or max_rounds rounds have run; otherwise rt.render_tiles(mask, batch_spp).
    Under the pinhole the film and the stats are render_adaptive's bit for bit; under a lens this is adaptive depth of field.  Fields not given keep
    mi355rt_adaptive_default_config's values.  Returns the keys of AdaptiveStats (rounds, tiles, tiles_active_first, tiles_active_last, samples_added —
    the sum of the calls' primary) and the rounds' summed primary, bounce, shadow and primary_hits."""
    from . import adaptive_config
    c = adaptive_config(**cfg)
    batch_spp, max_rounds = int(c.batch_spp), int(c.max_rounds)
    tx = (rt.width + TILE - 1) // TILE
    tile_rows = {int(r) // TILE for r in rt.owned_rows()}
    out = dict(rounds=0, tiles=len(tile_rows) * tx, tiles_active_first=0, tiles_active_last=0, samples_added=0, primary=0, bounce=0, shadow=0, primary_hits=0)
    while True:
        mask = rt.adaptive_tile_mask(**cfg)
        active = int(np.count_nonzero(mask))
        if out["rounds"] == 0:
            out["tiles_active_first"] = active
        out["tiles_active_last"] = active
        if active == 0 or (max_rounds and out["rounds"] >= max_rounds):
            break
        rc = rt.render_tiles(mask, batch_spp)
        out["rounds"] += 1
        for k in ("primary", "bounce", "shadow", "primary_hits"):
            out[k] += int(getattr(rc, k))
    out["samples_added"] = out["primary"]
    return out
