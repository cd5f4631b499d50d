"""The statement of a bake (include/mi355rt.h, "BAKE") in numpy: UV charts to texels and surface points, per-point values back into an
atlas with filled borders, a chart generator for meshes that have none, and the three atlases of RayTracer.bake.

Host code, float32 with every rounding explicit, no GPU:

    texels(uv, width, height, scene, flip)      owner, bary and the compact lists ids / points / normals / albedo     (what mi355rt_bake_texels makes)
    atlas(ids, values, width, height, dilate)   the values scattered, then the dilation                               (mi355rt_bake_atlas)
    auto_atlas(ntri, width, height, gutter)     two triangles per square cell                                         (mi355rt_bake_auto_atlas)
    indirect(res), radiance(albedo, direct, res)    sum / n, and albedo * direct + indirect

Conventions: u runs to the right and v downwards; texel (x, y) has index y * width + x and its centre at (x + 0.5, y + 0.5).  Every expression below is
f32, unfused, in the order written: csrc/bake_raster.hpp evaluates the same expressions on the host and in the kernels of csrc/bake.hip.
"""
import numpy as np

from . import features as _features
from . import gather as _gather

_F = np.float32
MISS = 0xFFFFFFFF


def _tri_px(uv6, width, height):
    """px_k = u_k * (float)width, py_k = v_k * (float)height"""
    uv6 = np.asarray(uv6, _F).reshape(3, 2)
    return uv6[:, 0] * _F(width), uv6[:, 1] * _F(height)


def box(px, py, width, height):
    """THE BOX: the texels a triangle is tested against, x in [floor(min px) - 1, floor(max px) + 1] and y alike, cut to the atlas; None: no texel (off the
    atlas, or a NaN or infinite coordinate: such a chart covers nothing).  An exactly covered centre has min px <= x + 0.5 <= max px and lies inside with a texel to spare; the box keeps a sliver
    from claiming a far centre that only the rounding of its edge functions gives it.  Returns (x0, x1, y0, y1), inclusive."""
    if not (np.isfinite(px).all() and np.isfinite(py).all()):
        return None
    with np.errstate(all="ignore"):
        lox, hix = np.floor(px.min()) - _F(1), np.floor(px.max()) + _F(1)
        loy, hiy = np.floor(py.min()) - _F(1), np.floor(py.max()) + _F(1)
    w, h = _F(width), _F(height)
    if not (lox < w) or not (hix >= 0) or not (loy < h) or not (hiy >= 0):
        return None
    return int(max(lox, _F(0))), int(min(hix, w - _F(1))), int(max(loy, _F(0))), int(min(hiy, h - _F(1)))


def edges(px, py, x, y):
    """(e0, e1, e2, s) at the centres of the texels (x, y) (arrays): edge(p, q) = (px_p - cx) * (py_q - cy) - (py_p - cy) * (px_q - cx), relative to the centre,
    so that edge(p, q) == -edge(q, p) exactly; e0 = edge(b, c), e1 = edge(c, a), e2 = edge(a, b), s = (e0 + e1) + e2"""
    cx = np.asarray(x).astype(_F) + _F(0.5)
    cy = np.asarray(y).astype(_F) + _F(0.5)
    with np.errstate(all="ignore"):
        ax, ay, bx, by, qx, qy = px[0] - cx, py[0] - cy, px[1] - cx, py[1] - cy, px[2] - cx, py[2] - cy
        e0 = bx * qy - by * qx
        e1 = qx * ay - qy * ax
        e2 = ax * by - ay * bx
        s = (e0 + e1) + e2
    return e0, e1, e2, s


def covered(e0, e1, e2, s):
    """both windings; NaN compares false and covers nothing; a centre on an edge or a vertex counts"""
    with np.errstate(all="ignore"):
        return (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & (s != 0)


def owners(uv, width, height):
    """(owner uint32 (height * width,), bary float32 (height * width, 2)): per texel the LOWEST triangle index that covers its centre (MISS: none) and
    u = e1 / s, v = e2 / s of that triangle (the weights of vertices 1 and 2, as the hit record's u, v; 0 where uncovered)"""
    uv = np.ascontiguousarray(uv, _F).reshape(-1, 3, 2)
    owner = np.full((height, width), MISS, np.uint32)
    bary = np.zeros((height, width, 2), _F)
    for i in range(uv.shape[0]):
        px, py = _tri_px(uv[i], width, height)
        b = box(px, py, width, height)
        if b is None:
            continue
        x0, x1, y0, y1 = b
        ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        e0, e1, e2, s = edges(px, py, xs, ys)
        m = covered(e0, e1, e2, s) & (owner[y0:y1 + 1, x0:x1 + 1] == MISS)          # ascending i: the first to cover a texel keeps it
        if not m.any():
            continue
        with np.errstate(all="ignore"):
            u, v = e1 / s, e2 / s
        owner[y0:y1 + 1, x0:x1 + 1][m] = i
        bary[y0:y1 + 1, x0:x1 + 1, 0][m] = u[m]
        bary[y0:y1 + 1, x0:x1 + 1, 1][m] = v[m]
    return owner.reshape(-1), bary.reshape(-1, 2)


def texels(uv, width, height, scene=None, flip=False):
    """mi355rt_bake_texels.  uv: float32 (ntri, 3, 2), one UV triangle per scene triangle.  Returns dict(owner, bary, ids, ncovered) and, with a scene (the dict
    scene_io loads), points, normals, albedo: the compact lists of the covered texels in ascending texel index.  ids: the texel index.
    P = (A + u * (B - A)) + v * (C - A) per component; normal: calc_normal (mod.rs:198-205), negated with flip; albedo: the material's diffuse colour or its
    texture's texel at (u, v) (features.hit_attributes)."""
    owner, bary = owners(uv, width, height)
    ids = np.nonzero(owner != MISS)[0].astype(np.uint32)
    out = dict(owner=owner, bary=bary, ids=ids, ncovered=int(ids.size))
    if scene is None:
        return out
    tri = owner[ids].astype(np.int64)
    u, v = bary[ids, 0], bary[ids, 1]
    verts = np.asarray(scene["tri_verts"], _F).reshape(-1, 9)
    a, e1, e2 = verts[tri, 0:3], verts[tri, 3:6] - verts[tri, 0:3], verts[tri, 6:9] - verts[tri, 0:3]
    with np.errstate(all="ignore"):
        out["points"] = np.ascontiguousarray((a + u[:, None] * e1) + v[:, None] * e2, _F)
    tuv = np.stack([np.zeros_like(u), u, v], axis=1)
    nrm, alb = _features.hit_attributes(tuv, tri, scene)
    out["normals"] = np.ascontiguousarray(-nrm if flip else nrm, _F)
    out["albedo"] = np.ascontiguousarray(alb, _F)
    return out


_NEIGHBOURS = ((0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))      # (dx, dy): N, W, E, S, NW, NE, SW, SE


def atlas(ids, values, width, height, dilate=2):
    """mi355rt_bake_atlas.  Returns (atlas float32 (height * width, 3), valid uint8 (height * width,)): the values scattered (0 elsewhere, valid 1), then
    `dilate` times from the PREVIOUS iteration's image: an empty texel with a non-empty 8-neighbour becomes (((v0 + v1) + v2) + ...) / (float)count over
    the neighbours that exist and are not empty, in the order N, W, E, S, NW, NE, SW, SE; its valid becomes 1 + k in iteration k = 1, 2, ..., saturating
    at 255.  The borders do not wrap.  Ids >= width * height and repeated ids are refused (ValueError)."""
    ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
    values = np.ascontiguousarray(values, _F).reshape(ids.size, 3)
    n = width * height
    if (ids >= n).any():
        raise ValueError("an id is >= width * height")
    if np.unique(ids).size != ids.size:
        raise ValueError("an id is named twice")
    img = np.zeros((height, width, 3), _F)
    val = np.zeros((height, width), np.uint8)
    img.reshape(-1, 3)[ids] = values
    val.reshape(-1)[ids] = 1
    for k in range(1, min(int(dilate), max(width, height) - 1) + 1):   # after max(width, height) - 1 iterations nothing is left to fill: more are not run
        count = np.zeros((height, width), np.uint32)
        acc = np.zeros((height, width, 3), _F)
        for dx, dy in _NEIGHBOURS:
            # the texels (x, y) whose neighbour (x + dx, y + dy) exists
            ys0, ys1 = max(0, -dy), min(height, height - dy)
            xs0, xs1 = max(0, -dx), min(width, width - dx)
            if ys0 >= ys1 or xs0 >= xs1:
                continue
            nv = val[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx] != 0
            ni = img[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
            c = count[ys0:ys1, xs0:xs1]
            a = acc[ys0:ys1, xs0:xs1]
            first = nv & (c == 0)
            more = nv & (c != 0)
            with np.errstate(all="ignore"):
                a[first] = ni[first]
                a[more] = a[more] + ni[more]
            c[nv] += np.uint32(1)
        fill = (val == 0) & (count != 0)
        with np.errstate(all="ignore"):
            mean = acc / np.maximum(count, 1).astype(_F)[:, :, None]
        img = img.copy(); val = val.copy()
        img[fill] = mean[fill]
        val[fill] = min(1 + k, 255)
    return img.reshape(-1, 3), val.reshape(-1)


def auto_atlas(ntri, width, height, gutter=1):
    """mi355rt_bake_auto_atlas: float32 (ntri, 3, 2).  Two triangles per square cell of `cell` texels, cells row by row from the top left, cell the largest
    with (width // cell) * (height // cell) >= ceil(ntri / 2).  With g = gutter, L = cell - 2 g, d = max(g - 0.5, 0.5), leg = L - d and (ox, oy) the cell's
    corner, in texels:
        even i:  (ox + g, oy + g), (ox + g + leg, oy + g), (ox + g, oy + g + leg)
        odd i:   (ox + cell - g, oy + cell - g), (ox + cell - g - leg, oy + cell - g), (ox + cell - g, oy + cell - g - leg)
    and uv = texels / (float)size, one f32 division each.  The legs lie on texel borders and the hypotenuses on x + y = integer + 0.5: no centre is near an
    edge.  Refused (ValueError) when L < 1 + d: a half would own no texel."""
    ntri, width, height, gutter = int(ntri), int(width), int(height), int(gutter)
    if ntri <= 0:
        raise ValueError("ntri is 0")
    if width <= 0 or height <= 0 or width > 16384 or height > 16384:
        raise ValueError("width and height must be 1 .. 16384")
    if gutter < 0 or gutter > 16384:
        raise ValueError("gutter must be 0 .. 16384")
    cells = (ntri + 1) // 2
    cell = min(width, height)
    while cell and (width // cell) * (height // cell) < cells:
        cell -= 1
    g = _F(gutter)
    d = g - _F(0.5) if gutter else _F(0.5)
    if cell == 0 or _F(cell) - _F(2) * g < _F(1) + d:
        raise ValueError("the atlas is too small: a cell cannot give both of its triangles a texel (larger atlas, or smaller gutter)")
    cols = width // cell
    c = _F(cell)
    leg = (c - _F(2) * g) - d
    i = np.arange(ntri)
    ox = ((i // 2) % cols * cell).astype(_F)
    oy = ((i // 2) // cols * cell).astype(_F)
    odd = (i & 1) == 1
    ax = np.where(odd, (ox + c) - g, ox + g).astype(_F)
    ay = np.where(odd, (oy + c) - g, oy + g).astype(_F)
    bx = np.where(odd, ax - leg, ax + leg).astype(_F)
    cy = np.where(odd, ay - leg, ay + leg).astype(_F)
    w, h = _F(width), _F(height)
    uv = np.empty((ntri, 3, 2), _F)
    uv[:, 0, 0] = ax / w; uv[:, 0, 1] = ay / h
    uv[:, 1, 0] = bx / w; uv[:, 1, 1] = ay / h
    uv[:, 2, 0] = ax / w; uv[:, 2, 1] = cy / h
    return uv


def indirect(res):
    """sum / n per texel of the list (gather.mean): the bounce estimator at the point"""
    return _gather.mean(res)


def radiance(albedo, direct, res):
    """albedo * direct + indirect, f32, elementwise, unfused: under weight "mean" what the reference's compute_radiance shows at the point without the
    view-dependent highlight"""
    with np.errstate(all="ignore"):
        return np.asarray(albedo, _F) * np.asarray(direct, _F) + indirect(res)
