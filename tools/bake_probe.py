#!/usr/bin/env python3
"""What a bake costs, on thai2 with the auto atlas at 2048 x 2048 and 16 spp.

The parts of RayTracer.bake on device tensors, each timed on its own (bake_texels, the gather at its points, one bake_atlas), the whole bake, and two other
ways to the same texels, each followed by the same gather:
  numpy_host      bake.texels in numpy on the host (the statement), then gather from host arrays
  torch_device    the statement written in torch on the GPU: per batch of triangles every texel of their boxes, the lowest covering index by scatter-min, then
                  (u, v), the compaction and the points; then gather in place
Every way is timed to the point where its results are complete where it leaves them.  One JSON line per measurement: wall-clock ms, median (min - max) of
--reps rounds after one warm-up round (numpy_host: of --host-reps rounds, it takes minutes), and which results equal the library's on the bits.
usage: tools/bake_probe.py [--size 2048] [--spp 16] [--reps 5] [--host-reps 1] [--scene thai2]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MISS = 0xFFFFFFFF


def torch_texels(torch, uv, verts, normals, w, h, batch=4096):
    """bake.texels in torch on the device (no albedo): owner (int64, -1 for none is mapped to MISS on the host), bary, ids, points, normals"""
    dev = uv.device
    ntri = uv.shape[0]
    fw, fh = torch.tensor(float(w), dtype=torch.float32, device=dev), torch.tensor(float(h), dtype=torch.float32, device=dev)
    px, py = uv[:, :, 0] * fw, uv[:, :, 1] * fh
    big = torch.iinfo(torch.int64).max
    owner = torch.full((w * h,), big, dtype=torch.int64, device=dev)

    def edges(px, py, cx, cy):
        ax, ay, bx, by, qx, qy = px[:, 0] - cx, py[:, 0] - cy, px[:, 1] - cx, py[:, 1] - cy, px[:, 2] - cx, py[:, 2] - cy
        e0 = bx * qy - by * qx
        e1 = qx * ay - qy * ax
        e2 = ax * by - ay * bx
        return e0, e1, e2, (e0 + e1) + e2

    finite = torch.isfinite(px).all(dim=1) & torch.isfinite(py).all(dim=1)
    lox, hix = torch.floor(px.min(dim=1).values) - 1, torch.floor(px.max(dim=1).values) + 1
    loy, hiy = torch.floor(py.min(dim=1).values) - 1, torch.floor(py.max(dim=1).values) + 1
    ok = finite & (lox < w) & (hix >= 0) & (loy < h) & (hiy >= 0)
    x0, x1 = lox.clamp(min=0).nan_to_num(0).to(torch.int64), hix.clamp(max=w - 1).nan_to_num(0).to(torch.int64)
    y0, y1 = loy.clamp(min=0).nan_to_num(0).to(torch.int64), hiy.clamp(max=h - 1).nan_to_num(0).to(torch.int64)
    for b0 in range(0, ntri, batch):
        sl = slice(b0, min(b0 + batch, ntri))
        kx = int((x1[sl] - x0[sl] + 1).clamp(min=0).max()); ky = int((y1[sl] - y0[sl] + 1).clamp(min=0).max())
        if kx <= 0 or ky <= 0:
            continue
        oy, ox = torch.meshgrid(torch.arange(ky, device=dev), torch.arange(kx, device=dev), indexing="ij")
        xs = x0[sl, None] + ox.reshape(1, -1); ys = y0[sl, None] + oy.reshape(1, -1)
        inside = ok[sl, None] & (xs <= x1[sl, None]) & (ys <= y1[sl, None])
        cx, cy = xs.to(torch.float32) + 0.5, ys.to(torch.float32) + 0.5
        e0, e1, e2, s = edges(px[sl, :, None], py[sl, :, None], cx, cy)
        cov = inside & (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & (s != 0)
        tri = torch.arange(sl.start, sl.stop, device=dev)[:, None].expand_as(xs)
        owner.scatter_reduce_(0, (ys * w + xs)[cov], tri[cov], reduce="amin")
    ids = torch.nonzero(owner != big)[:, 0]
    t = owner[ids]
    cx, cy = (ids % w).to(torch.float32) + 0.5, (ids // w).to(torch.float32) + 0.5
    e0, e1, e2, s = edges(px[t], py[t], cx, cy)
    u, v = e1 / s, e2 / s
    a, b1, b2 = verts[t, 0:3], verts[t, 3:6] - verts[t, 0:3], verts[t, 6:9] - verts[t, 0:3]
    points = ((a + u[:, None] * b1) + v[:, None] * b2).contiguous()
    return dict(owner=owner, ids=ids.to(torch.int32), u=u, v=v, points=points, normals=normals[t].contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--scene", default="thai2")
    a = ap.parse_args()
    import torch
    torch.cuda.is_available()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    bake = importlib.import_module("raytracer_rs_amd.bake")
    features = importlib.import_module("raytracer_rs_amd.features")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", a.scene + ".scene"))
    ntri, w, h, spp = int(scene["tri_geom"].size), a.size, a.size, a.spp
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, 64, 64, seed=1)
    uv = bake.auto_atlas(ntri, w, h)
    dev = torch.device("cuda", 0)
    tuv = torch.from_numpy(uv).to(dev)
    tverts = torch.from_numpy(np.ascontiguousarray(scene["tri_verts"], np.float32)).to(dev)
    tnormals = torch.from_numpy(features.tri_normals(scene)).to(dev)
    torch.cuda.synchronize()
    want_g = ("n", "sum", "sumsq", "direct")
    keep = {}

    def timed(fn, reps):
        ms = []
        for rep in range(reps + 1):
            rt.synchronize(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = ms[1:]
        return res, dict(ms=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), reps=reps)

    def line(what, stats, **kw):
        print(json.dumps(dict(what=what, **stats, **kw)), flush=True)

    tex, st = timed(lambda: rt.bake_texels(tuv, w, h), a.reps)
    n = tex["ncovered"]
    print(json.dumps(dict(what="atlas", scene=a.scene, triangles=ntri, width=w, height=h, spp=spp, covered=n, rays=n * spp)), flush=True)
    line("bake_texels", st)
    g, st = timed(lambda: rt.gather(tex["points"], tex["normals"], tex["ids"], spp=spp, want=want_g), a.reps)
    line("gather", st, library_total_ms=round(rt.last_counts().total_ms, 3))
    _, st = timed(lambda: rt.bake_atlas(tex["ids"], g["direct"], w, h, 2), a.reps)
    line("bake_atlas", st)
    _, st = timed(lambda: rt.bake(tuv, w, h, spp=spp), a.reps)
    line("bake", st, hbm_bytes=rt.hbm_allocated_bytes())

    def torch_way():
        t = torch_texels(torch, tuv, tverts, tnormals, w, h)
        torch.cuda.synchronize()
        keep["torch_ms"] = time.perf_counter()
        return t, rt.gather(t["points"], t["normals"], t["ids"], spp=spp, want=want_g)

    def torch_only():
        return torch_texels(torch, tuv, tverts, tnormals, w, h)

    tt, st = timed(torch_only, a.reps)
    line("torch_device texels", st)
    (tt, tg), st = timed(torch_way, a.reps)
    line("torch_device texels + gather", st)

    def numpy_only():
        return bake.texels(uv, w, h, scene)

    nt, st = timed(numpy_only, a.host_reps)
    line("numpy_host texels", st)
    ng, st = timed(lambda: rt.gather(nt["points"], nt["normals"], nt["ids"], spp=spp, want=want_g), a.host_reps)
    line("numpy_host gather from host arrays", st)

    b = lambda x: np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.uint32)
    lib = {k: b(tex[k]) for k in ("owner", "bary", "ids", "points", "normals", "albedo")}
    eq_numpy = {k: bool(np.array_equal(lib[k], b(nt[k]))) for k in lib}
    towner = tt["owner"].cpu().numpy(); towner = np.where(towner == np.iinfo(np.int64).max, MISS, towner).astype(np.uint32)
    eq_torch = dict(owner=bool(np.array_equal(lib["owner"], towner)), ids=bool(np.array_equal(lib["ids"], b(tt["ids"]))))
    if eq_torch["ids"]:
        ids = tex["ids"].cpu().numpy().view(np.uint32)
        eq_torch["bary"] = bool(np.array_equal(lib["bary"].reshape(-1, 2)[ids], np.stack([b(tt["u"]), b(tt["v"])], axis=1)))
        eq_torch["points"] = bool(np.array_equal(lib["points"], b(tt["points"])))
        eq_torch["normals"] = bool(np.array_equal(lib["normals"], b(tt["normals"])))
        eq_torch["gather"] = all(bool(np.array_equal(b(g[k]), b(tg[k]))) for k in want_g)
    eq_numpy["gather"] = all(bool(np.array_equal(b(g[k]), b(ng[k]))) for k in want_g)
    print(json.dumps(dict(what="equal to the library on the bits", numpy_host=eq_numpy, torch_device=eq_torch)), flush=True)
    rt.close()
    if not all(eq_numpy.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
