#!/usr/bin/env python3
"""What a gather costs, on thai2 at 1920x1080 and 8 spp: the ray count DESIGN.md §3h measured.

The points are the primary hit points of the view's pixels (one jittered camera ray each) with the face normal turned against the ray; a pixel whose ray
misses gets a free-space point one unit along its ray with the reversed ray as its normal, so that every pixel is a point.  Three ways to the same per-point
n / sum / sumsq, timed in turn (--reps rounds after one warm-up round), and checked to be equal on the bits:
  gather_device   RayTracer.gather with points and normals on the device: rays made, traced and reduced by the library
  numpy_host      gather.rays in numpy, trace_rays from host arrays, gather.reduce in numpy
  torch_device    the same statement written in torch on the GPU (hash, table walk, rays, keys), trace_rays in place, the reduce in torch
Each way is timed to the point where its results are complete where it leaves them (the device for the two device ways, host arrays for numpy_host).
One JSON line per measurement: wall-clock ms (median, min, max), for the two hand-made ways the parts (median), for gather the library's own event time.
usage: tools/gather_probe.py [--width 1920 --height 1080] [--spp 8] [--reps 5]"""
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


def torch_rays(torch, table_t, seed, pts, nrm, first, spp):
    """gather.rays in torch on the device (ids None): (rays6, keys as int32 bits).  uint32 arithmetic in int64, masked; f32 operations one kernel each, unfused."""
    M = 0xFFFFFFFF
    n = pts.shape[0]
    dev = pts.device
    x = torch.arange(n, device=dev, dtype=torch.int64).repeat(spp)
    y = (first + torch.arange(spp, device=dev, dtype=torch.int64)).repeat_interleave(n) & M
    ids, sno = x.clone(), y.clone()
    z = torch.full_like(x, 0xFFFFFFFE)
    w = torch.full_like(x, seed & M)
    x, y, z, w = ((v * 1664525 + 1013904223) & M for v in (x, y, z, w))
    x = (x + y * w) & M; y = (y + z * x) & M; z = (z + x * y) & M; w = (w + y * z) & M
    x, y, z, w = (v ^ (v >> 16) for v in (x, y, z, w))
    x = (x + y * w) & M
    j = (x * 65535) >> 32
    nb = nrm.repeat(spp, 1)

    def rejected(idx, normals):
        t = table_t[idx]
        return (t[:, 0] * normals[:, 0] + t[:, 1] * normals[:, 1] + t[:, 2] * normals[:, 2]) <= 0

    act = torch.nonzero(rejected(j, nb))[:, 0]
    for _ in range(65535):
        if act.numel() == 0:
            break
        nj = (j[act] + 1) % 65535
        j[act] = nj
        act = act[rejected(nj, nb[act])]
    assert act.numel() == 0, "the probe's normals are unit normals: no void sample"
    d = table_t[j]
    rays = torch.cat([pts.repeat(spp, 1) + 0.00001 * d, d], dim=1).contiguous()
    keys = torch.stack([ids, sno], dim=1)
    keys = torch.where(keys >= 2**31, keys - 2**32, keys).to(torch.int32).contiguous()        # the uint32 bits in an int32 tensor
    return rays, keys


def torch_reduce(torch, rgb, n, spp):
    """gather.reduce for weight "mean" without void samples: per point, the samples in order"""
    rgb = rgb.reshape(spp, n, 3)
    s = torch.zeros((n, 3), dtype=torch.float32, device=rgb.device); q = torch.zeros_like(s)
    for k in range(spp):
        s = s + rgb[k]
        q = q + rgb[k] * rgb[k]
    return dict(n=torch.full((n,), spp, dtype=torch.int32, device=rgb.device), sum=s, sumsq=q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.is_available()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    cams = importlib.import_module("raytracer_rs_amd.cameras")
    ga = importlib.import_module("raytracer_rs_amd.gather")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h, spp, seed = a.width, a.height, a.spp, 1
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=seed)
    cam_rays = cams.pinhole(rt.camera.matrices(), w, h, 1, seed)
    tuv, prim = rt.intersect_rays(cam_rays)
    hit = prim != MISS
    o, d = cam_rays[:, :3], cam_rays[:, 3:]
    pts = np.where(hit[:, None], o + tuv[:, :1] * d, o + d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    v = scene["tri_verts"][np.where(hit, prim, 0)].astype(np.float64)
    nrm = np.cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
    nrm[~hit] = -d[~hit]
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[(nrm * d).sum(axis=1) > 0] *= -1
    pts, nrm = np.ascontiguousarray(pts), np.ascontiguousarray(nrm.astype(np.float32))
    n = pts.shape[0]
    dev = torch.device("cuda", 0)
    tp, tn = torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev)
    table = rt.sample_table()
    table_t = torch.from_numpy(table).to(dev)
    torch.cuda.synchronize()
    print(json.dumps(dict(what="points", width=w, height=h, spp=spp, points=n, on_a_surface=int(hit.sum()), rays=n * spp)), flush=True)
    want = ("n", "sum", "sumsq")
    parts = {"numpy_host": [], "torch_device": []}
    lib_ms, counts = [], []

    def gather_device():
        res = rt.gather(tp, tn, None, spp=spp, want=want)          # returns when the library's stream is idle
        counts.append(rt.last_counts())
        lib_ms.append(counts[-1].total_ms)
        return res

    def numpy_host():
        t0 = time.perf_counter()
        rays, keys, valid, wgt = ga.rays(table, seed, pts, nrm, None, 0, spp)
        t1 = time.perf_counter()
        got = rt.trace_rays(rays, keys, want=("rgb",))
        t2 = time.perf_counter()
        res = ga.reduce(got["rgb"], np.zeros(n * spp, np.float32), np.zeros(n * spp, bool), valid, wgt)
        t3 = time.perf_counter()
        parts["numpy_host"].append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        return res

    def torch_device():
        t0 = time.perf_counter()
        rays, keys = torch_rays(torch, table_t, seed, tp, tn, 0, spp)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got = rt.trace_rays(rays, keys, want=("rgb",))
        t2 = time.perf_counter()
        res = torch_reduce(torch, got["rgb"], n, spp)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        parts["torch_device"].append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        return res

    entries = [("gather_device", gather_device), ("numpy_host", numpy_host), ("torch_device", torch_device)]
    wall = {k: [] for k, _ in entries}
    results = {}
    for rep in range(a.reps + 1):
        for name, fn in entries:
            rt.synchronize()
            t0 = time.perf_counter()
            res = fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            if rep == 0:                                   # outside the timed region: the results to the host
                results[name] = {k: (res[k].cpu().numpy() if isinstance(res[k], torch.Tensor) else res[k]) for k in want}
    equal = all(np.array_equal(np.ascontiguousarray(results[name][k]).view(np.uint32), np.ascontiguousarray(results["gather_device"][k]).view(np.uint32))
                for name in ("numpy_host", "torch_device") for k in want)
    for name, _ in entries:
        t = wall[name][1:]
        line = dict(what=name, ms=round(float(np.median(t)), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3))
        if name in parts:
            p = np.median(np.array(parts[name][1:]), axis=0)
            line.update(rays_ms=round(float(p[0]), 3), trace_rays_ms=round(float(p[1]), 3), reduce_ms=round(float(p[2]), 3))
        else:
            line.update(library_total_ms=round(float(np.median(lib_ms[1:])), 3), each_ms=[round(x, 3) for x in t])
        print(json.dumps(line), flush=True)
    c = counts[-1]
    print(json.dumps(dict(what="counts of one gather", primary=c.primary, bounce=c.bounce, shadow=c.shadow, hbm_bytes=rt.hbm_allocated_bytes())), flush=True)
    print(json.dumps(dict(what="results_equal", equal=bool(equal))), flush=True)
    rt.close()
    if not equal:
        sys.exit(1)


if __name__ == "__main__":
    main()
