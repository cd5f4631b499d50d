#!/usr/bin/env python3
"""What a probe grid costs, on thai2: a grid of 32 x 16 x 32 probes over the scene's box at 256 spp (4.2 M rays), looked up at the primary hit
points of a 1920x1080 view with their face normals (tools/gather_probe.py makes the same points).

Two ways to the grid's n / sh, and two ways to the looked-up irradiance, timed in turn (--reps rounds after one warm-up round) and compared on the bits:
  probes_gather_device   RayTracer.probes_gather with the probe positions on the device: rays made, traced and projected by the library
  torch_gather_device    the same statement written in torch on the GPU (hash, table entry, rays, keys), trace_rays in place, the projection in torch
  probes_lookup_device   RayTracer.probes_lookup with everything on the device
  torch_lookup_device    probes.lookup written in torch on the GPU
Each way is timed to the point where its results are complete on the device.  One JSON line per measurement: wall-clock ms (median, min, max).  Last, without
pass or fail: the RMS relative difference between the looked-up irradiance and gather's cosine-weighted irradiance (--gather-spp) at the surface points.
usage: tools/probes_probe.py [--width 1920 --height 1080] [--counts 32,16,32] [--spp 256] [--gather-spp 64] [--reps 5]"""
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


def torch_sphere_rays(torch, table_t, seed, pts, first, spp):
    """gather.rays(normals=None, ids=None) in torch on the device: (rays6, keys as int32 bits).  uint32 arithmetic in int64, masked; f32 operations unfused."""
    M = 0xFFFFFFFF
    n, dev = pts.shape[0], pts.device
    x = torch.arange(n, device=dev, dtype=torch.int64).repeat(spp)
    y = (first + torch.arange(spp, device=dev, dtype=torch.int64)).repeat_interleave(n) & M
    ids, sno = x.clone(), y.clone()
    z = torch.full_like(x, 0xFFFFFFFE)
    w = torch.full_like(x, seed & M)
    x, y, z, w = ((v * 1664525 + 1013904223) & M for v in (x, y, z, w))
    x = (x + y * w) & M; y = (y + z * x) & M; z = (z + x * y) & M; w = (w + y * z) & M
    x, y, z, w = (v ^ (v >> 16) for v in (x, y, z, w))
    x = (x + y * w) & M
    d = table_t[(x * 65535) >> 32]
    rays = torch.cat([pts.repeat(spp, 1) + 0.00001 * d, d], dim=1).contiguous()
    keys = torch.stack([ids, sno], dim=1)
    keys = torch.where(keys >= 2**31, keys - 2**32, keys).to(torch.int32).contiguous()        # the uint32 bits in an int32 tensor
    return rays, keys


def torch_basis(torch, pr, d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c4 = (float(v) for v in (pr.C0, pr.C1, pr.C2, pr.C3, pr.C4))
    return torch.stack([torch.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (3.0 * (z * z) - 1.0), c2 * (x * z), c4 * (x * x - y * y)], dim=1)


def torch_project(torch, pr, rgb, dirs, n, spp):
    """probes.project in torch: per point, the samples in order"""
    rgb, dirs = rgb.reshape(spp, n, 3), dirs.reshape(spp, n, 3)
    sh = torch.zeros((n, 9, 3), dtype=torch.float32, device=rgb.device)
    for s in range(spp):
        sh = sh + torch_basis(torch, pr, dirs[s])[:, :, None] * rgb[s][:, None, :]
    return dict(n=torch.full((n,), spp, dtype=torch.int32, device=rgb.device), sh=sh)


def torch_lookup(torch, pr, g, res, pts, dirs, mode):
    """probes.lookup in torch on the device (no usable mask): (rgb, ok)"""
    dev, m = pts.device, pts.shape[0]
    counts = [int(c) for c in g["counts"]]
    n, sh = res["n"], res["sh"].reshape(-1, 27)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    i, f = [], []
    for a in range(3):
        # the divisor as a tensor: torch turns a division by a Python scalar into a multiplication by its reciprocal, which rounds differently
        gq = (pts[:, a] - float(g["origin"][a])) / torch.full((), float(g["spacing"][a]), dtype=torch.float32, device=dev)
        gq = torch.where(gq >= 0.0, gq, zero)
        top = torch.full((), float(np.float32(counts[a] - 1)), dtype=torch.float32, device=dev)
        gq = torch.where(gq <= top, gq, top)
        ia = gq.to(torch.int64)
        if counts[a] >= 2:
            ia = torch.clamp(ia, max=counts[a] - 2)
        fa = gq - ia.to(torch.float32)
        if counts[a] == 1:
            ia, fa = torch.zeros_like(ia), torch.zeros_like(fa)
        i.append(ia); f.append(fa)
    C = torch.zeros((m, 27), dtype=torch.float32, device=dev); wsum = torch.zeros(m, dtype=torch.float32, device=dev); ok = torch.zeros(m, dtype=torch.bool, device=dev)
    for j in range(8):
        c, w = [], []
        for a in range(3):
            up = (j >> a) & 1
            c.append(torch.clamp(i[a] + 1, max=counts[a] - 1) if up else i[a])
            w.append(f[a] if up else 1.0 - f[a])
        t = (w[0] * w[1]) * w[2]
        probe = (c[2] * counts[1] + c[1]) * counts[0] + c[0]
        nj = n[probe]
        used = (t != 0.0) & (nj != 0)
        s = t * (float(pr.SPHERE) / nj.to(torch.float32))
        wsum = torch.where(used, wsum + t, wsum)
        C = torch.where(used[:, None], C + s[:, None] * sh[probe], C)
        ok = ok | used
    b = torch_basis(torch, pr, dirs)
    r = torch.zeros((m, 3), dtype=torch.float32, device=dev)
    for k in range(9):
        ck = C[:, 3 * k:3 * k + 3]
        r = r + ((float(pr.A[k]) * ck) if mode == "irradiance" else ck) * b[:, k, None]
    return torch.where(ok[:, None], r / wsum[:, None], zero), ok.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--counts", default="32,16,32")
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--gather-spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.is_available()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    cams = importlib.import_module("raytracer_rs_amd.cameras")
    ga = importlib.import_module("raytracer_rs_amd.gather")
    pr = importlib.import_module("raytracer_rs_amd.probes")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h, spp, seed = a.width, a.height, a.spp, 1
    counts = tuple(int(c) for c in a.counts.split(","))
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=seed)
    verts = scene["tri_verts"].reshape(-1, 3)
    grid = pr.grid_over(verts.min(axis=0), verts.max(axis=0), counts)
    gp = pr.grid_points(grid)
    nprobes = gp.shape[0]
    # the queries: the primary hit points of the view, with the face normal turned against the ray (tools/gather_probe.py)
    cam_rays = cams.pinhole(rt.camera.matrices(), w, h, 1, seed)
    tuv, prim = rt.intersect_rays(cam_rays)
    hit = prim != MISS
    o, d = cam_rays[hit, :3], cam_rays[hit, 3:]
    qp = np.ascontiguousarray((o + tuv[hit, :1] * d).astype(np.float32))
    v = scene["tri_verts"][prim[hit]].astype(np.float64)
    qn = np.cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
    qn /= np.linalg.norm(qn, axis=1)[:, None]
    qn[(qn * d).sum(axis=1) > 0] *= -1
    qn = np.ascontiguousarray(qn.astype(np.float32))
    dev = torch.device("cuda", 0)
    tgp, tqp, tqn = torch.from_numpy(gp).to(dev), torch.from_numpy(qp).to(dev), torch.from_numpy(qn).to(dev)
    table_t = torch.from_numpy(rt.sample_table()).to(dev)
    torch.cuda.synchronize()
    print(json.dumps(dict(what="setup", counts=counts, probes=nprobes, spp=spp, rays=nprobes * spp, queries=int(qp.shape[0]), width=w, height=h,
                          origin=[float(x) for x in grid["origin"]], spacing=[float(x) for x in grid["spacing"]])), flush=True)
    parts, lib_ms = [], []
    state = {}

    def probes_gather_device():
        res = rt.probes_gather(tgp, None, spp=spp, want=("n", "sh"))          # returns when the library's stream is idle
        lib_ms.append(rt.last_counts().total_ms)
        return res

    def torch_gather_device():
        t0 = time.perf_counter()
        rays, keys = torch_sphere_rays(torch, table_t, seed, tgp, 0, spp)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got = rt.trace_rays(rays, keys, want=("rgb",))
        t2 = time.perf_counter()
        res = torch_project(torch, pr, got["rgb"], rays[:, 3:], nprobes, spp)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        return res

    def probes_lookup_device():
        return dict(rgb=rt.probes_lookup(grid, state["res"], tqp, tqn, "irradiance"))

    def torch_lookup_device():
        rgb, ok = torch_lookup(torch, pr, grid, state["res"], tqp, tqn, "irradiance")
        torch.cuda.synchronize()
        return dict(rgb=rgb)

    state["res"] = probes_gather_device()
    lib_ms.clear()
    entries = [("probes_gather_device", probes_gather_device), ("torch_gather_device", torch_gather_device), ("probes_lookup_device", probes_lookup_device),
               ("torch_lookup_device", torch_lookup_device)]
    wall = {k: [] for k, _ in entries}
    results = {}
    for rep in range(a.reps + 1):
        for name, fn in entries:
            rt.synchronize()
            t0 = time.perf_counter()
            res = fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            if rep == 0:                                   # outside the timed region: the results to the host
                results[name] = {k: res[k].cpu().numpy() for k in res}
    u32 = lambda x: np.ascontiguousarray(x).view(np.uint32)
    gather_equal = all(np.array_equal(u32(results["torch_gather_device"][k]), u32(results["probes_gather_device"][k])) for k in ("n", "sh"))
    lookup_equal = np.array_equal(u32(results["torch_lookup_device"]["rgb"]), u32(results["probes_lookup_device"]["rgb"]))
    differing = int((u32(results["torch_lookup_device"]["rgb"]) != u32(results["probes_lookup_device"]["rgb"])).sum())
    for name, _ in entries:
        t = wall[name][1:]
        line = dict(what=name, ms=round(float(np.median(t)), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3))
        if name == "torch_gather_device":
            p = np.median(np.array(parts[1:]), axis=0)
            line.update(rays_ms=round(float(p[0]), 3), trace_rays_ms=round(float(p[1]), 3), project_ms=round(float(p[2]), 3))
        if name == "probes_gather_device":
            line.update(library_total_ms=round(float(np.median(lib_ms[1:])), 3))
        print(json.dumps(line), flush=True)
    print(json.dumps(dict(what="results_equal", gather=bool(gather_equal), lookup=bool(lookup_equal), lookup_words_differing=differing)), flush=True)
    # the looked-up irradiance against gather's own cosine-weighted irradiance at the same surface points: a figure, no verdict
    e_probe = results["probes_lookup_device"]["rgb"].astype(np.float64)
    g = rt.gather(tqp, tqn, None, spp=a.gather_spp, weight="cosine", want=("n", "sum"))
    e_gather = ga.irradiance({k: x.cpu().numpy().view(np.uint32 if k == "n" else np.float32) for k, x in g.items()}).astype(np.float64)
    rms = float(np.sqrt(((e_probe - e_gather) ** 2).mean()) / np.sqrt((e_gather ** 2).mean()))
    print(json.dumps(dict(what="irradiance_vs_gather", gather_spp=a.gather_spp, rms_relative_difference=round(rms, 4), mean_probe=round(float(e_probe.mean()), 5),
                          mean_gather=round(float(e_gather.mean()), 5), share_negative_probe=round(float((e_probe < 0).mean()), 5))), flush=True)
    print(json.dumps(dict(what="hbm_bytes", hbm_bytes=rt.hbm_allocated_bytes())), flush=True)
    rt.close()
    if not (gather_equal and lookup_equal):
        sys.exit(1)


if __name__ == "__main__":
    main()
