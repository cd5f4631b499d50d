#!/usr/bin/env python3
"""What visibility-weighted probes cost and what they buy, on thai2: the grid of tools/probes_probe.py — 32 x 16 x 32 probes over the scene's
box at 256 spp (4.2 M rays) — looked up at the primary hit points of a 1920x1080 view with their face normals.

Timed in turn (--reps rounds after one warm-up round), everything on the device, each to the point where its results are complete:
  probes_gather               RayTracer.probes_gather (n, sh): the yardstick, the path without depth films
  probes_gather_depth_R<R>    RayTracer.probes_gather_depth (n, sh, count, moments) for every R of --res: the same traced pass plus the depth reduce
  probes_lookup               RayTracer.probes_lookup: the yardstick
  probes_lookup_vis_R<R>      RayTracer.probes_lookup_vis with both weights
One JSON line per measurement: wall-clock ms (median, min, max), and the library's own total for the gathers.  --label names the library build in every line
(MI355RT_LIB selects an A/B build of it).  Then, unless --timing-only and without pass or fail: the looked-up irradiance against gather's cosine-weighted
irradiance (--gather-spp) at the same surface points — unweighted, Chebyshev only, facing only and both, per R, with normal_bias 0 and a fifth of the smallest
spacing: RMS relative difference, mean, share of negative values, share of queries no probe could serve (ok = 0).
usage: tools/probes_vis_probe.py [--width 1920 --height 1080] [--counts 32,16,32] [--spp 256] [--res 8,16] [--gather-spp 64] [--reps 5] [--label NAME] [--timing-only]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--counts", default="32,16,32")
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--res", default="8,16")
    ap.add_argument("--gather-spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--timing-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/probes_vis_probe.py measures on the GPU and there is none")
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    cams = importlib.import_module("raytracer_rs_amd.cameras")
    ga = importlib.import_module("raytracer_rs_amd.gather")
    pr = importlib.import_module("raytracer_rs_amd.probes")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h, spp, seed = a.width, a.height, a.spp, 1
    counts = tuple(int(c) for c in a.counts.split(","))
    Rs = tuple(int(r) for r in a.res.split(","))
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=seed)
    verts = scene["tri_verts"].reshape(-1, 3)
    grid = pr.grid_over(verts.min(axis=0), verts.max(axis=0), counts)
    gp = pr.grid_points(grid)
    nprobes = gp.shape[0]
    D = pr.grid_max_distance(grid)
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
    torch.cuda.synchronize()
    say = lambda **kw: print(json.dumps(dict(kw, label=a.label)), flush=True)
    say(what="setup", counts=counts, probes=nprobes, spp=spp, rays=nprobes * spp, queries=int(qp.shape[0]), width=w, height=h, res=Rs, max_distance=D,
        spacing=[float(x) for x in grid["spacing"]])
    lib_ms = {}
    films = {}

    def gather():
        res = rt.probes_gather(tgp, None, spp=spp, want=("n", "sh"))            # returns when the library's stream is idle
        lib_ms.setdefault("probes_gather", []).append(rt.last_counts().total_ms)
        return res

    def gather_depth(R):
        def run():
            res = rt.probes_gather_depth(tgp, None, spp=spp, res=R, max_distance=D)
            lib_ms.setdefault("probes_gather_depth_R%d" % R, []).append(rt.last_counts().total_ms)
            return res
        return run

    def lookup():
        return rt.probes_lookup(grid, films[Rs[0]], tqp, tqn, "irradiance")

    def lookup_vis(R):
        return lambda: rt.probes_lookup_vis(grid, films[R], tqp, tqn, tqn, "irradiance")

    entries = [("probes_gather", gather)] + [("probes_gather_depth_R%d" % R, gather_depth(R)) for R in Rs]
    entries += [("probes_lookup", lookup)] + [("probes_lookup_vis_R%d" % R, lookup_vis(R)) for R in Rs]
    wall = {k: [] for k, _ in entries}
    plain = None
    for rep in range(a.reps + 1):
        for name, fn in entries:
            rt.synchronize()
            t0 = time.perf_counter()
            res = fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            if rep == 0:                                   # the warm-up round keeps what the later entries read
                if name == "probes_gather":
                    plain = res
                elif name.startswith("probes_gather_depth"):
                    films[res["depth_res"]] = res
    for name, _ in entries:
        t = wall[name][1:]
        line = dict(what=name, ms=round(float(np.median(t)), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3))
        if name in lib_ms:
            line.update(library_total_ms=round(float(np.median(lib_ms[name][1:])), 3))
        say(**line)
    u32 = lambda x: x.cpu().numpy().view(np.uint32)
    say(what="sh_equal_probes_gather", **{"R%d" % R: bool(all(np.array_equal(u32(films[R][k]), u32(plain[k])) for k in ("n", "sh"))) for R in Rs})
    for R in Rs:
        c = films[R]["count"].cpu().numpy().view(np.uint32)
        say(what="depth_film", R=R, samples_per_texel=round(float(c.mean()), 3), share_empty_texels=round(float((c == 0).mean()), 5), bytes=int(c.size * 12))
    say(what="hbm_bytes", hbm_bytes=rt.hbm_allocated_bytes())
    if a.timing_only:
        rt.close()
        return
    # the looked-up irradiance against gather's own cosine-weighted irradiance at the same surface points: figures, no verdict
    g = rt.gather(tqp, tqn, None, spp=a.gather_spp, weight="cosine", want=("n", "sum"))
    e_gather = ga.irradiance({k: x.cpu().numpy().view(np.uint32 if k == "n" else np.float32) for k, x in g.items()}).astype(np.float64)
    norm = np.sqrt((e_gather ** 2).mean())
    say(what="gather_irradiance", gather_spp=a.gather_spp, mean=round(float(e_gather.mean()), 5))

    def report(what, rgb, ok, **kw):
        e = rgb.cpu().numpy().astype(np.float64); k = ok.cpu().numpy() != 0
        served = float(np.sqrt(((e - e_gather)[k] ** 2).mean()) / np.sqrt((e_gather[k] ** 2).mean())) if k.any() else float("nan")
        say(what=what, rms_relative_difference=round(float(np.sqrt(((e - e_gather) ** 2).mean()) / norm), 4), rms_relative_difference_where_ok=round(served, 4),
            mean=round(float(e.mean()), 5), share_negative=round(float((e < 0).mean()), 5), share_not_ok=round(float((~k).mean()), 5), **kw)

    report("unweighted", *rt.probes_lookup(grid, plain, tqp, tqn, "irradiance", want_ok=True))
    for R in Rs:
        for bias in (0.0, 0.2 * float(grid["spacing"].min())):
            for cheb, facing in ((False, False), (True, False), (False, True), (True, True)):
                if not (cheb or facing):
                    continue                               # the unweighted lookup once more: without a weight the bias moves nothing
                rgb, ok = rt.probes_lookup_vis(grid, films[R], tqp, tqn, tqn, "irradiance", None, cheb, facing, bias, want_ok=True)
                report("weighted", rgb, ok, R=R, chebyshev=cheb, facing=facing, normal_bias=round(bias, 5))
    rt.close()


if __name__ == "__main__":
    main()
