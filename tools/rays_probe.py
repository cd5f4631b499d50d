#!/usr/bin/env python3
"""What a ray-fed frame costs, on thai2 at 1920x1080 and 8 spp.

Three ways to the same film, timed in turn (--reps rounds after one warm-up round; every round starts from a cleared film, so the rays of
cameras.pinhole — made once, for a fresh film — are the frame's own and all three films are equal, which is checked):
  render              mi355rt_render: camera rays made on the device, primaries through the tile bins, culled chunks skipped
  render_rays_device  mi355rt_render_rays from a torch tensor on the GPU: the same samples, the primary round walking the tree, nothing culled
  render_rays_host    mi355rt_render_rays from a numpy array: the same plus the upload of 24 bytes per ray
device - render is the price of tree-walking, unculled primaries; host - device is the upload.  One JSON line per measurement: wall-clock ms
(median, min, max), the library's own total_ms and trace_ms of the last round, and the counters that differ.  trace_rays of the same rays (rgb only)
is timed as a fourth line.
usage: tools/rays_probe.py [--width 1920 --height 1080] [--spp 8] [--reps 5]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h, spp = a.width, a.height, a.spp
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1)
    t0 = time.perf_counter()
    rays = cams.pinhole(rt.camera.matrices(), w, h, spp, 1)
    gen_ms = (time.perf_counter() - t0) * 1e3
    rays_t = torch.from_numpy(rays).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    print(json.dumps(dict(what="rays", width=w, height=h, spp=spp, rays=int(rays.shape[0]), megabytes=round(rays.nbytes / 1e6, 1), numpy_pinhole_ms=round(gen_ms, 1))), flush=True)
    entries = [("render", lambda: rt.render(spp)), ("render_rays_device", lambda: rt.render_rays(rays_t, spp)), ("render_rays_host", lambda: rt.render_rays(rays, spp))]
    wall = {k: [] for k, _ in entries}
    last, films = {}, {}
    for rep in range(a.reps + 1):
        for name, fn in entries:
            rt.film.clear()
            rt.synchronize()
            t0 = time.perf_counter()
            c = fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            last[name] = c
            if rep == 0:
                films[name] = [x.copy() for x in rt.film.pixel_datas()]
    for name in ("render_rays_device", "render_rays_host"):
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(films[name], films["render"])), name
    for name, _ in entries:
        t, c = wall[name][1:], last[name]
        print(json.dumps(dict(what=name, ms=round(float(np.median(t)), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3), total_ms=round(c.total_ms, 3),
                              primary=c.primary, primary_hits=c.primary_hits, primary_culled=c.primary_culled, trace_launches=c.trace_launches,
                              hbm_bytes=rt.hbm_allocated_bytes())), flush=True)
    ts = []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        rt.trace_rays(rays_t, None, want=("rgb",))
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(what="trace_rays_device, rgb", ms=round(float(np.median(ts[1:])), 3), ms_min=round(min(ts[1:]), 3), ms_max=round(max(ts[1:]), 3),
                          total_ms=round(rt.last_counts().total_ms, 3))), flush=True)
    rt.close()


if __name__ == "__main__":
    main()
