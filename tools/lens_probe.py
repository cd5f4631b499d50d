#!/usr/bin/env python3
"""What a frame under a lens costs, on thai2 at 1920x1080 and 8 spp.

Four calls, timed in turn (--reps rounds after one warm-up round; every round starts from a cleared film, so the rays made once for a fresh film are the
frame's own):
  render_pinhole      mi355rt_render under LENS_PINHOLE: the frame as it always was (tile bins, culled chunks skipped)
  render_thin         mi355rt_render under THIN (0.1, 5): the rays made in registers by the lens instantiations, the primary round walking the tree
  render_rays_device  mi355rt_render_rays of the same rays from a torch tensor on the GPU (made by lens_rays): the same walk, plus 24 bytes read per ray
  lens_rays_device    mi355rt_lens_rays(8) into a torch tensor on the GPU (allocated once, outside the timing)
The films of render_thin and render_rays_device are checked to be equal.  One JSON line per call: wall-clock ms (median, min, max), the library's own
total_ms of the last round, the counters that differ and mi355rt_hbm_allocated_bytes after the call.
usage: tools/lens_probe.py [--width 1920 --height 1080] [--spp 8] [--reps 5]"""
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
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h, spp = a.width, a.height, a.spp
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1)
    thin = dict(model="thin", radius=0.1, focus=5.0)
    rt.set_lens(**thin)
    rays_t = rt.lens_rays(spp, device=True)                 # the rays of a fresh film
    rt.set_lens("pinhole")
    print(json.dumps(dict(what="rays", width=w, height=h, spp=spp, rays=int(rays_t.shape[0]), megabytes=round(rays_t.numel() * 4 / 1e6, 1))), flush=True)

    out_t = torch.empty_like(rays_t)
    torch.cuda.synchronize()

    def lens_rays_into():
        rt._check(pkg.lib().mi355rt_lens_rays(rt._h, spp, pkg.RAYS_DEVICE, out_t.data_ptr(), out_t.shape[0]))

    def under(lens, fn):
        rt.set_lens(**lens)
        try:
            return fn()
        finally:
            rt.set_lens("pinhole")

    entries = [("render_pinhole", lambda: rt.render(spp)),
               ("render_thin", lambda: under(thin, lambda: rt.render(spp))),
               ("render_rays_device", lambda: rt.render_rays(rays_t, spp)),
               ("lens_rays_device", lambda: under(thin, lens_rays_into))]
    wall = {k: [] for k, _ in entries}
    last, films, hbm = {}, {}, {}
    for rep in range(a.reps + 1):
        for name, fn in entries:
            rt.film.clear()
            rt.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            last[name] = c
            hbm[name] = rt.hbm_allocated_bytes()
            if rep == 0 and name.startswith("render"):
                films[name] = [x.copy() for x in rt.film.pixel_datas()]
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(films["render_thin"], films["render_rays_device"]))
    assert not np.array_equal(films["render_thin"][0].view(np.uint32), films["render_pinhole"][0].view(np.uint32))
    assert torch.equal(out_t.view(torch.int32), rays_t.view(torch.int32))          # (a cleared film each time: the same rays)
    for name, _ in entries:
        t, c = wall[name][1:], last[name]
        line = dict(what=name, ms=round(float(np.median(t)), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3), hbm_bytes=hbm[name])
        if name.startswith("render"):
            line.update(total_ms=round(c.total_ms, 3), primary=c.primary, primary_hits=c.primary_hits, primary_culled=c.primary_culled, trace_launches=c.trace_launches)
        print(json.dumps(line), flush=True)
    rt.close()


if __name__ == "__main__":
    main()
