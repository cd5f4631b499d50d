#!/usr/bin/env python3
"""What a probe-lit frame costs and what it looks like against render(), on thai2, on the setup of tools/probes_vis_probe.py and
tools/probes_place_probe.py so that the tables read side by side: a grid of 32 x 16 x 32 probes over the scene's box, relocated, films at 256 spp with depth
films of 8 x 8 texels, a 1920x1080 view.  Everything on the device.

Timed in turn within each round (--reps rounds after one warm-up round), wall-clock ms to the point where the results are complete on the device:
  render_probe_lit_<s>     RayTracer.render_probe_lit at s = 1 and 4 spp: lens_rays, probe_lit_rays, frame_mean
  probe_lit_rays_<s>       its probe_lit_rays part alone, on the same rays
  trace_rays_<s>           RayTracer.trace_rays on the same rays: the whole bounce tree
  render_<s>               RayTracer.render(s) on a cleared film
  probe_lit_points         RayTracer.probe_lit_points at the view's hit points with their triangle normals
  probes_lookup_placed     RayTracer.probes_lookup_placed(mode="irradiance") at the same points
Then, without pass or fail: the RMSE against a --ref-spp render of the probe-lit 4-spp mean, of render at 4 spp and of render at 4 spp denoised; and `indirect`
against gather(weight="mean", spp=--gather-spp) at the same hit points, by ok share and RMSE.  One JSON line per measurement.
usage: tools/probe_lit_probe.py [--width 1920 --height 1080] [--counts 32,16,32] [--spp 256] [--res 8] [--ref-spp 256] [--gather-spp 64] [--reps 5] [--label tree]"""
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
    ap.add_argument("--survey-spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--res", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--gather-spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="tree")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/probe_lit_probe.py measures on the GPU and there is none")
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    ga = importlib.import_module("raytracer_rs_amd.gather")
    pr = importlib.import_module("raytracer_rs_amd.probes")
    plit = importlib.import_module("raytracer_rs_amd.probe_lit")
    ft = importlib.import_module("raytracer_rs_amd.features")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h, seed = a.width, a.height, 1
    npix = w * h
    counts = tuple(int(c) for c in a.counts.split(","))
    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=seed)
    verts = scene["tri_verts"].reshape(-1, 3)
    grid = pr.grid_over(verts.min(axis=0), verts.max(axis=0), counts)
    D = pr.grid_max_distance(grid)
    bias = 0.2 * float(grid["spacing"].min())
    dev = torch.device("cuda", 0)
    say = lambda **kw: print(json.dumps(dict(kw, label=a.label)), flush=True)
    # the volume: relocated, then gathered at the moved points
    placed = rt.probes_relocate(grid, rounds=a.rounds, spp=a.survey_spp, device=dev)
    films = rt.probes_gather_depth(placed["points"], None, spp=a.spp, res=a.res, max_distance=D)
    vol = plit.volume(grid, films, depth=films, offsets=placed, normal_bias=bias)
    say(what="setup", counts=counts, probes=int(placed["points"].shape[0]), spp=a.spp, res=a.res, rounds=a.rounds, width=w, height=h, max_distance=D, normal_bias=round(bias, 5),
        usable=int(placed["usable"].sum().item()), lights=int(len(scene["lights"])))
    rays = {s: rt.lens_rays(s, device=dev) for s in (1, 4)}
    # the view's hit points with their triangle normals (not flipped: the statement's N)
    tr = rt.trace_rays(rays[1], want=("tuv", "prim"))
    prim = tr["prim"].cpu().numpy().view(np.uint32); tuv = tr["tuv"].cpu().numpy()
    hit = prim != MISS
    r1 = rays[1].cpu().numpy()
    qp = np.ascontiguousarray(plit.hit_points(r1[hit], tuv[hit]))
    qn = np.ascontiguousarray(ft.tri_normals(scene)[prim[hit].astype(np.int64)])
    tqp, tqn = torch.from_numpy(qp).to(dev), torch.from_numpy(qn).to(dev)
    torch.cuda.synchronize()
    say(what="view", pixels=npix, hits=int(hit.sum()))

    def render(s):
        rt.film.clear()
        rt.render(s)

    entries = []
    for s in (1, 4):
        entries += [("render_probe_lit_%d" % s, lambda s=s: rt.render_probe_lit(vol, spp=s, device=dev)),
                    ("probe_lit_rays_%d" % s, lambda s=s: rt.probe_lit_rays(vol, rays[s], want=("rgb",))),
                    ("trace_rays_%d" % s, lambda s=s: rt.trace_rays(rays[s], want=("rgb",))),
                    ("render_%d" % s, lambda s=s: render(s))]
    entries += [("probe_lit_points", lambda: rt.probe_lit_points(vol, tqp, tqn)),
                ("probes_lookup_placed", lambda: rt.probes_lookup_placed(grid, films, tqp, tqn, tqn, "irradiance", placed["usable"], True, True, bias, placed["offsets"]))]
    wall = {k: [] for k, _ in entries}
    for rep in range(a.reps + 1):
        for name, fn in entries:
            rt.synchronize(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    for name, _ in entries:
        t = wall[name][1:]
        say(what=name, ms=round(float(np.median(t)), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3))
    # the images: figures, no verdict
    rmse = lambda x, ref: float(np.sqrt(((x.astype(np.float64) - ref) ** 2).mean()))
    render(a.ref_spp)
    ref = rt.film.get_pixels().astype(np.float64)
    lit = rt.render_probe_lit(vol, spp=4, device=dev)
    mean = lit["mean"].cpu().numpy().reshape(-1, 3)
    render(4)
    raw = rt.film.get_pixels()
    den = rt.get_denoised_pixels(rgb=True, packed=False)[0]
    say(what="rmse_against_render", ref_spp=a.ref_spp, probe_lit_4=round(rmse(mean, ref), 5), render_4=round(rmse(raw, ref), 5), render_4_denoised=round(rmse(den, ref), 5),
        mean_ref=round(float(ref.mean()), 5), mean_probe_lit=round(float(mean.mean()), 5), mean_render_4=round(float(raw.mean()), 5),
        ok_share_of_hits=round(float(lit["ok_share"].sum().item() / max(int(hit.sum()), 1)), 4))
    # indirect against gather's uniform hemisphere mean at the same points
    g = rt.gather(tqp, tqn, None, spp=a.gather_spp, weight="mean", want=("n", "sum"))
    gm = ga.mean({k: x.cpu().numpy().view(np.uint32 if k == "n" else np.float32) for k, x in g.items()}).astype(np.float64)
    ind, ok = rt.probe_lit_points(vol, tqp, tqn, want_ok=True)
    ind, ok = ind.cpu().numpy().astype(np.float64), ok.cpu().numpy() != 0
    raw_ind = rt.probe_lit_points(vol, tqp, tqn, clamp=False).cpu().numpy()
    fin = np.isfinite(gm).all(axis=1)
    say(what="indirect_against_gather_mean", gather_spp=a.gather_spp, ok_share=round(float(ok.mean()), 5), rmse=round(rmse(ind[fin], gm[fin]), 5),
        rmse_where_ok=round(rmse(ind[fin & ok], gm[fin & ok]), 5) if (fin & ok).any() else None, mean_gather=round(float(gm[fin].mean()), 5),
        mean_indirect=round(float(ind.mean()), 5), share_clamped=round(float((raw_ind < 0).any(axis=1).mean()), 5))
    say(what="hbm_bytes", hbm_bytes=rt.hbm_allocated_bytes())
    rt.close()


if __name__ == "__main__":
    main()
