#!/usr/bin/env python3
"""What probe placement costs and what it buys, on thai2, on the setup of tools/probes_vis_probe.py so that the tables read side by side: a
grid of 32 x 16 x 32 probes over the scene's box, films at 256 spp, looked up at the primary hit points of a 1920x1080 view with their face normals.  Everything
on the device.

Timed in turn within each round (--reps rounds after one warm-up round), wall-clock ms to the point where the results are complete on the device:
  probes_gather_64         RayTracer.probes_gather at 64 spp: the whole bounce tree of every sample
  probes_survey_64         RayTracer.probes_survey at 64 spp: the closest hits of the same samples
  probes_relocate_4        RayTracer.probes_relocate, four rounds at 64 spp: five surveys, four placements, the states
  probes_lookup_vis_R<R>   RayTracer.probes_lookup_vis on the unmoved grid's films
  probes_lookup_placed_R<R> RayTracer.probes_lookup_placed on the relocated grid's films with its offsets
Then, without pass or fail: the probes per state before and after, the verdicts of the last round, the back-hit share of the probes that see no geometry nearer
than min_front (thai2's winding has never been checked), and the RMS relative difference between the looked-up irradiance (both weights, normal_bias a fifth of
the smallest spacing) and gather's cosine-weighted irradiance (--gather-spp) at the surface points for three grids per R: unmoved; unmoved with usable_states;
relocated (films gathered at the moved points, lookup_placed, usable_states).  One JSON line per measurement.
usage: tools/probes_place_probe.py [--width 1920 --height 1080] [--counts 32,16,32] [--spp 256] [--res 8,16] [--gather-spp 64] [--reps 5] [--label tree]"""
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
    ap.add_argument("--res", default="8,16")
    ap.add_argument("--gather-spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="tree")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/probes_place_probe.py measures on the GPU and there is none")
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
    D, min_front = pr.grid_max_distance(grid), pr.grid_min_front(grid)
    bias = 0.2 * float(grid["spacing"].min())
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
    say(what="setup", counts=counts, probes=nprobes, spp=spp, survey_spp=a.survey_spp, rounds=a.rounds, queries=int(qp.shape[0]), width=w, height=h, res=Rs, max_distance=D,
        min_front=min_front, normal_bias=round(bias, 5), spacing=[float(x) for x in grid["spacing"]])
    # what the timed entries read: the relocated grid, and the films of both grids
    placed = rt.probes_relocate(grid, rounds=a.rounds, spp=a.survey_spp, device=dev)
    before = rt.probes_survey(tgp, None, spp=a.survey_spp, max_distance=D)
    state0 = rt.probes_place(grid, before, None, want=("state",))[0]
    films0 = {R: rt.probes_gather_depth(tgp, None, spp=spp, res=R, max_distance=D) for R in Rs}
    films1 = {R: rt.probes_gather_depth(placed["points"], None, spp=spp, res=R, max_distance=D) for R in Rs}
    lib_ms = {}

    def timed(name, fn):
        def run():
            res = fn()
            lib_ms.setdefault(name, []).append(rt.last_counts().total_ms)
            return res
        return run

    entries = [("probes_gather_%d" % a.survey_spp, timed("probes_gather_%d" % a.survey_spp, lambda: rt.probes_gather(tgp, None, spp=a.survey_spp, want=("n", "sh")))),
               ("probes_survey_%d" % a.survey_spp, timed("probes_survey_%d" % a.survey_spp, lambda: rt.probes_survey(tgp, None, spp=a.survey_spp, max_distance=D))),
               ("probes_relocate_%d" % a.rounds, lambda: rt.probes_relocate(grid, rounds=a.rounds, spp=a.survey_spp, device=dev))]
    for R in Rs:
        entries.append(("probes_lookup_vis_R%d" % R, lambda R=R: rt.probes_lookup_vis(grid, films0[R], tqp, tqn, tqn, "irradiance", None, True, True, bias)))
        entries.append(("probes_lookup_placed_R%d" % R, lambda R=R: rt.probes_lookup_placed(grid, films1[R], tqp, tqn, tqn, "irradiance", None, True, True, bias, placed["offsets"])))
    wall = {k: [] for k, _ in entries}
    for rep in range(a.reps + 1):
        for name, fn in entries:
            rt.synchronize()
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    for name, _ in entries:
        t = wall[name][1:]
        line = dict(what=name, ms=round(float(np.median(t)), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3))
        if name in lib_ms:
            line.update(library_total_ms=round(float(np.median(lib_ms[name][1:])), 3))
        say(**line)
    # states, verdicts, and what the back-hit share looks like where nothing is near
    host = lambda x: x.cpu().numpy()
    s0, s1, verdict = host(state0), host(placed["state"]), host(placed["verdict"])
    names = ("unknown", "buried", "idle", "active")
    say(what="states", before={names[k]: int((s0 == k).sum()) for k in range(4)}, after={names[k]: int((s1 == k).sum()) for k in range(4)})
    vnames = {0: "unsampled", 1: "through", 2: "away", 3: "stay", 4: "back", 5: "rest"}
    say(what="last_round_verdicts", accepted={vnames[k]: int((verdict == k).sum()) for k in vnames}, refused={vnames[k]: int((verdict == (k | 8)).sum()) for k in (1, 2, 4)})
    off = host(placed["offsets"])
    moved = (off != 0).any(axis=1)
    say(what="offsets", moved=int(moved.sum()), mean_length_in_spacings=round(float(np.linalg.norm(off[moved] / grid["spacing"], axis=1).mean()) if moved.any() else 0.0, 4))
    bn, bb = host(before["n"]).view(np.uint32).astype(np.float64), host(before["back"]).view(np.uint32).astype(np.float64)
    nf, nb = host(before["near_front"])[:, 0], host(before["near_back"])[:, 0]
    free = np.minimum(nf, nb) >= min_front
    share = bb / bn
    say(what="back_share_of_free_probes", probes=int(free.sum()), mean=round(float(share[free].mean()), 4), median=round(float(np.median(share[free])), 4),
        share_over_back_share=round(float((share[free] > 0.25).mean()), 4), share_zero=round(float((share[free] == 0).mean()), 4))
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

    use0, use1 = pr.usable_states(state0), placed["usable"]
    for R in Rs:
        report("unmoved", *rt.probes_lookup_vis(grid, films0[R], tqp, tqn, tqn, "irradiance", None, True, True, bias, want_ok=True), R=R)
        report("unmoved_usable_states", *rt.probes_lookup_vis(grid, films0[R], tqp, tqn, tqn, "irradiance", use0, True, True, bias, want_ok=True), R=R)
        report("relocated", *rt.probes_lookup_placed(grid, films1[R], tqp, tqn, tqn, "irradiance", use1, True, True, bias, placed["offsets"], want_ok=True), R=R)
    say(what="hbm_bytes", hbm_bytes=rt.hbm_allocated_bytes())
    rt.close()


if __name__ == "__main__":
    main()
