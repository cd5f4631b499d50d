#!/usr/bin/env python3
"""Adaptive sampling against uniform sampling on thai2 at 1920x1080: what the defaults of
mi355rt_adaptive_default_config rest on.

Prints one JSON line per measurement:
  reference   a 1024-spp uniform image (the "truth" every RMSE below is taken against; seed 99, independent of the others)
  uniform     64 spp: ms, RMSE
  adaptive    each config of the grid: ms, samples_added (per pixel), rounds, RMSE
  equal_time  uniform at the spp whose time equals the adaptive call's (from the measured ms per spp): RMSE
RMSE is over every pixel and channel of Film::get_pixels (mean radiance), timings are wall-clock medians of --reps calls after one
warm-up call (the film is cleared before each).
usage: tools/adaptive_probe.py [--width 1920 --height 1080] [--reps 3] [--grid default|sweep]"""
import argparse
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--grid", choices=["default", "sweep"], default="sweep")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    import importlib
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h = a.width, a.height
    npix = w * h

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    ref_rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=99)
    t0 = time.perf_counter()
    for _ in range(a.ref_spp // 64):
        ref_rt.render(64)
    ref = ref_rt.film.get_pixels().astype(np.float64)
    emit(what="reference", spp=a.ref_spp, s=round(time.perf_counter() - t0, 2))
    ref_rt.close()

    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1)

    def rmse():
        p = rt.film.get_pixels().astype(np.float64)
        return float(np.sqrt(np.mean((p - ref) ** 2)))

    def timed(fn):
        rt.film.clear(); fn(); rt.synchronize()                 # warm-up (pass buffers, bins)
        ts = []
        for _ in range(a.reps):
            rt.film.clear(); rt.synchronize()
            t = time.perf_counter(); out = fn(); ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts)), out

    ms64, _ = timed(lambda: rt.render(64))
    emit(what="uniform", spp=64, ms=round(ms64, 2), rmse=rmse())
    ms_per_spp = ms64 / 64.0
    grid = [dict()]
    if a.grid == "sweep":
        grid += [dict(rel_error=0.1), dict(rel_error=0.03), dict(batch_spp=16, min_spp=16), dict(abs_floor=0.05), dict(max_spp=128)]
    for kw in grid:
        cfg = pkg.adaptive_config(**kw)
        desc = {f: (round(getattr(cfg, f), 4) if isinstance(getattr(cfg, f), float) else getattr(cfg, f)) for f, _ in cfg._fields_}
        ms, st = timed(lambda: rt.render_adaptive(**kw))
        e = rmse()
        emit(what="adaptive", config=desc, ms=round(ms, 2), samples_added=st["samples_added"], spp_mean=round(st["samples_added"] / npix, 2),
             rounds=st["rounds"], rmse=e)
        spp_eq = max(1, int(round(ms / ms_per_spp)))
        rt.film.clear(); rt.render(spp_eq)
        emit(what="equal_time", config=desc, spp=spp_eq, rmse=rmse(), adaptive_rmse=e)


if __name__ == "__main__":
    main()
