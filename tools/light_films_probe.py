#!/usr/bin/env python3
"""Light films on thai2 at 1920x1080 x 64 spp: what MI355RT_FLAG_LIGHT_FILMS costs a render, what the relit read-out costs, and the memory.

Prints one JSON line per measurement (and writes it to --out), for 1, 2 and 4 lights (thai2's own, then the extra lights of
tests/test_gpu_parity.py::test_several_lights_on_multi_leaf_octrees):
  render   render(spp) of a handle without and with the flag on the same scene, alternating, film cleared before each, every call ended by a device
           synchronise: wall-clock ms, median (min - max) of --reps after one warm-up call each
  relit    get_relit_pixels at weight 1 without and with a display config (sRGB, ACES, auto-exposure): wall-clock ms including the copy to the host
  memory   mi355rt_hbm_allocated_bytes of both handles after the renders, and the planes' share
--trace N: only --reps renders each of a handle without and with the flag and N lights, for a run under a kernel trace (the resolve kernel's own time:
           profiles/README.md has the command line).
usage: tools/light_films_probe.py [--width 1920 --height 1080] [--spp 64] [--reps 5] [--trace N] [--out profiles/light_films_probe.jsonl]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXTRA = np.array([[-3.0, 4.0, -2.0, 2.0, 5.0, 8.0], [6.0, -2.5, 3.0, 4.0, 1.0, 0.5], [1.5, 6.0, 2.5, 3.0, 3.0, 1.0]], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0, help="number of lights of a trace run (0: the whole probe)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_films_probe.jsonl"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    base = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h, spp = a.width, a.height, a.spp

    def scene(nl):
        sc = dict(base)
        sc["lights"] = np.concatenate([base["lights"][:1], EXTRA])[:nl].astype(np.float32)
        return sc

    def handle(nl, on):
        # the pass buffers grow with the light count (a plane of light terms per node and light): from 4 lights on the frame runs as passes of 32 samples
        # per pixel, so that the two handles of a measurement fit on the device side by side (one handle alone would halve its passes by itself)
        kw = dict(samples_per_pass=32) if nl >= 4 else {}
        return pkg.create_raytracer_from_arrays(scene(nl), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1, flags=pkg.FLAG_LIGHT_FILMS if on else 0, **kw)

    def one_render(rt):
        rt.film.clear(); rt.synchronize()
        t = time.perf_counter(); rt.render(spp); rt.synchronize()
        return (time.perf_counter() - t) * 1e3

    if a.trace:
        for on in (False, True):
            rt = handle(a.trace, on)
            for _ in range(a.reps + 1):
                one_render(rt)
            rt.close()
        return

    log = open(a.out, "w")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        log.write(line + "\n"); log.flush()

    def stats(ts):
        return dict(median=round(float(np.median(ts)), 3), min=round(min(ts), 3), max=round(max(ts), 3))

    for nl in (1, 2, 4):
        off, on = handle(nl, False), handle(nl, True)
        one_render(off); one_render(on)                                   # warm-up: pass buffers, the cull caches
        t_off, t_on = [], []
        for _ in range(a.reps):
            t_off.append(one_render(off)); t_on.append(one_render(on))
        emit(what="render", lights=nl, width=w, height=h, spp=spp, reps=a.reps, off_ms=stats(t_off), on_ms=stats(t_on),
             added_ms=round(float(np.median(t_on) - np.median(t_off)), 3))
        emit(what="memory", lights=nl, off_bytes=off.hbm_allocated_bytes(), on_bytes=on.hbm_allocated_bytes(), planes_bytes=nl * w * h * 12)
        ones = np.ones(nl, np.float32)
        for name, cfg in (("none", {}), ("srgb_aces_auto", dict(transfer=1, curve=2, auto_exposure=1))):
            on.get_relit_pixels(ones, **cfg)                              # first use: the read-out's buffers
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter(); on.get_relit_pixels(ones, **cfg); ts.append((time.perf_counter() - t) * 1e3)
            emit(what="relit", lights=nl, display=name, ms=stats(ts))
        off.close(); on.close()
    log.close()


if __name__ == "__main__":
    main()
