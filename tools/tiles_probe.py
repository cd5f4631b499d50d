#!/usr/bin/env python3
"""render_tiles and refine under a thin lens on thai2 at 1920x1080: adaptive depth of field against uniform sampling — the case
§3c left unmeasured, a frame whose background is not free — and what a region of the frame costs against the whole.

Prints one JSON line per measurement (and writes it to --out):
  reference   a 1024-spp uniform image under the same lens (the "truth" every RMSE below is taken against; seed 99, independent of the others)
  uniform     64 spp under the lens: ms, RMSE
  refine      RayTracer.refine with the default config and with batches of 8: ms, samples_added (per pixel), rounds, RMSE
  equal_time  uniform at the spp whose time equals the refine call's (from the measured ms per spp): its own ms, RMSE
  region      a centred 256x256 region at 64 spp (render_tiles with adaptive.region_mask) against the whole frame: ms, share of the pixels, share of the time;
              region_pinhole: the same under the pinhole
RMSE is over every pixel and channel of Film::get_pixels (mean radiance); timings are wall-clock medians of --reps calls after one warm-up call (the
film is cleared before each; every call ends in a device synchronise).
usage: tools/tiles_probe.py [--width 1920 --height 1080] [--reps 3] [--out profiles/tiles_probe.jsonl]"""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiles_probe.jsonl"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    ad = importlib.import_module("raytracer_rs_amd.adaptive")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h = a.width, a.height
    npix = w * h
    lens = dict(model="thin", radius=0.1, focus=5.0)
    log = open(a.out, "w")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        log.write(line + "\n"); log.flush()

    ref_rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=99)
    ref_rt.set_lens(**lens)
    t0 = time.perf_counter()
    for _ in range(a.ref_spp // 64):
        ref_rt.render(64)
    ref = ref_rt.film.get_pixels().astype(np.float64)
    emit(what="reference", lens=lens, width=w, height=h, spp=a.ref_spp, s=round(time.perf_counter() - t0, 2))
    ref_rt.close()

    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1)
    rt.set_lens(**lens)

    def rmse():
        p = rt.film.get_pixels().astype(np.float64)
        return float(np.sqrt(np.mean((p - ref) ** 2)))

    def timed(fn):
        rt.film.clear(); fn(); rt.synchronize()                 # warm-up (pass buffers)
        ts = []
        for _ in range(a.reps):
            rt.film.clear(); rt.synchronize()
            t = time.perf_counter(); out = fn(); rt.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts)), out

    ms64, c64 = timed(lambda: rt.render(64))
    emit(what="uniform", spp=64, ms=round(ms64, 2), rmse=rmse(), primary_hits_share=round(c64.primary_hits / c64.primary, 4))
    ms_per_spp = ms64 / 64.0
    for kw in (dict(), dict(batch_spp=8, min_spp=8)):
        cfg = pkg.adaptive_config(**kw)
        desc = {f: (round(getattr(cfg, f), 4) if isinstance(getattr(cfg, f), float) else getattr(cfg, f)) for f, _ in cfg._fields_}
        ms, st = timed(lambda: rt.refine(**kw))
        e = rmse()
        emit(what="refine", config=desc, ms=round(ms, 2), samples_added=st["samples_added"], spp_mean=round(st["samples_added"] / npix, 2),
             rounds=st["rounds"], tiles_active_first=st["tiles_active_first"], tiles=st["tiles"], rmse=e)
        spp_eq = max(1, int(round(ms / ms_per_spp)))
        ms_eq, _ = timed(lambda: rt.render(spp_eq))
        emit(what="equal_time", config=desc, spp=spp_eq, ms=round(ms_eq, 2), rmse=rmse(), refine_ms=round(ms, 2), refine_rmse=e)
    x0, y0 = (w - 256) // 2, (h - 256) // 2
    mask = ad.region_mask(w, h, x0, y0, x0 + 256, y0 + 256)
    ms_r, c = timed(lambda: rt.render_tiles(mask, 64))
    emit(what="region", rect=[x0, y0, x0 + 256, y0 + 256], spp=64, tiles=int(mask.sum()), ms=round(ms_r, 2), frame_ms=round(ms64, 2),
         pixel_share=round(c.primary / 64 / npix, 4), time_share=round(ms_r / ms64, 4))
    rt.set_lens("pinhole")
    ms_p, _ = timed(lambda: rt.render(64))
    ms_rp, c = timed(lambda: rt.render_tiles(mask, 64))
    emit(what="region_pinhole", spp=64, ms=round(ms_rp, 2), frame_ms=round(ms_p, 2), pixel_share=round(c.primary / 64 / npix, 4), time_share=round(ms_rp / ms_p, 4))
    log.close()


if __name__ == "__main__":
    main()
