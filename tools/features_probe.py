#!/usr/bin/env python3
"""The feature film on thai2 at 1920x1080: what the pass costs against the render it guides, and whether its guides denoise better
than the centre-ray guides — under a thin lens (radius 0.1, focus 5), where the centre ray is pinhole-sharp and the film is not, and under the pinhole.

Prints one JSON line per measurement (and writes it to --out):
  cost       features.render(spp) against render(spp) on the same handle in the same call: ms of each (wall-clock medians of --reps calls after one warm-up
             call, film and feature film cleared before each, every call ends in a device synchronise) and their ratio, per lens
  reference  a --ref-spp film of another seed under the same lens (the "truth" of the RMSE below)
  quality    the spp film read out raw, denoised with centre guides and denoised with feature guides (spp feature samples), each also split (the handle keeps
             a direct film): tone-mapped RMSE, over every pixel and channel of c / (1 + c), per lens; coverage: the share of pixels with 0 < hits < n.
             Once more per count of --more-feature-spp (64): the same film under guides of more feature samples, which tells noise in the guides from
             what their averaging itself does to the filter
usage: tools/features_probe.py [--width 1920 --height 1080] [--spp 16] [--reps 3] [--ref-spp 1024] [--more-feature-spp 64] [--out profiles/features_probe.jsonl]"""
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
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--more-feature-spp", default="64", help="further feature sample counts for the quality table, comma-separated (the film stays at --spp)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_probe.jsonl"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h, spp = a.width, a.height, a.spp
    log = open(a.out, "w")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        log.write(line + "\n"); log.flush()

    def tm(x):
        x = x.astype(np.float64)
        return x / (1.0 + x)

    for lens in (dict(model="pinhole"), dict(model="thin", radius=0.1, focus=5.0)):
        rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1, flags=pkg.FLAG_DIRECT_FILM)
        rt.set_lens(**lens)

        def timed(fn):
            rt.film.clear(); rt.features.clear(); fn(); rt.synchronize()          # warm-up (pass buffers, the planes)
            ts = []
            for _ in range(a.reps):
                rt.film.clear(); rt.features.clear(); rt.synchronize()
                t = time.perf_counter(); fn(); rt.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
            return float(np.median(ts))

        ms_render = timed(lambda: rt.render(spp))
        ms_feat = timed(lambda: rt.features.render(spp))
        emit(what="cost", lens=lens, width=w, height=h, spp=spp, render_ms=round(ms_render, 2), features_ms=round(ms_feat, 2), ratio=round(ms_feat / ms_render, 3))

        ref_rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=99)
        ref_rt.set_lens(**lens)
        t0 = time.perf_counter()
        for _ in range(a.ref_spp // 64):
            ref_rt.render(64)
        ref = tm(ref_rt.film.get_pixels())
        ref_rt.close()
        emit(what="reference", lens=lens, spp=a.ref_spp, s=round(time.perf_counter() - t0, 2))

        def rmse(x):
            return float(np.sqrt(np.mean((tm(x) - ref) ** 2)))

        rt.film.clear()
        rt.render(spp)
        raw = rmse(rt.film.get_pixels())
        for fspp in [spp] + [int(x) for x in a.more_feature_spp.split(",") if x]:
            rt.features.clear()
            rt.features.render(fspp)
            f = rt.features.get()
            out = dict(raw=raw)
            for source in ("centre", "features"):
                rt.set_guide_source(source)
                out[source] = rmse(rt.get_denoised_pixels(packed=False)[0])
                out[source + "_split"] = rmse(rt.get_denoised_pixels(packed=False, split=True)[0])
            emit(what="quality", lens=lens, spp=spp, feature_spp=fspp, rmse={k: round(v, 6) for k, v in out.items()},
                 partial_pixel_share=round(float(((f["hits"] > 0) & (f["hits"] < f["n"])).mean()), 4), hit_pixel_share=round(float((f["hits"] > 0).mean()), 4))
        rt.close()
    log.close()


if __name__ == "__main__":
    main()
