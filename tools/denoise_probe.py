#!/usr/bin/env python3
"""The denoised read-out against plain sampling on thai2 at 1920x1080: what the defaults of mi355rt_denoise_default_config
rest on, and what the read-out costs.

Prints one JSON line per measurement:
  reference   a 1024-spp uniform image (the "truth" every RMSE below is taken against; seed 99, independent of the others)
  spp         for spp in 1, 4, 8, 16, 32, 64: render ms, denoise ms (guides cold: right after a camera change; cached), and the RMSE of the
              raw and of the denoised image, on the means (Film::get_pixels) and on the tone-mapped values c / (1 + c)
  equal_time  uniform sampling at the spp whose render time equals render + denoise of each row above (from the measured ms per spp)
  sweep       one field of the default config varied at a time, at 8 and 16 spp: RMSE of the denoised image; `best` lines name the winner
  dropin      the drop-in loop at 1024x768 (trace_frame_additive + a read-out per step): ms per step with get_tonemapped_pixels and with
              the denoised read-out (which settles the speculative next frame every step)
  --split      a second handle of the same seed created with FLAG_DIRECT_FILM renders the same films; every `spp` line gains
              render_ms_direct_film (against render_ms: what keeping the direct film costs), split_ms_cached (the split read-out, guides
              cached) and rmse_split / rmse_tm_split beside the raw and denoised columns, and the drop-in loop runs once more on a handle
              with the flag (`dropin_direct_film` lines: get_tonemapped_pixels and the split read-out)
Timings are wall-clock medians of --reps calls after one warm-up call.
usage: tools/denoise_probe.py [--width 1920 --height 1080] [--reps 5] [--ref-spp 1024] [--skip-sweep] [--skip-dropin] [--split]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--skip-dropin", action="store_true")
    ap.add_argument("--split", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    import importlib
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h = a.width, a.height

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    ref_rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=99)
    t0 = time.perf_counter()
    for _ in range(a.ref_spp // 64):
        ref_rt.render(64)
    ref = ref_rt.film.get_pixels().astype(np.float64)
    ref_tm = ref / (1.0 + ref)
    emit(what="reference", spp=a.ref_spp, s=round(time.perf_counter() - t0, 2))
    ref_rt.close()

    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1)
    rs = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1, flags=pkg.FLAG_DIRECT_FILM) if a.split else None

    def errors(p):
        p = np.asarray(p, np.float64)
        return float(np.sqrt(np.mean((p - ref) ** 2))), float(np.sqrt(np.mean((p / (1.0 + p) - ref_tm) ** 2)))

    def median_ms(fn, before=None):
        ts = []
        for i in range(a.reps + 1):
            if before:
                before(i)
            t = time.perf_counter(); fn(); dt = (time.perf_counter() - t) * 1e3
            if i:
                ts.append(dt)
        return float(np.median(ts))

    def render_ms(spp, rt=rt):
        def before(_):
            rt.film.clear(); rt.synchronize()
        return median_ms(lambda: rt.render(spp), before)

    eps = [1e-4]

    def nudge(_):                    # a camera change: the next read-out rebuilds the guides
        rt.camera.move_rel(0.0, 0.0, eps[0]); eps[0] = -eps[0]

    rows = []
    for spp in (1, 4, 8, 16, 32, 64):
        ms_r = render_ms(spp)                      # leaves a film of spp samples
        raw = errors(rt.film.get_pixels())
        rt.get_denoised_pixels(rgb=False)
        ms_cached = median_ms(lambda: rt.get_denoised_pixels(rgb=False))
        ms_cold = median_ms(lambda: rt.get_denoised_pixels(rgb=False), nudge)
        if eps[0] < 0:
            nudge(0)                               # back where the film was rendered
        den_rgb, _ = rt.get_denoised_pixels(packed=False)
        den = errors(den_rgb)
        row = dict(what="spp", spp=spp, render_ms=round(ms_r, 3), denoise_ms_cached=round(ms_cached, 3), denoise_ms_cold=round(ms_cold, 3),
                   rmse_raw=raw[0], rmse_denoised=den[0], rmse_tm_raw=raw[1], rmse_tm_denoised=den[1])
        if rs is not None:
            ms_rs = render_ms(spp, rs)             # the same film, and the direct film beside it
            rs.get_denoised_pixels(split=True, rgb=False)
            ms_split = median_ms(lambda: rs.get_denoised_pixels(split=True, rgb=False))
            spl = errors(rs.get_denoised_pixels(split=True, packed=False)[0])
            row.update(render_ms_direct_film=round(ms_rs, 3), split_ms_cached=round(ms_split, 3), rmse_split=spl[0], rmse_tm_split=spl[1])
        rows.append(row)
        emit(**row)
    ms_per_spp = rows[-1]["render_ms"] / 64.0
    for row in rows:
        spp_eq = max(1, int(round((row["render_ms"] + row["denoise_ms_cached"]) / ms_per_spp)))
        rt.film.clear(); rt.render(spp_eq)
        e = errors(rt.film.get_pixels())
        emit(what="equal_time", spp=row["spp"], ms=round(row["render_ms"] + row["denoise_ms_cached"], 3), uniform_spp=spp_eq,
             rmse_uniform=e[0], rmse_tm_uniform=e[1], rmse_denoised=row["rmse_denoised"], rmse_tm_denoised=row["rmse_tm_denoised"])

    if not a.skip_sweep:
        grid = dict(iterations=[3, 4, 5, 6, 7], normal_power_log2=[1, 3, 5, 7, 9], sigma_luminance=[1.0, 2.0, 4.0, 8.0, 16.0],
                    sigma_depth=[0.02, 0.05, 0.1, 0.3, 1.0], sigma_albedo=[0.02, 0.05, 0.1, 0.3, 1.0])
        for spp in (8, 16):
            rt.film.clear(); rt.render(spp)
            for field, values in grid.items():
                res = []
                for v in values:
                    den_rgb, _ = rt.get_denoised_pixels(packed=False, **{field: v})
                    e = errors(den_rgb)
                    res.append((e[1], v))
                    emit(what="sweep", spp=spp, field=field, value=v, rmse_denoised=e[0], rmse_tm_denoised=e[1])
                emit(what="best", spp=spp, field=field, value=min(res)[1], rmse_tm_denoised=min(res)[0])
    rt.close()
    if rs is not None:
        rs.close()

    if not a.skip_dropin:
        out = np.empty(1024 * 768, np.uint32)
        handles = [("", 0)] + ([("_direct_film", pkg.FLAG_DIRECT_FILM)] if a.split else [])      # --split: the same loop on a handle with the flag
        for suffix, flags in handles:
            d = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, 1024, 768, seed=1, flags=flags)
            reads = [("tonemapped", lambda: d.get_tonemapped_pixels(out)), ("denoised", lambda: d.get_denoised_pixels(rgb=False))]
            if flags:
                reads[1] = ("split", lambda: d.get_denoised_pixels(split=True, rgb=False))
            for label, read in reads + reads:
                for _ in range(20):
                    d.trace_frame_additive(); read()
                steps = 200
                t = time.perf_counter()
                for _ in range(steps):
                    d.trace_frame_additive(); read()
                d.synchronize()
                emit(what="dropin" + suffix, readout=label, ms_per_step=round((time.perf_counter() - t) * 1e3 / steps, 4), speculation=d.debug_speculation())
            d.close()


if __name__ == "__main__":
    main()
