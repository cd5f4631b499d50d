#!/usr/bin/env python3
"""What film set / add / save / load cost on thai2 at 1920x1080, without and with a direct film.

Prints one JSON line per handle kind: wall-clock medians (ms) of --reps calls after one warm-up call of Film.set, Film.add, Film.save and
Film.load (each call returns after the device has finished: mi355rt_film_set synchronises), of film_get (+ film_get_direct) for scale,
the bytes a call moves over the host link, and the file's size.  Run it under `rocprofv3 --kernel-trace --stats` for the device time of
film_merge_kernel<ADD, DIRECT>.
usage: tools/film_io_probe.py [--width 1920 --height 1080] [--reps 7] [--spp 4] [--dir DIR]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--dir", default=None, help="where the film file goes (default: a temporary directory)")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    import importlib
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h = a.width, a.height

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)

    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for direct in (False, True):
            rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1, flags=pkg.FLAG_DIRECT_FILM if direct else 0)
            rt.render(a.spp)
            s, q, n = rt.film.pixel_datas()
            d = rt.film.direct_sums() if direct else None
            path = os.path.join(tmp, "probe.film")
            hbm = rt.hbm_allocated_bytes()
            out = dict(what="film_io", width=w, height=h, direct_film=direct, reps=a.reps, bytes_per_pixel=40 if direct else 28,
                       host_link_mb=round(w * h * (40 if direct else 28) / 1e6, 2))
            out["get_ms"] = median_ms(lambda: (rt.film.pixel_datas(), rt.film.direct_sums() if direct else None))
            out["set_ms"] = median_ms(lambda: rt.film.set(s, q, n, d))
            out["add_ms"] = median_ms(lambda: rt.film.add(s, q, n, d))
            rt.film.set(s, q, n, d)
            out["save_ms"] = median_ms(lambda: rt.film.save(path))
            out["file_bytes"] = os.path.getsize(path)
            out["load_ms"] = median_ms(lambda: rt.film.load(path))
            out["load_add_ms"] = median_ms(lambda: rt.film.load(path, add=True))
            out["hbm_unchanged"] = rt.hbm_allocated_bytes() == hbm
            out["columns"] = "median, min, max"
            print(json.dumps(out), flush=True)
            rt.close()


if __name__ == "__main__":
    main()
