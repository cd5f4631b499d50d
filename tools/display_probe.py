#!/usr/bin/env python3
"""What the display read-out costs, on thai2 at 1920x1080 and 16 spp.

Prints one JSON line per measurement:
  film        the render the read-outs below read (ms), the handle's device memory
  histogram   per source: occupied bins (first, last, count), empty / nan / nonpositive, the largest luminance, the auto exposure at key 0.18 over
              all pixels and over the 1 % .. 99 % ranks
  readout     wall-clock ms of get_tonemapped_pixels (no row changed since the last call; every row changed), get_denoised_pixels and its split
              form (packed only), display_histogram per source and get_display_pixels per source with auto-exposure off and on, with the default
              mapping (Reinhard, reference transfer) and with ACES + sRGB
  flat        the same display read-outs of the film source on a flat film (every pixel in one bin: a whole wave counts in one LDS word)
Timings are wall-clock medians of --reps calls after one warm-up call, the calls of a group taken in turn.  The kernels' own times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/display_probe.py --reps 2`: the dispatches behind the last film_merge_kernel are the flat film's.
usage: tools/display_probe.py [--width 1920 --height 1080] [--spp 16] [--reps 5] [--skip-flat]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-flat", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    scene = scene_io.load_scene_file(os.path.join(ROOT, "tests", "golden", "scenes", "thai2.scene"))
    w, h = a.width, a.height
    npix = w * h

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def measure(what, entries):
        """entries: (labels, call, before or None).  The calls are timed in turn, --reps + 1 rounds over the whole list (the first round warms up), so
        that no call's figure depends on where in the list it stands; one JSON line each: the median and the extremes of its rounds"""
        ts = [[] for _ in entries]
        for _ in range(a.reps + 1):
            for k, (_, fn, before) in enumerate(entries):
                if before:
                    before()
                t0 = time.perf_counter()
                fn()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (labels, _, _), t in zip(entries, ts):
            emit(what=what, **labels, ms=round(float(np.median(t[1:])), 4), ms_min=round(min(t[1:]), 4), ms_max=round(max(t[1:]), 4))

    rt = pkg.create_raytracer_from_arrays(scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1, flags=pkg.FLAG_DIRECT_FILM)
    c = rt.render(a.spp)
    emit(what="film", width=w, height=h, spp=a.spp, render_ms=round(c.total_ms, 3), hbm_bytes=rt.hbm_allocated_bytes())
    zeros3, zeros1 = np.zeros((npix, 3), np.float32), np.zeros(npix, np.uint32)

    def touch():
        """every row changed, the film the same: film + 0 (get_tonemapped_pixels maps only the rows written since its last call)"""
        rt.film.add(zeros3, zeros3, zeros1, zeros3)
        rt.synchronize()

    out = np.zeros(npix, np.uint32)
    for source in (0, 1, 2):
        hist = rt.display_histogram(source)
        used = np.flatnonzero(hist["bins"])
        emit(what="histogram", source=source, first_bin=int(used[0]), last_bin=int(used[-1]), bins_used=int(used.size), empty=hist["empty"], nan=hist["nan"],
             nonpositive=hist["nonpositive"], max_luminance=float(np.array([hist["max_bits"]], np.uint32).view(np.float32)[0]),
             log2_range=[(int(used[0]) + 856) / 8.0 - 127.0, (int(used[-1]) + 857) / 8.0 - 127.0],
             auto_exposure=float(pkg.display_auto_exposure(hist)), auto_exposure_1_99=float(pkg.display_auto_exposure(hist, 0.18, 0.01, 0.99)))

    def readouts(what, sources):
        used = {}
        entries = [(dict(call="get_tonemapped_pixels, no row changed"), lambda: rt.get_tonemapped_pixels(out), None),
                   (dict(call="get_tonemapped_pixels, every row changed"), lambda: rt.get_tonemapped_pixels(out), touch)]
        for source in sources:
            if source:
                entries.append((dict(call="get_denoised_pixels%s, packed" % ("_split" if source == 2 else "")),
                                lambda source=source: rt.get_denoised_pixels(rgb=False, split=source == 2), None))
            entries.append((dict(call="display_histogram", source=source), lambda source=source: rt.display_histogram(source), None))
            for name, kw in (("default", {}), ("aces + srgb", dict(curve=pkg.CURVE_ACES, transfer=pkg.TRANSFER_SRGB))):
                for auto in (0, 1):
                    def call(source=source, name=name, kw=kw, auto=auto):
                        used[(source, name, auto)] = float(rt.get_display_pixels(out=out, source=source, auto_exposure=auto, **kw)[1])
                    entries.append((dict(call="get_display_pixels", source=source, mapping=name, auto_exposure=auto), call, None))
        measure(what, entries)
        emit(what=what + " exposures", exposure_used={"source %d, %s, auto %d" % k: v for k, v in used.items()})

    readouts("readout", (0, 1, 2))
    if not a.skip_flat:
        rt.film.set(np.tile(np.asarray([[2.0, 3.0, 1.0]], np.float32), (npix, 1)), zeros3, np.full(npix, 4, np.uint32), zeros3)
        hist = rt.display_histogram(0)
        assert int((hist["bins"] > 0).sum()) == 1 and int(hist["bins"].sum()) == npix
        readouts("flat", (0,))
    rt.close()


if __name__ == "__main__":
    main()
