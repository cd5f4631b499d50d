"""Adaptive sampling without a GPU: the new entry points are exported, their structs agree with the header, the default config
is the documented one, and the numpy statement of the settled / active criterion (raytracer_rs_amd.adaptive) gives the
verdicts the contract in include/mi355rt.h prescribes on hand-made films."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_adaptive_default_config", "mi355rt_render_adaptive", "mi355rt_adaptive_tile_mask"]


@pytest.fixture(scope="module")
def ad(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.adaptive")


def test_adaptive_symbols_are_exported(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)


def test_adaptive_struct_layouts_match_the_header(pkg, tmp_path):
    fields_c = [("mi355rt_adaptive_config", f) for f, _ in pkg.AdaptiveConfig._fields_] + \
               [("mi355rt_adaptive_stats", f) for f, _ in pkg.AdaptiveStats._fields_]
    src = tmp_path / "asizes.c"
    body = "".join('printf("%%zu\\n", offsetof(%s, %s));' % (s, f) for s, f in fields_c)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355rt.h"\nint main(void){printf("%zu\\n%zu\\n%u\\n",'
                   'sizeof(mi355rt_adaptive_config),sizeof(mi355rt_adaptive_stats),MI355RT_ADAPTIVE_TILE);' + body + 'return 0;}\n')
    exe = tmp_path / "asizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(pkg.AdaptiveConfig), C.sizeof(pkg.AdaptiveStats), pkg.ADAPTIVE_TILE]
    want += [getattr(pkg.AdaptiveConfig, f).offset for f, _ in pkg.AdaptiveConfig._fields_]
    want += [getattr(pkg.AdaptiveStats, f).offset for f, _ in pkg.AdaptiveStats._fields_]
    assert got == want
    assert (C.sizeof(pkg.AdaptiveConfig), C.sizeof(pkg.AdaptiveStats)) == (24, 24)


def test_adaptive_default_config_is_the_documented_one(pkg):
    c = pkg.AdaptiveConfig()
    pkg.lib().mi355rt_adaptive_default_config(C.byref(c))
    assert (c.min_spp, c.max_spp, c.batch_spp, c.max_rounds) == (16, 64, 16, 0)
    assert np.float32(c.rel_error) == np.float32(0.05) and np.float32(c.abs_floor) == np.float32(0.02)
    c2 = pkg.adaptive_config(batch_spp=3)
    assert (c2.min_spp, c2.max_spp, c2.batch_spp) == (16, 64, 3)
    with pytest.raises(TypeError):
        pkg.adaptive_config(spp=3)


def test_adaptive_calls_without_a_handle_are_rejected(pkg):
    c = pkg.adaptive_config()
    st = pkg.AdaptiveStats()
    assert pkg.lib().mi355rt_render_adaptive(None, C.byref(c), C.byref(st)) == -1
    assert pkg.lib().mi355rt_adaptive_tile_mask(None, C.byref(c), None, 0) == -1


def film(samples):
    """per-pixel lists of RGB samples -> (sum, sumsq, n) accumulated in f32 in sample order, as PixelData::add_sample does"""
    s = np.zeros((len(samples), 3), np.float32); q = np.zeros_like(s); n = np.zeros(len(samples), np.uint32)
    for i, smp in enumerate(samples):
        for c in smp:
            c = np.asarray(c, np.float32)
            s[i] = s[i] + c; q[i] = q[i] + c * c; n[i] += 1
    return s, q, n


def test_settled_criterion_on_hand_made_pixels(ad):
    cfg = dict(min_spp=2, rel_error=0.05, abs_floor=0.02)
    s, q, n = film([
        [(0.5, 0.5, 0.5)] * 8,                          # zero variance: settled
        [(0.0, 0.0, 0.0)] * 8,                          # black: 0 <= 0 settles it
        [(0.5, 0.5, 0.5)],                              # n < 2: never settled
        [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)] * 4,         # noisy: not settled
        [(0.5, 0.5, 0.5)] * 7 + [(0.5, 0.5, 1.5)],      # one channel noisy: not settled
    ])
    assert ad.settled_pixels(s, q, n, **cfg).tolist() == [True, True, False, False, False]
    # NaN never passes, in any channel
    s2, q2 = s.copy(), q.copy(); s2[0, 1] = np.nan; q2[1, 2] = np.nan
    assert ad.settled_pixels(s2, q2, n, **cfg).tolist()[:2] == [False, False]
    # min_spp: the zero-variance pixel with 8 samples is not settled below min_spp = 9
    assert not ad.settled_pixels(s, q, n, min_spp=9, rel_error=0.05, abs_floor=0.02)[0]
    # rel_error = 0 settles exactly the zero-variance pixels
    assert ad.settled_pixels(s, q, n, min_spp=2, rel_error=0.0, abs_floor=0.0).tolist() == [True, True, False, False, False]


def test_floor_judges_dark_pixels_against_it(ad):
    # a dark noisy pixel: mean 0.005, standard error 0.0013 -- above 5 % of max(mean, 0.02), below 5 % of a floor of 0.2
    smp = [(0.0, 0.0, 0.0), (0.01, 0.01, 0.01)] * 8
    s, q, n = film([smp])
    assert not ad.settled_pixels(s, q, n, min_spp=2, rel_error=0.05, abs_floor=0.02)[0]
    assert ad.settled_pixels(s, q, n, min_spp=2, rel_error=0.05, abs_floor=0.2)[0]
    # the same expression by hand, in f32
    fn = np.float32(16); sc, qc = s[0, 0], q[0, 0]
    lhs = fn * qc - sc * sc
    m = max(sc, np.float32(0.2) * fn)
    assert lhs <= (np.float32(0.05) * np.float32(0.05)) * ((fn - np.float32(1)) * (m * m))


def test_tile_mask_geometry_ownership_and_the_max_spp_cap(ad):
    w, h = 20, 11                                        # tiles 3 x 2, clipped at the right and bottom
    npix = w * h
    rng = np.random.default_rng(3)
    smp = rng.uniform(0, 1, (npix, 4, 3)).astype(np.float32)
    s, q, n = film([list(p) for p in smp])
    cfg = dict(min_spp=2, max_spp=64, batch_spp=8, rel_error=0.05, abs_floor=0.02)
    m = ad.tile_mask(s, q, n, w, h, **cfg)
    assert m.shape == (2, 3) and m.dtype == np.uint8 and m.all()                  # noisy everywhere
    # cap: 4 samples + batch 8 > max_spp 11 -> nothing active; == 12 -> active
    assert not ad.tile_mask(s, q, n, w, h, **dict(cfg, max_spp=11)).any()
    assert ad.tile_mask(s, q, n, w, h, **dict(cfg, max_spp=12)).all()
    # the cap looks at the largest n of the tile's owned pixels
    n2 = n.copy(); n2[5] = 100                            # pixel (0, 5): tile (0, 0)
    assert ad.tile_mask(s, q, n2, w, h, **cfg).tolist() == [[0, 1, 1], [1, 1, 1]]
    # settle tile (1, 2) (rows 8-10, columns 16-19) by zero variance
    s3, q3 = s.copy(), q.copy()
    for y in range(8, 11):
        for x in range(16, 20):
            p = y * w + x
            s3[p] = np.float32(4) * np.float32(0.25); q3[p] = np.float32(4) * np.float32(0.0625)
    assert ad.tile_mask(s3, q3, n, w, h, **cfg).tolist() == [[1, 1, 1], [1, 1, 0]]
    # ownership: rows 0-3 and 8-10 (stripes of 4, rank 0 of 2): tile row 1 keeps rows 8-10, tile row 0 rows 0-3; a pixel that
    # is not owned neither keeps its tile active nor caps it
    owned = [0, 1, 2, 3, 8, 9, 10]
    n4 = n.copy(); n4[4 * w:8 * w] = 1000                # rows 4-7 are not owned: their n does not cap tile row 0
    assert ad.tile_mask(s3, q3, n4, w, h, owned_rows=owned, **cfg).tolist() == [[1, 1, 1], [1, 1, 0]]
    # a tile with no owned pixel is never active
    assert ad.tile_mask(s, q, n, w, h, owned_rows=[8, 9, 10], **cfg).tolist() == [[0, 0, 0], [1, 1, 1]]
    assert ad.pixel_tiles(w, h)[10, 19] == 5 and ad.pixel_tiles(w, h)[7, 8] == 1
