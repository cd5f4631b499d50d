"""mi355rt_render_tiles without a GPU (include/mi355rt.h, "RENDER TILES"): the symbol is declared and exported; adaptive.region_mask equals
its brute-force statement; adaptive.refine — the adaptive loop on the caller's side — is driven by a fake handle with scripted verdicts."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 8


@pytest.fixture(scope="module")
def ad(pkg):
    return importlib.import_module("raytracer_rs_amd.adaptive")


def test_header_declares_and_library_exports_render_tiles(pkg):
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    m = re.search(r"\bint\s+mi355rt_render_tiles\s*\(([^;]*)\)\s*;", header)
    assert m, "mi355rt_render_tiles is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[0].replace(" *", "*") for a in args] == ["mi355rt_handle*", "const uint8_t*", "size_t", "uint32_t", "uint32_t", "mi355rt_ray_counts*"]
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "raytracer-rs_amd", "libmi355rt.so")], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mi355rt_render_tiles\b", out)
    assert any(name == "mi355rt_render_tiles" for name, _, _ in pkg.ABI)
    # a NULL handle is refused before anything is touched
    assert pkg.lib().mi355rt_render_tiles(None, None, 0, 1, 0, None) == -1


def brute_region(w, h, x0, y0, x1, y1):
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    out = np.zeros((ty, tx), np.uint8)
    for y in range(h):
        for x in range(w):
            if x0 <= x < x1 and y0 <= y < y1:
                out[y // TILE, x // TILE] = 1
    return out


RECTS = [
    (9, 3, 20, 12), (8, 8, 16, 16), (10, 10, 11, 11), (0, 0, 1, 1),                  # inside the image
    (-5, 2, 4, 9), (30, 5, 99, 9), (3, -7, 12, 2), (3, 17, 12, 50),                  # across the left, right, top and bottom edge
    (-9, -9, 3, 3), (33, 18, 40, 30),                                                # across two edges at a corner
    (5, 5, 5, 9), (7, 9, 3, 12), (4, 4, 9, 4), (-8, 0, 0, 5), (37, 0, 50, 5), (0, 21, 9, 30), (100, 100, 200, 200),   # empty: zero width / height, inverted, wholly outside
    (0, 0, 37, 21), (-100, -100, 100, 100), (0, 0, 5, 3),                            # everything
]


@pytest.mark.parametrize("w,h", [(37, 21), (5, 3)])
def test_region_mask_equals_the_brute_force_statement(ad, w, h):
    seen = set()
    for r in RECTS:
        got = ad.region_mask(w, h, *r)
        want = brute_region(w, h, *r)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), r
        seen.add(int(want.sum()))
    assert 0 in seen and ((w + 7) // 8) * ((h + 7) // 8) in seen      # an empty and a full mask occurred
    if (w, h) == (37, 21):
        assert len(seen) > 4


class Counts:
    def __init__(self, primary, bounce, shadow, primary_hits):
        self.primary, self.bounce, self.shadow, self.primary_hits = primary, bounce, shadow, primary_hits


class FakeHandle:
    """adaptive_tile_mask hands out the scripted verdicts one after the other; render_tiles records its arguments and returns scripted counters"""

    def __init__(self, w, h, verdicts, owned=None):
        self.width, self.height = w, h
        self.verdicts, self.owned = list(verdicts), list(range(h)) if owned is None else owned
        self.calls, self.cfgs = [], []

    def owned_rows(self):
        return np.asarray(self.owned, np.uint32)

    def adaptive_tile_mask(self, **cfg):
        self.cfgs.append(cfg)
        return self.verdicts[len(self.cfgs) - 1].copy()

    def render_tiles(self, mask, spp):
        self.calls.append((np.array(mask), spp))
        k = len(self.calls)
        return Counts(100 * k, 10 * k, 20 * k + 1, 7 * k)


def verdict(w, h, *tiles):
    m = np.zeros(((h + 7) // 8, (w + 7) // 8), np.uint8)
    for t in tiles:
        m[t] = 1
    return m


def test_refine_stops_when_no_tile_is_active(ad):
    w, h = 37, 21
    v = [verdict(w, h, (0, 0), (1, 2), (2, 4)), verdict(w, h, (1, 2)), verdict(w, h)]
    rt = FakeHandle(w, h, v)
    out = ad.refine(rt, batch_spp=3, min_spp=2, max_spp=50, rel_error=0.25)
    assert len(rt.cfgs) == 3 and len(rt.calls) == 2
    assert all(c == dict(batch_spp=3, min_spp=2, max_spp=50, rel_error=0.25) for c in rt.cfgs)
    assert [spp for _, spp in rt.calls] == [3, 3]
    assert np.array_equal(rt.calls[0][0], v[0]) and np.array_equal(rt.calls[1][0], v[1])
    assert out == dict(rounds=2, tiles=15, tiles_active_first=3, tiles_active_last=0, samples_added=300, primary=300, bounce=30, shadow=62, primary_hits=21)


def test_refine_stops_at_max_rounds_and_uses_the_default_batch(ad, pkg):
    w, h = 37, 21
    v = [verdict(w, h, (0, 0), (0, 1)), verdict(w, h, (0, 1), (2, 2), (2, 3), (1, 1)), verdict(w, h, (2, 2)), verdict(w, h, (2, 2))]
    rt = FakeHandle(w, h, v, owned=[0, 1, 2, 3, 16, 17, 18, 19])          # two of the three tile rows hold an owned row
    out = ad.refine(rt, max_rounds=2)
    assert len(rt.cfgs) == 3 and len(rt.calls) == 2
    assert [spp for _, spp in rt.calls] == [pkg.adaptive_config().batch_spp] * 2 == [16, 16]
    assert out["rounds"] == 2 and out["tiles"] == 10 and out["tiles_active_first"] == 2 and out["tiles_active_last"] == 1
    assert out["samples_added"] == out["primary"] == 300 and out["bounce"] == 30 and out["shadow"] == 62 and out["primary_hits"] == 21
    # nothing active at the first verdict: no call at all
    idle = FakeHandle(w, h, [verdict(w, h)])
    out = ad.refine(idle)
    assert idle.calls == [] and out["rounds"] == 0 and out["samples_added"] == 0 and out["tiles_active_first"] == out["tiles_active_last"] == 0
    with pytest.raises(TypeError):
        ad.refine(FakeHandle(w, h, [verdict(w, h)]), no_such_field=1)
