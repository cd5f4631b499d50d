"""Reflection rays that the direction mask of their triangle proves free are never made (bounce_skipped; csrc/reflmask.cpp, kernels.hip
reflection_proves_miss).  A handle built with the masks and one built with MI355RT_NO_REFLECT_MASK must agree bit for bit in every film, pixel and
counter but the new one — whole frames and a 50-row frame, both shipped semantics, and a frame of caller-supplied rays."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

CASES = [("ico2", 96, 40, 3), ("ico2", 96, 40, 8), ("4boxes", 64, 48, 4), ("ico3_tex", 80, 60, 2), ("thai2", 160, 120, 2)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def counters(c):
    return (c.primary, c.bounce, c.shadow, c.primary_hits, c.primary_culled, c.shadow_skipped)


def handle(pkg, monkeypatch, sc, w, h, mask, flags, **kw):
    monkeypatch.delenv("MI355RT_NO_REFLECT_MASK", raising=False)
    if not mask:
        monkeypatch.setenv("MI355RT_NO_REFLECT_MASK", "1")
    rt = pkg.create_raytracer_from_arrays(sc, 70, w, h, seed=9, flags=flags, **kw)
    assert (rt.reflect_mask_info()["bins"] != 0) == mask
    return rt


@pytest.mark.parametrize("name,w,h,spp", CASES)
def test_reflection_masks_never_change_a_frame(pkg, scenes, sem, monkeypatch, name, w, h, spp):
    sc = scenes(name)
    runs = {}
    for mask in (True, False):
        rt = handle(pkg, monkeypatch, sc, w, h, mask, sem.gpu)
        c = rt.render(spp)
        frame = (rt.film.pixel_datas(), rt.get_tonemapped_pixels())
        rt.trace_frame_additive()                               # the fused 50-row kernel
        c2 = rt.last_counts()
        runs[mask] = (frame, (rt.film.pixel_datas(), rt.get_tonemapped_pixels()), counters(c), counters(c2), c.bounce_skipped, c2.bounce_skipped)
        del rt
    on, off = runs[True], runs[False]
    for k in (0, 1):
        (fa, pa), (fb, pb) = on[k], off[k]
        assert np.array_equal(pa, pb)
        for x, y in zip(fa, fb):                                # sums, sums of squares, sample counts
            assert np.array_equal(bits(x), bits(y))
    assert on[2] == off[2] and on[3] == off[3]
    assert off[4] == 0 and off[5] == 0
    assert 0 <= on[4] <= on[2][1] and 0 <= on[5] <= on[3][1]
    print(name, w, h, spp, sem.name if hasattr(sem, "name") else "", "bounce", on[2][1], "skipped", on[4], "| 50 rows: bounce", on[3][1], "skipped", on[5])
    if name in ("thai2", "ico2"):
        assert on[4] > 0


@pytest.mark.parametrize("name,w,h,spp", [("thai2", 160, 120, 2), ("ico2", 96, 40, 3)])
def test_skipped_rays_are_not_read_by_the_trace_launches(pkg, scenes, sem, monkeypatch, name, w, h, spp):
    """bounce - bounce_skipped equals the rays the secondary launches read: the instrumented trace kernels count the rays they take from their queues
    (the primary rays walk the tree here, so that every ray of the call goes through a trace launch)."""
    monkeypatch.setenv("MI355RT_NO_RASTER", "1")
    for mask in (True, False):
        rt = handle(pkg, monkeypatch, scenes(name), w, h, mask, sem.gpu | pkg.FLAG_COUNT_STEPS)
        c = rt.render(spp)
        read = rt.debug_rays_read()
        assert read == (c.primary - c.primary_culled) + (c.bounce - c.bounce_skipped) + (c.shadow - c.shadow_skipped), (mask, read, c.as_dict())
        assert (c.bounce_skipped > 0) == mask
        del rt


def test_reflection_masks_never_change_a_frame_of_caller_rays(pkg, scenes, sem, monkeypatch):
    """render_rays: the primary round is the ray-fed instantiation of the shade kernel; rays from a point beside the camera towards the statue"""
    sc = scenes("thai2")
    w, h, spp = 64, 48, 2
    v = np.asarray(sc["tri_verts"], np.float32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    rng = np.random.default_rng(3)
    eye = (hi + (hi - lo) * np.float32(0.8)).astype(np.float32)
    target = rng.uniform(lo, hi, (w * h * spp, 3)).astype(np.float32)
    d = target - eye
    rays = np.concatenate([np.broadcast_to(eye, d.shape), d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)
    runs = {}
    for mask in (True, False):
        rt = handle(pkg, monkeypatch, sc, w, h, mask, sem.gpu)
        c = rt.render_rays(rays, spp)
        runs[mask] = (rt.film.pixel_datas(), rt.get_tonemapped_pixels(), counters(c), c.bounce_skipped)
        del rt
    on, off = runs[True], runs[False]
    assert np.array_equal(on[1], off[1]) and on[2] == off[2]
    for x, y in zip(on[0], off[0]):
        assert np.array_equal(bits(x), bits(y))
    assert off[3] == 0 and on[3] > 0
