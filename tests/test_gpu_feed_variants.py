"""The six feeds of a pass's primary round (csrc/device_types.hpp, kFeed*) under FLAG_COUNT_STEPS and without it: the counting halves of the ray-fed and
lens instantiations of the trace kernels, which no other test launches, must render what the plain halves render.

Per feed and semantics, a counting handle and a plain one render 4boxes at 37 x 21 (the frame of tests/test_gpu_tiles.py: 1554 samples at 2 spp, several chunks and
many waves; 5 x 3 tiles clipped at both edges; a ragged last row group) with 2 samples per pixel: the films agree on the bits and the counting handle's `primary` is
width * height * spp.  Under each lens the frame through render_tiles with an all-ones mask (the masked feed) is the unmasked frame, bit for bit.
A statement about behaviour, not about a build: MI355RT_LIB may point it at any library with this ABI."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SEED, SPP = 37, 21, 5, 2
T = 8
THIN = dict(model="thin", radius=0.1, focus=5.0)
ORTHO = dict(model="ortho", width_world=9.5)
FEEDS = ["camera", "rays", "thin", "ortho", "thin_masked", "ortho_masked"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def frames(pkg, scenes):
    """frame(feed, sem, count) -> (film sum bits, sumsq bits, n, the call's primary counter); every frame is rendered once, on one handle per (sem, count)"""
    cams = importlib.import_module("raytracer_rs_amd.cameras")
    handles, made = {}, {}

    def frame(feed, sem, count):
        key = (feed, sem.name, count)
        if key in made:
            return made[key]
        hk = (sem.name, count)
        if hk not in handles:
            handles[hk] = pkg.create_raytracer_from_arrays(scenes("4boxes"), pkg.DEFAULT_TRIANGLES_PER_LEAF, W, H, seed=SEED,
                                                           flags=sem.gpu | (pkg.FLAG_COUNT_STEPS if count else 0))
        rt = handles[hk]
        rt.set_lens(**(THIN if feed.startswith("thin") else ORTHO if feed.startswith("ortho") else dict(model="pinhole")))
        rt.film.clear()
        if feed == "rays":
            c = rt.render_rays(cams.pinhole(rt.camera.matrices(), W, H, SPP, SEED, film_n=rt.film.pixel_datas()[2]), SPP)
        elif feed.endswith("_masked"):
            c = rt.render_tiles(np.ones(((H + T - 1) // T, (W + T - 1) // T), np.uint8), SPP)
        else:
            c = rt.render(SPP)
        s, q, n = rt.film.pixel_datas()
        made[key] = (bits(s).copy(), bits(q).copy(), np.asarray(n).copy(), int(c.primary))
        return made[key]
    yield frame
    for rt in handles.values():
        rt.close()


@pytest.mark.parametrize("feed", FEEDS)
def test_counting_and_plain_kernels_render_the_same_film(frames, sem3, feed):
    cs, cq, cn, cprimary = frames(feed, sem3, True)
    ps, pq, pn, _ = frames(feed, sem3, False)
    assert cprimary == W * H * SPP
    assert np.all(cn == SPP) and np.array_equal(cn, pn)
    assert np.array_equal(cs, ps)
    assert np.array_equal(cq, pq)
    assert np.any(cs != 0), "an empty frame proves nothing"


@pytest.mark.parametrize("lens", ["thin", "ortho"])
def test_an_all_ones_mask_is_the_unmasked_frame(frames, sem3, lens):
    for count in (False, True):
        ms, mq, mn, _ = frames(lens + "_masked", sem3, count)
        us, uq, un, _ = frames(lens, sem3, count)
        assert np.array_equal(mn, un)
        assert np.array_equal(ms, us)
        assert np.array_equal(mq, uq)
