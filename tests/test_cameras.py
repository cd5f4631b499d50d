"""raytracer_rs_amd.cameras: ray generators in numpy, no GPU.  `pinhole` is held to the CPU oracle's primary rays bit for bit — every pixel of
two image sizes, with and without FIX_ROW_INDEX, before and after the camera moved — and the others to what their statements promise."""
import importlib

import numpy as np
import pytest

SIZES = [(37, 21), (16, 12)]
SPP = 3
SEED = 5


@pytest.fixture(scope="module")
def cams(pkg):
    return importlib.import_module("raytracer_rs_amd.cameras")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_rays(orc, npix, spp):
    return np.array([[orc.primary_ray(p, s) for p in range(npix)] for s in range(spp)], np.float32).reshape(-1, 6)


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("w,h", SIZES)
def test_pinhole_equals_the_oracles_primary_rays(cams, oracle, scenes, w, h, fix):
    orc = oracle.Oracle(scenes("thai2"), w, h, seed=SEED, flags=oracle.FLAG_FIX_ROW_INDEX if fix else 0)
    for moved in (False, True):
        if moved:
            orc.camera_move_rel(0.3, -0.2, 0.5); orc.camera_add_y_angle(0.2); orc.camera_add_x_angle(-0.1)
        got = cams.pinhole(orc.camera_matrices(), w, h, SPP, SEED, flags=fix)
        assert got.shape == (w * h * SPP, 6) and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(bits(got), bits(oracle_rays(orc, w * h, SPP))), (w, h, fix, moved)
    orc.close()


def test_pinhole_numbers_its_samples_from_film_n(cams, oracle, scenes):
    w, h = 16, 12
    orc = oracle.Oracle(scenes("ico2"), w, h, seed=SEED)
    film_n = (np.arange(w * h, dtype=np.uint32) * 7) % 5
    got = cams.pinhole(orc.camera_matrices(), w, h, 2, SEED, film_n=film_n).reshape(2, w * h, 6)
    want = np.array([[orc.primary_ray(p, int(film_n[p]) + s) for p in range(w * h)] for s in range(2)], np.float32)
    assert np.array_equal(bits(got), bits(want))
    with pytest.raises(ValueError, match="film_n"):
        cams.pinhole(orc.camera_matrices(), w, h, 2, SEED, film_n=film_n[:-1])
    orc.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_thin_lens_of_radius_zero_and_focus_one_is_pinhole(cams, oracle, scenes, w, h):
    orc = oracle.Oracle(scenes("thai2"), w, h, seed=SEED)
    orc.camera_move_rel(0.3, -0.2, 0.5); orc.camera_add_y_angle(0.2)
    cam = orc.camera_matrices()
    assert np.array_equal(bits(cams.thin_lens(cam, w, h, SPP, SEED, 0.0, 1.0)), bits(cams.pinhole(cam, w, h, SPP, SEED)))
    # a real lens moves the origins by at most radius * sqrt(2) * the longest rotation row, and every ray still passes through o + focus * d
    lens, pin = cams.thin_lens(cam, w, h, SPP, SEED, 0.25, 3.0), cams.pinhole(cam, w, h, SPP, SEED)
    off = lens[:, :3] - pin[:, :3]
    assert 0.05 < np.abs(off).max() < 0.25 * 1.5
    through = lens[:, :3] + lens[:, 3:]                      # t = 1 along d' = focus * d - off
    assert np.allclose(through, pin[:, :3] + 3.0 * pin[:, 3:], atol=1e-5)
    orc.close()


def test_orthographic_directions_are_equal_and_origins_span_the_width(cams, oracle, scenes):
    w, h, width_world = 37, 21, 6.0
    orc = oracle.Oracle(scenes("4boxes"), w, h, seed=SEED)
    cam = orc.camera_matrices()
    rays = cams.orthographic(cam, w, h, SPP, SEED, width_world)
    assert rays.shape == (w * h * SPP, 6)
    assert np.all(bits(rays[:, 3:]) == bits(rays[0, 3:]))                      # one direction: the optical axis
    centre = cams.pinhole(cam, 1, 1, 1, SEED)                                    # its direction at the image centre, up to the jitter of that one sample
    rot = cam[0].reshape(4, 4)
    assert np.array_equal(bits(rays[0, 3:]), bits(rot[2, :3] + rot[3, :3]))
    assert np.dot(rays[0, 3:], centre[0, 3:]) > 0.9 * np.dot(rays[0, 3:], rays[0, 3:])
    # the origins lie on the image plane through the camera position and span width_world x width_world * h / w (to within one pixel of jitter)
    rel = (rays[:, :3] - centre[0, :3]).astype(np.float64)
    right, up, axis = (rot[k, :3].astype(np.float64) for k in range(3))
    sx, sy = rel @ right / (right @ right), rel @ up / (up @ up)
    assert np.abs(rel @ axis).max() < 1e-4
    assert width_world * (1 - 1.0 / w) <= sx.max() - sx.min() <= width_world
    assert width_world * h / w * (1 - 1.0 / h) <= sy.max() - sy.min() <= width_world * h / w
    # pixel 0 is the top left corner: right grows with the column, up falls with the row
    grid_x, grid_y = sx[:w * h].reshape(h, w), sy[:w * h].reshape(h, w)
    assert np.all(np.diff(grid_x[:, ::2], axis=1) > 0) and np.all(np.diff(grid_y[::2], axis=0) < 0)
    orc.close()


def test_equirect_directions_are_unit_and_cover_both_hemispheres(cams, oracle, scenes):
    w, h = 16, 12
    orc = oracle.Oracle(scenes("ico2"), w, h, seed=SEED)
    cam = orc.camera_matrices()
    rays = cams.equirect(cam, w, h, SPP, SEED)
    d = rays[:, 3:].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-6
    rot = cam[0].reshape(4, 4).astype(np.float64)
    for axis in (rot[0, :3], rot[1, :3], rot[2, :3]):                           # in front and behind, left and right, above and below
        assert (d @ axis).max() > 0.8 and (d @ axis).min() < -0.8
    assert np.all(bits(rays[:, :3]) == bits(rays[0, :3]))                      # one origin: the camera position
    top, bottom = d[:w] @ rot[1, :3], d[w * (h - 1):w * h] @ rot[1, :3]
    assert top.min() > 0.8 and bottom.max() < -0.8
    orc.close()


def test_generators_check_their_arguments(cams):
    cam = (np.eye(4, dtype=np.float32).reshape(-1), np.eye(4, dtype=np.float32).reshape(-1), np.array([0.4, 0.3], np.float32))
    with pytest.raises(ValueError, match="cam"):
        cams.pinhole((cam[0][:9], cam[1], cam[2]), 4, 3, 1, 1)
    with pytest.raises(ValueError, match="spp"):
        cams.orthographic(cam, 4, 3, 0, 1, 2.0)
    assert cams.equirect(cam, 4, 3, 2, 1).shape == (24, 6)
