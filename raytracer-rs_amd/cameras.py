"""Ray generators for RayTracer.render_rays / mi355rt_render_rays (include/mi355rt.h, "caller-supplied rays").

Host code, numpy float32, no GPU.  Every generator returns float32[(npix * spp), 6] in render_rays layout: row s * npix + p is the ray (pos3, dir3) of the
call's sample s of film pixel p, npix = width * height.  They share their arguments:

    cam      (rot16, orient16, max_xy) as RayTracer.camera.matrices() / mi355rt_camera_get return them
    width, height, spp
    seed     the handle's seed (its low 32 bits)
    film_n   uint32[npix], the film's sample counts BEFORE the call (Film.pixel_datas()[2]); None: a fresh film.  Sample s of pixel p is
             numbered film_n[p] + s, and its jitter is words 0 and 1 of pcg4d(p, film_n[p] + s, 0, seed) — the library's own jitter, so `pinhole`
             reproduces the rays mi355rt_render makes, bit for bit.

Every expression below is f32, unfused, in the order written: the operand order of pixel_ray in csrc/kernels.hip for `pinhole`, and the order the C++
CLI repeats for `orthographic` (csrc/cli/raytracer_main.cpp), so that the bytes of both paths can be held to each other.
"""
import numpy as np

FLAG_FIX_ROW_INDEX = 1
_F = np.float32


def pcg4d(x, y, z, w):
    """pcg4d (Jarzynski & Olano, JCGT 2020) on uint32 arrays, as csrc/device_math.hpp runs it; returns the four words"""
    x, y, z, w = (np.array(np.broadcast_to(np.asarray(a, np.uint32), np.broadcast(x, y, z, w).shape), np.uint32) for a in (x, y, z, w))
    m, c = np.uint32(1664525), np.uint32(1013904223)
    with np.errstate(over="ignore"):
        x = x * m + c; y = y * m + c; z = z * m + c; w = w * m + c
        x = x + y * w; y = y + z * x; z = z + x * y; w = w + y * z
        x = x ^ (x >> np.uint32(16)); y = y ^ (y >> np.uint32(16)); z = z ^ (z >> np.uint32(16)); w = w ^ (w >> np.uint32(16))
        x = x + y * w; y = y + z * x; z = z + x * y; w = w + y * z
    return x, y, z, w


def u01(bits):
    """23 random mantissa bits -> [0, 1) (device_math.hpp)"""
    return (bits >> np.uint32(9)).astype(_F) * _F(1.0 / 8388608.0)


def _setup(cam, width, height, spp, seed, film_n):
    rot, orient, max_xy = (np.ascontiguousarray(a, _F).reshape(-1) for a in cam)
    if rot.size != 16 or orient.size != 16 or max_xy.size != 2:
        raise ValueError("cam must be (rot16, orient16, max_xy) as RayTracer.camera.matrices() returns them")
    width, height, spp = int(width), int(height), int(spp)
    if width < 1 or height < 1 or spp < 1:
        raise ValueError("width, height and spp must be >= 1")
    npix = width * height
    n = np.zeros(npix, np.uint32) if film_n is None else np.ascontiguousarray(film_n, np.uint32).reshape(-1)
    if n.size != npix:
        raise ValueError("film_n must hold width * height counts")
    pixel = np.arange(npix, dtype=np.uint32)[None, :]
    with np.errstate(over="ignore"):
        sampleno = n[None, :] + np.arange(spp, dtype=np.uint32)[:, None]
    words = pcg4d(pixel, sampleno, np.uint32(0), np.uint32(int(seed) & 0xFFFFFFFF))
    # orientation * (0, 0, 0, 1), camera.rs:88, in vecmath's operand order
    z, one = _F(0.0), _F(1.0)
    origin = [z * orient[k] + z * orient[4 + k] + z * orient[8 + k] + one * orient[12 + k] for k in range(3)]
    return rot, origin, max_xy, width, height, npix, pixel, words


def _screen(max_xy, width, height, pixel, xi1, xi2, fix_row):
    """(dir_x, dir_y) of camera.rs:81-84 as pixel_ray evaluates them; fix_row False: the reference's idx / height"""
    cu = (pixel % np.uint32(width)).astype(_F)
    cv = (pixel // np.uint32(width if fix_row else height)).astype(_F)
    dir_x = -max_xy[0] + (_F(2.0) * max_xy[0]) * ((cu + xi1) / _F(width))
    dir_y = -max_xy[1] + (_F(2.0) * max_xy[1]) * ((cv + xi2) / _F(height))
    return dir_x, dir_y


def _pinhole_parts(rot, origin, max_xy, width, height, pixel, words, flags):
    dir_x, dir_y = _screen(max_xy, width, height, pixel, u01(words[0]), u01(words[1]), bool(flags & FLAG_FIX_ROW_INDEX))
    vx, vy, one = dir_x, -dir_y, _F(1.0)
    d = [vx * rot[k] + vy * rot[4 + k] + one * rot[8 + k] + one * rot[12 + k] for k in range(3)]
    o = [np.broadcast_to(origin[k], d[0].shape) for k in range(3)]
    return o, d


def _pack(o, d):
    out = np.empty(o[0].shape + (6,), _F)
    for k in range(3):
        out[..., k] = o[k]; out[..., 3 + k] = d[k]
    return out.reshape(-1, 6)


def pinhole(cam, width, height, spp, seed, film_n=None, flags=0):
    """The reference's Camera::get_ray (camera.rs:80-90) under the library's jitter: the rays of mi355rt_render.  flags: the handle's flags
    (FLAG_FIX_ROW_INDEX selects the true row instead of the reference's idx / height)."""
    rot, origin, max_xy, width, height, npix, pixel, words = _setup(cam, width, height, spp, seed, film_n)
    return _pack(*_pinhole_parts(rot, origin, max_xy, width, height, pixel, words, flags))


def thin_lens(cam, width, height, spp, seed, radius, focus, film_n=None, flags=0):
    """Depth of field: the pinhole ray (o, d) leaves from a point of a square lens of half-width `radius` around o and passes through the point
    o + focus * d, which stays sharp.  The lens sample (lx, ly) in [-1, 1)^2 comes from words 2 and 3 of the same pcg4d hash whose words 0 and 1 are
    the jitter (nothing else uses them):  off = radius * (lx * right + ly * up),  o' = o + off,  d' = focus * d - off  (right, up: rows 0 and 1 of the
    rotation matrix).  radius 0 and focus 1 give `pinhole` bit for bit."""
    rot, origin, max_xy, width, height, npix, pixel, words = _setup(cam, width, height, spp, seed, film_n)
    o, d = _pinhole_parts(rot, origin, max_xy, width, height, pixel, words, flags)
    lx = _F(2.0) * u01(words[2]) - _F(1.0)
    ly = _F(2.0) * u01(words[3]) - _F(1.0)
    r, f = _F(radius), _F(focus)
    off = [r * (lx * rot[k] + ly * rot[4 + k]) for k in range(3)]
    return _pack([o[k] + off[k] for k in range(3)], [f * d[k] - off[k] for k in range(3)])


def orthographic(cam, width, height, spp, seed, width_world, film_n=None):
    """Parallel projection: the direction is the optical axis (the pinhole ray of the image centre, rot row 2 + row 3), the origin moves on the image
    plane through the camera position, `width_world` wide and width_world * height / width high:
        hw = width_world / 2, hh = hw * (height / width)
        sx = -hw + (2 hw) * ((x + xi1) / width),  sy = -hh + (2 hh) * ((y + xi2) / height)     x = p % width, y = p / width (the true row)
        o = (origin + sx * right) + (-sy) * up
    Arithmetic only (the C++ CLI's --ortho-width repeats it)."""
    rot, origin, max_xy, width, height, npix, pixel, words = _setup(cam, width, height, spp, seed, film_n)
    hw = _F(width_world) * _F(0.5)
    hh = hw * (_F(height) / _F(width))
    sx, sy = _screen(np.array([hw, hh], _F), width, height, pixel, u01(words[0]), u01(words[1]), True)
    o = [(origin[k] + sx * rot[k]) + (-sy) * rot[4 + k] for k in range(3)]
    d = [np.broadcast_to(rot[8 + k] + rot[12 + k], sx.shape) for k in range(3)]
    return _pack(o, d)


def equirect(cam, width, height, spp, seed, film_n=None):
    """A full panorama from the camera position: column -> longitude phi in [-pi, pi) around the up axis (0 = the optical axis), row -> polar angle
    theta in [0, pi] from up; unit directions  d = (sin theta sin phi) right + (cos theta) up + (sin theta cos phi) forward."""
    rot, origin, max_xy, width, height, npix, pixel, words = _setup(cam, width, height, spp, seed, film_n)
    u = ((pixel % np.uint32(width)).astype(_F) + u01(words[0])) / _F(width)
    v = ((pixel // np.uint32(width)).astype(_F) + u01(words[1])) / _F(height)
    phi = (_F(2.0 * np.pi) * (u - _F(0.5))).astype(np.float64)
    theta = (_F(np.pi) * v).astype(np.float64)
    lx, ly, lz = np.sin(theta) * np.sin(phi), np.cos(theta), np.sin(theta) * np.cos(phi)
    r = rot.astype(np.float64)
    # the rows of the rotation matrix, made orthonormal in f64 first: the result is unit length to f32 rounding
    right, up, fwd = r[0:3] / np.linalg.norm(r[0:3]), r[4:7] / np.linalg.norm(r[4:7]), r[8:11] / np.linalg.norm(r[8:11])
    d = [(lx * right[k] + ly * up[k] + lz * fwd[k]).astype(_F) for k in range(3)]
    o = [np.broadcast_to(origin[k], d[0].shape) for k in range(3)]
    return _pack(o, d)
