"""Film files (include/mi355rt.h, "FILM FILE") in numpy: the format's second, independent statement.

The library writes and reads these files on the device's side (mi355rt_film_save / mi355rt_film_load / mi355rt_film_file_info); this module
needs no library and no GPU, so films of several renders of one view can be inspected and merged anywhere and loaded back later.  A film
here is a dict: width, height, seed, flags (the saving handle's config.flags), n uint32[npix], sum float32[npix, 3], sumsq float32[npix, 3],
direct float32[npix, 3] or None.  read and info make the checks the library makes of a file on its own and raise FilmFileError where it
returns MI355RT_E_LOAD.

    version 1, little-endian: 64-byte header, then the planes, nothing else
    header: b"MI355FLM" | u32 version = 1 | u32 width | u32 height | u32 planes (bit 0: direct present) | u64 seed | u32 flags | zeros
    planes: n u32[npix] | sum f32[3 npix] | sumsq f32[3 npix] | direct f32[3 npix] (only with bit 0)
"""
import os
import struct

import numpy as np

MAGIC = b"MI355FLM"
VERSION = 1
HEADER_BYTES = 64
PLANE_DIRECT = 1
_HEAD = struct.Struct("<8sIIIIQI")


class FilmFileError(ValueError):
    """a file that is not a well-formed film file; the message names the reason"""


def _header(path, head, length):
    where = "film file %s: " % path
    if len(head) < HEADER_BYTES:
        raise FilmFileError(where + "wrong file length: shorter than the 64-byte header")
    magic, version, width, height, planes, seed, flags = _HEAD.unpack_from(head)
    if magic != MAGIC:
        raise FilmFileError(where + "bad magic (not a film file)")
    if version != VERSION:
        raise FilmFileError(where + "unsupported version %d" % version)
    if planes & ~PLANE_DIRECT:
        raise FilmFileError(where + "unknown bits in the planes field")
    if width == 0 or height == 0:
        raise FilmFileError(where + "width and height must be non-zero")
    want = HEADER_BYTES + width * height * (40 if planes & PLANE_DIRECT else 28)
    if length != want:
        raise FilmFileError(where + "wrong file length: %d bytes, the header asks for %d" % (length, want))
    return dict(version=version, width=width, height=height, planes=planes, seed=seed, flags=flags)


def info(path):
    """dict(version, width, height, planes, seed, flags) of a film file, checked as mi355rt_film_file_info checks it"""
    with open(path, "rb") as f:
        head = f.read(HEADER_BYTES)
    return _header(path, head, os.path.getsize(path))


def read(path):
    """the film of a film file (see the module text), checked like info()"""
    with open(path, "rb") as f:
        data = f.read()
    h = _header(path, data[:HEADER_BYTES], len(data))
    npix = h["width"] * h["height"]
    pos = HEADER_BYTES
    n = np.frombuffer(data, "<u4", npix, pos).astype(np.uint32); pos += 4 * npix
    planes = []
    for _ in range(3 if h["planes"] & PLANE_DIRECT else 2):
        planes.append(np.frombuffer(data, "<f4", 3 * npix, pos).astype(np.float32).reshape(npix, 3)); pos += 12 * npix
    return dict(width=h["width"], height=h["height"], seed=h["seed"], flags=h["flags"], n=n, sum=planes[0], sumsq=planes[1],
                direct=planes[2] if len(planes) == 3 else None)


def film(width, height, n, sum, sumsq, direct=None, seed=0, flags=0):
    """a film dict of arrays in the layout of RayTracer.film.pixel_datas() / direct_sums(); the values are taken as they are"""
    npix = int(width) * int(height)

    def plane(a, dtype, shape):
        a = np.asarray(a)
        if a.dtype != dtype or a.size != int(np.prod(shape)):
            raise ValueError("film plane: expected %s%s, got %s%s" % (np.dtype(dtype).name, list(shape), a.dtype.name, list(a.shape)))
        return np.ascontiguousarray(a).reshape(shape)
    if npix == 0:
        raise ValueError("width and height must be non-zero")
    return dict(width=int(width), height=int(height), seed=int(seed), flags=int(flags), n=plane(n, np.uint32, (npix,)),
                sum=plane(sum, np.float32, (npix, 3)), sumsq=plane(sumsq, np.float32, (npix, 3)),
                direct=None if direct is None else plane(direct, np.float32, (npix, 3)))


def write(path, width, height, n, sum, sumsq, direct=None, seed=0, flags=0):
    """write a film file; what mi355rt_film_save writes for a handle holding these planes, byte for byte"""
    f = film(width, height, n, sum, sumsq, direct, seed, flags)
    head = _HEAD.pack(MAGIC, VERSION, f["width"], f["height"], PLANE_DIRECT if direct is not None else 0, f["seed"] & 0xFFFFFFFFFFFFFFFF,
                      f["flags"] & 0xFFFFFFFF)
    with open(path, "wb") as out:
        out.write(head + bytes(HEADER_BYTES - len(head)))
        out.write(f["n"].astype("<u4").tobytes())
        for p in (f["sum"], f["sumsq"]) + ((f["direct"],) if direct is not None else ()):
            out.write(p.astype("<f4").tobytes())


def merge(*films):
    """The film a fresh (zero) handle holds after mi355rt_film_add of every argument in turn: ((0 + f0) + f1) + ... per value, each + one f32
    addition with the running value on the left; n in u32 (wrapping, as on the device).  The films must have one size; the result has a
    direct plane when all of them have one, and the first film's seed and flags."""
    if not films:
        raise ValueError("merge: no film given")
    w, h = films[0]["width"], films[0]["height"]
    for f in films:
        if (f["width"], f["height"]) != (w, h):
            raise ValueError("merge: %d x %d and %d x %d films" % (w, h, f["width"], f["height"]))
    direct = all(f["direct"] is not None for f in films)
    npix = w * h
    out = dict(width=w, height=h, seed=films[0]["seed"], flags=films[0]["flags"], n=np.zeros(npix, np.uint32),
               sum=np.zeros((npix, 3), np.float32), sumsq=np.zeros((npix, 3), np.float32), direct=np.zeros((npix, 3), np.float32) if direct else None)
    with np.errstate(all="ignore"):
        for f in films:
            out["n"] = out["n"] + np.asarray(f["n"], np.uint32).reshape(npix)
            for k in ("sum", "sumsq") + (("direct",) if direct else ()):
                out[k] = out[k] + np.asarray(f[k], np.float32).reshape(npix, 3)
    return out
