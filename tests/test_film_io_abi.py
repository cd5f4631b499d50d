"""Film set / add / save / load without a GPU (include/mi355rt.h): the header declares, the library exports, and the ctypes
mirror, the C++ mirror and the Rust shim list the five entry points; calls without a handle or a path are rejected; the numpy statement of
the file format (raytracer_rs_amd.film_io) round-trips, merges as the contract says and rejects every malformed file; and the library's
host-side mi355rt_film_file_info agrees with it on good and on malformed files."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_film_set", "mi355rt_film_add", "mi355rt_film_save", "mi355rt_film_load", "mi355rt_film_file_info"]
E_INVALID, E_LOAD = -1, -3


@pytest.fixture(scope="module")
def fio(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.film_io")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_film(w, h, seed, direct=True):
    """planes with awkward values: a NaN with a payload, -0.0, an infinity, a denormal, counts near the top of u32"""
    rng = np.random.default_rng(seed)
    npix = w * h
    s = rng.random((npix, 3), np.float32) * 9; q = rng.random((npix, 3), np.float32) * 90
    d = rng.random((npix, 3), np.float32) if direct else None
    n = rng.integers(0, 50, npix).astype(np.uint32)
    s.view(np.uint32)[0, 0] = 0x7FC12345; s[1, 1] = -0.0; q[2, 2] = np.inf; q.view(np.uint32)[3, 0] = 1; n[4] = 0xFFFFFFF0
    return s, q, n, d


def test_film_io_symbols_are_declared_everywhere(pkg):
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    header_nc = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    rust = open(os.path.join(ROOT, "raytracer-rs_amd", "integration", "rust_shim", "src", "lib.rs")).read()
    cpp = open(os.path.join(ROOT, "raytracer-rs_amd", "csrc", "raytracer_lib.hpp")).read()
    proto = {n: (r, a) for n, r, a in pkg.ABI}
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header_nc), name
        assert " T %s\n" % name in exported, name
        assert name in proto and proto[name][0] is C.c_int and hasattr(pkg.lib(), name)
        assert getattr(pkg.lib(), name).argtypes == proto[name][1]
        assert re.search(r"fn\s+%s\s*\(" % name, rust), name
        assert name + "(" in cpp, name
    assert [len(proto[n][1]) for n in NEW] == [6, 6, 2, 3, 2]
    assert proto["mi355rt_film_set"] == proto["mi355rt_film_add"]
    for method in ("set", "add", "save", "load"):
        assert callable(getattr(pkg.Film, method))
        assert re.search(r"\bvoid\s+%s\s*\(" % method, cpp), method
    assert callable(pkg.film_file_info)


def test_film_io_calls_without_a_handle_or_a_path_are_rejected(pkg, tmp_path):
    L = pkg.lib()
    s = np.ones((4, 3), np.float32); n = np.ones(4, np.uint32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))            # noqa: E731
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))           # noqa: E731
    assert L.mi355rt_film_set(None, fp(s), fp(s), up(n), None, 4) == E_INVALID
    assert L.mi355rt_film_add(None, fp(s), fp(s), up(n), None, 4) == E_INVALID
    assert L.mi355rt_film_set(None, None, None, None, None, 0) == E_INVALID
    path = str(tmp_path / "never_written.film").encode()
    assert L.mi355rt_film_save(None, path) == E_INVALID and not os.path.exists(path)
    assert L.mi355rt_film_save(None, None) == E_INVALID
    assert L.mi355rt_film_load(None, path, 0) == E_INVALID
    assert L.mi355rt_film_load(None, None, 1) == E_INVALID
    out = (C.c_uint32 * 8)(*([7] * 8))
    assert L.mi355rt_film_file_info(None, out) == E_INVALID
    assert L.mi355rt_film_file_info(path, None) == E_INVALID
    assert L.mi355rt_film_file_info(path, out) == E_LOAD              # no such file
    assert b"cannot open" in L.mi355rt_last_error(None)
    assert list(out) == [7] * 8


@pytest.mark.parametrize("direct", [False, True])
def test_write_then_read_round_trips_bit_for_bit(fio, tmp_path, direct):
    w, h = 7, 5
    s, q, n, d = random_film(w, h, 1, direct)
    path = tmp_path / "f.film"
    fio.write(path, w, h, n, s, q, d, seed=(5 << 32) | 17, flags=129)
    assert os.path.getsize(path) == 64 + w * h * (40 if direct else 28)
    raw = path.read_bytes()
    assert raw[:8] == b"MI355FLM" and struct.unpack_from("<IIIIQI", raw, 8) == (1, w, h, 1 if direct else 0, (5 << 32) | 17, 129)
    assert raw[36:64] == bytes(28)
    assert raw[64:64 + 4 * w * h] == n.astype("<u4").tobytes()       # the planes in the documented order: n, sum, sumsq, direct
    assert raw[64 + 4 * w * h:64 + 16 * w * h] == s.astype("<f4").tobytes()
    f = fio.read(path)
    assert (f["width"], f["height"], f["seed"], f["flags"]) == (w, h, (5 << 32) | 17, 129)
    assert np.array_equal(f["n"], n) and f["n"].dtype == np.uint32
    assert np.array_equal(bits(f["sum"]), bits(s)) and np.array_equal(bits(f["sumsq"]), bits(q))
    assert (f["direct"] is None) == (not direct)
    if direct:
        assert np.array_equal(bits(f["direct"]), bits(d))
    assert fio.info(path) == dict(version=1, width=w, height=h, planes=1 if direct else 0, seed=(5 << 32) | 17, flags=129)


def test_write_checks_its_planes(fio, tmp_path):
    s, q, n, d = random_film(4, 3, 2)
    with pytest.raises(ValueError):
        fio.write(tmp_path / "x", 4, 3, n[:-1], s, q)
    with pytest.raises(ValueError):
        fio.write(tmp_path / "x", 4, 3, n, s.astype(np.float64), q)
    with pytest.raises(ValueError):
        fio.write(tmp_path / "x", 0, 3, n, s, q)
    assert not (tmp_path / "x").exists()


def test_merge_is_the_f32_sum_in_argument_order(fio):
    w, h = 6, 4
    films = []
    for k in range(3):
        s, q, n, d = random_film(w, h, 10 + k)
        films.append(fio.film(w, h, n, s, q, d, seed=k, flags=k))
    m = fio.merge(*films)
    zero = np.zeros((w * h, 3), np.float32)
    with np.errstate(all="ignore"):
        for k in ("sum", "sumsq", "direct"):
            want = ((zero + films[0][k]) + films[1][k]) + films[2][k]
            assert np.array_equal(bits(m[k]), bits(want)), k
        other = ((zero + films[2]["sum"]) + films[1]["sum"]) + films[0]["sum"]
    assert not np.array_equal(bits(m["sum"]), bits(other))            # 72 values of like magnitude: the order of the additions shows in the bits
    assert np.array_equal(bits(fio.merge(*films[::-1])["sum"]), bits(other))
    assert np.array_equal(m["n"], films[0]["n"] + films[1]["n"] + films[2]["n"]) and m["n"].dtype == np.uint32
    assert m["n"][4] == (3 * 0xFFFFFFF0) & 0xFFFFFFFF                 # u32, wrapping
    assert (m["seed"], m["flags"]) == (0, 0)
    assert bits(m["sum"])[1, 1] != 0x80000000                         # 0 + -0.0 = +0.0 and so on: an ADD, as the device does it
    one = fio.merge(films[1])
    ok = ~np.isnan(films[1]["sum"]) & (bits(films[1]["sum"]) != 0x80000000)
    assert np.array_equal(bits(one["sum"])[ok], bits(films[1]["sum"])[ok])
    # a film without a direct plane: the merge has none
    s, q, n, _ = random_film(w, h, 20, direct=False)
    assert fio.merge(films[0], fio.film(w, h, n, s, q))["direct"] is None
    s2, q2, n2, _ = random_film(w, h + 1, 21, direct=False)
    with pytest.raises(ValueError):
        fio.merge(films[0], fio.film(w, h + 1, n2, s2, q2))
    with pytest.raises(ValueError):
        fio.merge()


def malformed_files(fio, tmp_path):
    """(name, path, word the reason must contain) of one good file's corruptions"""
    w, h = 5, 4
    s, q, n, d = random_film(w, h, 3)
    good = tmp_path / "good.film"
    fio.write(good, w, h, n, s, q, d, seed=9, flags=1)
    raw = good.read_bytes()

    def variant(name, data):
        p = tmp_path / (name + ".film")
        p.write_bytes(data)
        return p
    head = lambda **kw: struct.pack("<8sIIIIQI", kw.get("magic", b"MI355FLM"), kw.get("version", 1), kw.get("w", w), kw.get("h", h),   # noqa: E731
                                    kw.get("planes", 1), 9, 1) + bytes(28)
    return good, [
        ("bad_magic", variant("bad_magic", head(magic=b"MI355FLX") + raw[64:]), "magic"),
        ("bad_version", variant("bad_version", head(version=2) + raw[64:]), "version"),
        ("truncated", variant("truncated", raw[:-1]), "length"),
        ("too_long", variant("too_long", raw + b"\0"), "length"),
        ("short_header", variant("short_header", raw[:40]), "length"),
        ("empty", variant("empty", b""), "length"),
        ("planes_bit_without_plane", variant("planes_bit_without_plane", raw[:64 + 28 * w * h]), "length"),
        ("plane_without_planes_bit", variant("plane_without_planes_bit", head(planes=0) + raw[64:]), "length"),
        ("unknown_planes_bits", variant("unknown_planes_bits", head(planes=3) + raw[64:]), "planes"),
        ("other_size", variant("other_size", head(w=w + 1) + raw[64:]), "length"),
        ("zero_size", variant("zero_size", head(w=0)), "non-zero"),
    ]


def test_film_io_rejects_every_malformed_file(fio, tmp_path):
    good, bad = malformed_files(fio, tmp_path)
    fio.info(good); fio.read(good)
    for name, path, word in bad:
        for fn in (fio.info, fio.read):
            with pytest.raises(fio.FilmFileError, match=word):
                fn(path)
    with pytest.raises(OSError):
        fio.info(tmp_path / "absent.film")


def test_library_file_info_agrees_with_film_io(pkg, fio, tmp_path):
    good, bad = malformed_files(fio, tmp_path)
    assert pkg.film_file_info(good) == fio.info(good) == dict(version=1, width=5, height=4, planes=1, seed=9, flags=1)
    s, q, n, _ = random_film(9, 2, 4, direct=False)
    other = tmp_path / "other.film"
    fio.write(other, 9, 2, n, s, q, seed=(3 << 32) | 1, flags=32)
    assert pkg.film_file_info(other) == fio.info(other) == dict(version=1, width=9, height=2, planes=0, seed=(3 << 32) | 1, flags=32)
    L = pkg.lib()
    for name, path, word in bad:
        out = (C.c_uint32 * 8)(*([7] * 8))
        assert L.mi355rt_film_file_info(os.fsencode(path), out) == E_LOAD, name
        reason = L.mi355rt_last_error(None).decode()
        assert word in reason and str(path) in reason, (name, reason)
        assert list(out) == [7] * 8
        with pytest.raises(RuntimeError, match=word):
            pkg.film_file_info(path)
