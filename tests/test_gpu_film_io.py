"""Film set / add / save / load on the device (include/mi355rt.h): a film that is put back is a complete checkpoint -- a render
continued from it equals the uninterrupted one and the CPU oracle bit for bit, through arrays and through files; add is the f32 sum numpy
computes; the films of striped ranks reassemble into the unstriped film, which the denoiser then serves; only owned rows are written, on
stripes and on device groups; disjoint sample ranges of one seed merge to within the rounding of their association; the calls settle
queued and speculative work first and change nothing but the film; every misuse is refused with the film untouched; the CLI."""
import ctypes as C
import importlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
E_INVALID, E_LOAD = -1, -3


@pytest.fixture(scope="module")
def fio(pkg):
    return importlib.import_module("raytracer_rs_amd.film_io")


@pytest.fixture(scope="module")
def dn(pkg):
    return importlib.import_module("raytracer_rs_amd.denoise")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(pkg, scenes, name, w, h, flags=0, direct=False, **kw):
    rt = pkg.create_raytracer_from_arrays(scenes(name), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h,
                                          flags=flags | (pkg.FLAG_DIRECT_FILM if direct else 0), **kw)
    rt.has_direct = direct
    return rt


def film_of(fio, rt):
    """the handle's film as a film_io dict (copies)"""
    s, q, n = rt.film.pixel_datas()
    return fio.film(rt.width, rt.height, n, s, q, rt.film.direct_sums() if rt.has_direct else None)


def put(rt, f, add=False):
    (rt.film.add if add else rt.film.set)(f["sum"], f["sumsq"], f["n"], f["direct"] if rt.has_direct else None)


def assert_same_film(a, b, direct=True):
    assert np.array_equal(a["n"], b["n"])
    assert np.array_equal(bits(a["sum"]), bits(b["sum"])) and np.array_equal(bits(a["sumsq"]), bits(b["sumsq"]))
    if direct and a["direct"] is not None:
        assert b["direct"] is not None and np.array_equal(bits(a["direct"]), bits(b["direct"]))


def random_film(fio, w, h, seed, direct):
    rng = np.random.default_rng(seed)
    npix = w * h
    return fio.film(w, h, rng.integers(1, 9, npix).astype(np.uint32), rng.random((npix, 3), np.float32) * 5, rng.random((npix, 3), np.float32) * 25,
                    rng.random((npix, 3), np.float32) if direct else None)


# ---- 1. resume is exact -------------------------------------------------------------------------------------------------------------
SEED = 5
_CONTINUOUS = {}


def continuous(pkg, fio, scenes, oracle, name, w, h, sem, fix_row, direct):
    """(film, packed pixels) of ONE handle after render(3) then render(5), checked against the oracle's 8-spp film; computed once per
    configuration and shared, never modified"""
    key = (name, w, h, sem.name, fix_row, direct)
    if key not in _CONTINUOUS:
        a = make(pkg, scenes, name, w, h, flags=sem.gpu | (pkg.FLAG_FIX_ROW_INDEX if fix_row else 0), direct=direct, seed=SEED)
        a.render(3); a.render(5)
        fa = film_of(fio, a)
        orc = oracle.Oracle(scenes(name), w, h, seed=SEED, flags=sem.orc | (oracle.FLAG_FIX_ROW_INDEX if fix_row else 0))
        orc.render(8, nthreads=8)
        os_, oq, on = orc.film()
        assert np.array_equal(fa["n"], on) and np.array_equal(bits(fa["sum"]), bits(os_)) and np.array_equal(bits(fa["sumsq"]), bits(oq))
        for v in fa.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CONTINUOUS[key] = (fa, a.get_tonemapped_pixels().copy())
    return _CONTINUOUS[key]


@pytest.mark.parametrize("via", ["arrays", "file"])
@pytest.mark.parametrize("direct", [False, True])
def test_resume_is_exact(pkg, fio, scenes, oracle, sem, tmp_path, direct, via):
    name, w, h = ("ico3_tex", 33, 27) if direct else ("ico2", 37, 30)
    for fix_row in (False, True):
        flags = sem.gpu | (pkg.FLAG_FIX_ROW_INDEX if fix_row else 0)
        want, want_px = continuous(pkg, fio, scenes, oracle, name, w, h, sem, fix_row, direct)
        b = make(pkg, scenes, name, w, h, flags=flags, direct=direct, seed=SEED)
        b.render(3)
        c = make(pkg, scenes, name, w, h, flags=flags, direct=direct, seed=SEED)
        if via == "arrays":
            put(c, film_of(fio, b))
        else:
            path = tmp_path / ("resume_%d.film" % fix_row)
            b.film.save(path)
            assert pkg.film_file_info(path) == dict(version=1, width=w, height=h, planes=1 if direct else 0, seed=SEED,
                                                    flags=flags | (pkg.FLAG_DIRECT_FILM if direct else 0))
            c.film.load(path)
        b.close()
        c.render(5)
        got = film_of(fio, c)
        assert_same_film(want, got)
        assert int(got["n"].min()) == int(got["n"].max()) == 8 and (not direct or got["direct"].any())
        assert np.array_equal(c.get_tonemapped_pixels(), want_px)


def test_resume_is_exact_on_the_large_scene(pkg, fio, scenes, oracle, sem):
    name, w, h = "thai2", 64, 48
    want, want_px = continuous(pkg, fio, scenes, oracle, name, w, h, sem, False, True)
    b = make(pkg, scenes, name, w, h, flags=sem.gpu, direct=True, seed=SEED)
    b.render(3)
    c = make(pkg, scenes, name, w, h, flags=sem.gpu, direct=True, seed=SEED)
    put(c, film_of(fio, b))
    c.render(5)
    assert_same_film(want, film_of(fio, c))
    assert np.array_equal(c.get_tonemapped_pixels(), want_px)


# ---- 2. add equals numpy, set returns the input's bits ----------------------------------------------------------------------------------
def test_add_equals_numpy_and_set_keeps_the_bits(pkg, fio, scenes):
    name, w, h = "thai2", 64, 48
    a = make(pkg, scenes, name, w, h, direct=True, seed=3); a.render(3)
    b = make(pkg, scenes, name, w, h, direct=True, seed=4); b.render(4)
    fa, fb = film_of(fio, a), film_of(fio, b)
    assert not np.array_equal(bits(fa["sum"]), bits(fb["sum"]))
    t = make(pkg, scenes, name, w, h, direct=True, seed=1)
    put(t, fa, add=True); put(t, fb, add=True)
    m = fio.merge(fa, fb)
    assert_same_film(m, film_of(fio, t))
    assert int(m["n"].max()) == 7 and m["direct"].any()
    # onto a rendered film: the handle's value on the left
    put(a, fb, add=True)
    want = fio.film(w, h, fa["n"] + fb["n"], fa["sum"] + fb["sum"], fa["sumsq"] + fb["sumsq"], fa["direct"] + fb["direct"])
    assert_same_film(want, film_of(fio, a))
    # set: the bits as they are -- a NaN's payload, the sign of -0.0, an infinity, a denormal, any count
    x = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fa.items()}
    x["sum"].view(np.uint32)[5, 1] = 0x7FC12345; x["sum"][6, 0] = -0.0; x["sumsq"].view(np.uint32)[7, 2] = 0xFFA00001
    x["sumsq"][8, 0] = np.inf; x["direct"].view(np.uint32)[9, 1] = 1; x["direct"][10, 2] = -0.0; x["n"][11] = 0xFFFFFFFF; x["n"][12] = 0
    put(t, x)
    assert_same_film(x, film_of(fio, t))
    assert bits(film_of(fio, t)["sum"])[6, 0] == 0x80000000


# ---- 3. stripes reassemble, and the result denoises ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,direct", [("ico2", 37, 30, False), ("thai2", 64, 48, True)])
def test_stripes_reassemble_into_the_unstriped_film(pkg, fio, scenes, name, w, h, direct):
    u = make(pkg, scenes, name, w, h, direct=direct, seed=6); u.render(4)
    t = make(pkg, scenes, name, w, h, direct=direct, seed=6)
    rows = []
    for rank in (0, 1):
        r = make(pkg, scenes, name, w, h, direct=direct, seed=6, stripe_rows=4, stripe_rank=rank, stripe_world=2)
        r.render(4)
        f = film_of(fio, r)
        rows.append(set(r.owned_rows().tolist()))
        assert not f["n"].reshape(h, w)[sorted(set(range(h)) - rows[-1])].any()     # zero on the rows it does not own
        put(t, f, add=True)
    assert rows[0] | rows[1] == set(range(h)) and not rows[0] & rows[1]
    assert h % 8 == 0 or len(rows[0]) != len(rows[1])                 # 37 x 30: the last stripe is partial
    assert_same_film(film_of(fio, u), film_of(fio, t))
    assert np.array_equal(t.get_tonemapped_pixels(), u.get_tonemapped_pixels())
    for split in ([False, True] if direct else [False]):
        (rgb_t, px_t), (rgb_u, px_u) = t.get_denoised_pixels(split=split), u.get_denoised_pixels(split=split)
        assert np.array_equal(bits(rgb_t), bits(rgb_u)) and np.array_equal(px_t, px_u)
        assert not np.array_equal(px_t, u.get_tonemapped_pixels())


# ---- 4. ownership -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [False, True])
def test_a_striped_handle_writes_owned_rows_only(pkg, fio, scenes, direct):
    name, w, h = "ico2", 37, 30
    rt = make(pkg, scenes, name, w, h, direct=direct, seed=7, stripe_rows=4, stripe_rank=1, stripe_world=2)
    own = np.zeros(h, bool); own[rt.owned_rows()] = True
    assert own.any() and not own.all()
    mask = np.repeat(own, w)
    x = random_film(fio, w, h, 1, direct)
    put(rt, x)
    got = film_of(fio, rt)
    keys = ("sum", "sumsq", "n") + (("direct",) if direct else ())
    for k in keys:
        assert np.array_equal(got[k][mask], x[k][mask]) and not got[k][~mask].any(), k
    put(rt, x, add=True)
    got = film_of(fio, rt)
    for k in keys:
        assert np.array_equal(got[k][mask], (x[k] + x[k])[mask]) and not got[k][~mask].any(), k
    assert np.array_equal(rt.get_tonemapped_pixels().reshape(h, w)[own], pkg_pack(x, 2)[own])
    rt.film.clear()
    assert not any(film_of(fio, rt)[k].any() for k in keys)


def pkg_pack(f, times):
    """tone-mapped pixels of the film f added to itself `times` times over (every sum doubles exactly, so does n)"""
    dn = importlib.import_module("raytracer_rs_amd.denoise")
    t = np.float32(times)
    return dn.pack(dn.film_inputs(f["sum"] * t, f["sumsq"] * t, f["n"] * np.uint32(times))[0]).reshape(f["height"], f["width"])


def test_a_device_group_round_trips_and_continues(pkg, fio, scenes, oracle, sem):
    name, w, h = "ico2", 37, 30
    want, want_px = continuous(pkg, fio, scenes, oracle, name, w, h, sem, False, False)
    single = make(pkg, scenes, name, w, h, flags=sem.gpu, seed=SEED); single.render(3)
    f3 = film_of(fio, single)
    g = make(pkg, scenes, name, w, h, flags=sem.gpu | pkg.FLAG_GROUP_SHARES_DEVICE, seed=SEED, device_count=2)
    assert g.device_count == 2
    hbm = g.hbm_allocated_bytes()
    put(g, f3)
    assert g.hbm_allocated_bytes() == hbm
    assert_same_film(f3, film_of(fio, g))
    g.render(5)
    assert_same_film(want, film_of(fio, g))
    assert np.array_equal(g.get_tonemapped_pixels(), want_px)
    put(g, f3, add=True)
    assert_same_film(fio.film(w, h, want["n"] + f3["n"], want["sum"] + f3["sum"], want["sumsq"] + f3["sumsq"]), film_of(fio, g))


# ---- 5. disjoint sample ranges of one seed ---------------------------------------------------------------------------------------------
def test_sample_ranges_of_one_seed_merge(pkg, fio, scenes):
    """A renders samples 0..7; C renders 0..3; B is told its pixels hold 4 samples already (zero sums, n = 4) and renders 4 more: samples
    4..7.  merge(C, B with its offset taken off n) holds the same 8 terms per value as A in another association, (x0+..+x3) + (x4+..+x7)
    against ((x0+x1)+..)+x7.  The terms are non-negative, so each sum carries at most 7 roundings of 2^-24 relative error:
    |a - b| <= 14 * 2^-24 * max(a, b) < 2^-20 * max(a, b).  The bound is derived, not measured."""
    name, w, h = "thai2", 64, 48
    a = make(pkg, scenes, name, w, h, direct=True, seed=8); a.render(8)
    c = make(pkg, scenes, name, w, h, direct=True, seed=8); c.render(4)
    b = make(pkg, scenes, name, w, h, direct=True, seed=8)
    z = np.zeros((w * h, 3), np.float32)
    b.film.set(z, z, np.full(w * h, 4, np.uint32), z)
    b.render(4)
    fa, fb, fc = film_of(fio, a), film_of(fio, b), film_of(fio, c)
    assert (fb["n"] == 8).all()
    fb["n"] = fb["n"] - np.uint32(4)
    m = fio.merge(fc, fb)
    assert np.array_equal(m["n"], fa["n"])
    for k in ("sum", "sumsq", "direct"):
        x, y = fa[k].astype(np.float64), m[k].astype(np.float64)
        assert (x >= 0).all() and (y >= 0).all()
        err = np.abs(x - y); bound = 2.0 ** -20 * np.maximum(x, y)
        print("%s: max |a-b| / max(a,b) = %.3g (bound %.3g)" % (k, float(np.max(err / np.maximum(np.maximum(x, y), 1e-300))), 2.0 ** -20))
        assert (err <= bound).all(), k
    assert not np.array_equal(bits(fb["sum"]), bits(fc["sum"]))       # B rendered other samples than C
    assert fa["sum"].any()


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,speculates", [(70, False), (120, True)])
def test_add_right_behind_the_drop_in_loop(pkg, fio, scenes, h, speculates):
    """h = 70: every second 50-row frame wraps (two windows share rows, so the library launches no frame ahead).  h = 120: a speculative
    frame IS out when film_add arrives; its rows must be given back before the film is written."""
    name, w = "thai2", 32
    src = make(pkg, scenes, name, w, h, direct=True, seed=9); src.render(2)
    f = film_of(fio, src)
    hh = make(pkg, scenes, name, w, h, direct=True, seed=10)
    tt = make(pkg, scenes, name, w, h, direct=True, seed=10)
    for rt in (hh, tt):
        for _ in range(3):
            rt.trace_frame_additive(); rt.get_tonemapped_pixels()
    launched, adopted = hh.debug_speculation()
    assert (launched >= 2 and adopted >= 1) if speculates else launched == 0
    if speculates:                                                    # a frame IS out right now: a handle that just goes on takes it over
        ctl = make(pkg, scenes, name, w, h, direct=True, seed=10)
        for _ in range(4):
            ctl.trace_frame_additive(); ctl.get_tonemapped_pixels()
        assert ctl.debug_speculation() == (launched + 1, adopted + 1)
    put(hh, f, add=True)                                              # at once
    before = film_of(fio, tt)                                         # reading the film settles the speculation
    put(tt, f, add=True)
    assert hh.debug_speculation() == (launched, adopted)              # given back, not taken over
    mid = film_of(fio, tt)
    assert_same_film(fio.film(w, h, before["n"] + f["n"], before["sum"] + f["sum"], before["sumsq"] + f["sumsq"], before["direct"] + f["direct"]), mid)
    assert hh.current_row == tt.current_row == 150 % h
    assert hh.trace_frame_additive() == tt.trace_frame_additive()
    if speculates:                                                    # ... whereas this call rendered its frame itself (and launched the next one)
        assert hh.debug_speculation() == tt.debug_speculation() == (launched + 1, adopted)
    fh, ft = film_of(fio, hh), film_of(fio, tt)
    assert_same_film(ft, fh)
    assert not np.array_equal(ft["n"], mid["n"])
    assert np.array_equal(hh.get_tonemapped_pixels(), tt.get_tonemapped_pixels())


def test_set_and_add_are_ordered_behind_a_queued_frame(pkg, fio, scenes):
    name, w, h = "thai2", 64, 48
    f = random_film(fio, w, h, 2, False)
    a = make(pkg, scenes, name, w, h, seed=11)
    a.render(2, wait=False)
    put(a, f)                                                         # the queued frame must not land on top of it
    assert_same_film(f, film_of(fio, a))
    assert a.last_counts().primary == 2 * w * h                       # the queued call's counters are still there
    b = make(pkg, scenes, name, w, h, seed=11); b.render(2)
    fb = film_of(fio, b)
    c = make(pkg, scenes, name, w, h, seed=11)
    c.render(2, wait=False)
    put(c, f, add=True)
    assert_same_film(fio.film(w, h, fb["n"] + f["n"], fb["sum"] + f["sum"], fb["sumsq"] + f["sumsq"]), film_of(fio, c))


def test_nothing_but_the_film_changes(pkg, fio, scenes, tmp_path):
    name, w, h = "thai2", 32, 70
    src = make(pkg, scenes, name, w, h, direct=True, seed=12); src.render(3)
    f, src_px = film_of(fio, src), src.get_tonemapped_pixels().copy()
    path = tmp_path / "f.film"
    src.film.save(path)
    rt = make(pkg, scenes, name, w, h, direct=True, seed=13)
    rt.camera.move_rel(0.1, 0.0, 0.05)
    rt.trace_frame_additive()
    px0 = rt.get_tonemapped_pixels().copy()
    rt.get_denoised_pixels()                                          # the guides and the filter's buffers are allocated now
    counts = rt.last_counts().as_dict()

    def state():
        return (rt.current_row, rt.last_counts().as_dict(), [m.tolist() for m in rt.camera.matrices()], rt.hbm_allocated_bytes(),
                bits(rt.guides()["depth"]).tolist())
    s0 = state()
    assert s0[0] == 50 and s0[1] == counts and counts["primary"] == 50 * w
    put(rt, f)
    assert state() == s0
    px1 = rt.get_tonemapped_pixels().copy()                           # every row is dirty: the cache shows the new film
    assert np.array_equal(px1, src_px) and not np.array_equal(px1, px0)
    put(rt, f, add=True)
    assert state() == s0
    assert np.array_equal(rt.get_tonemapped_pixels(), src_px)         # twice the sums over twice the samples: the same means
    rt.film.load(path)
    assert state() == s0
    assert_same_film(f, film_of(fio, rt))
    rt.film.load(path, add=True)
    assert state() == s0
    assert_same_film(fio.merge(f, f), film_of(fio, rt))
    rt.film.save(tmp_path / "g.film")
    assert state() == s0
    assert_same_film(fio.merge(f, f), fio.read(tmp_path / "g.film"))


def test_adaptive_sampling_continues_from_a_restored_film(pkg, fio, scenes):
    name, w, h = "thai2", 64, 48
    cfg = dict(min_spp=4, max_spp=16, batch_spp=3, max_rounds=0, rel_error=0.1, abs_floor=0.03)
    p = make(pkg, scenes, name, w, h, direct=True, seed=14); p.render(4)
    f4 = film_of(fio, p)
    st_p = p.render_adaptive(**cfg)
    r = make(pkg, scenes, name, w, h, direct=True, seed=14)
    put(r, f4)
    st_r = r.render_adaptive(**cfg)
    assert st_r == st_p and st_p["rounds"] >= 2
    fp = film_of(fio, p)
    assert_same_film(fp, film_of(fio, r))
    assert len(np.unique(fp["n"])) > 1


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------------
def fptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def uptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))


def last_error(pkg, rt):
    return pkg.lib().mi355rt_last_error(rt._h).decode()


def test_misuse_is_refused_and_the_film_is_untouched(pkg, fio, scenes, tmp_path):
    name, w, h = "ico2", 37, 30
    npix = w * h
    L = pkg.lib()
    plain = make(pkg, scenes, name, w, h, seed=15); plain.render(2)
    flagged = make(pkg, scenes, name, w, h, direct=True, seed=15); flagged.render(2)
    x = random_film(fio, w, h, 3, True)
    s, q, n, d = x["sum"], x["sumsq"], x["n"], x["direct"]
    for rt in (plain, flagged):
        f0 = film_of(fio, rt)
        dd = d if rt.has_direct else None
        calls = [("npix", (s, q, n, dd, npix - 1)), ("npix", (s, q, n, dd, npix + 1)), ("npix", (s, q, n, dd, 0)),
                 ("sum_rgb", (None, q, n, dd, npix)), ("sumsq_rgb", (s, None, n, dd, npix)), ("n is", (s, q, None, dd, npix)),
                 ("direct_rgb", (s, q, n, None if rt.has_direct else d, npix))]
        for fn_name in ("mi355rt_film_set", "mi355rt_film_add"):
            for word, (a, b, c, e, k) in calls:
                assert getattr(L, fn_name)(rt._h, fptr(a), fptr(b), uptr(c), fptr(e), k) == E_INVALID, (fn_name, word)
                msg = last_error(pkg, rt)
                assert word in msg and fn_name in msg, msg
                assert_same_film(f0, film_of(fio, rt))
        with pytest.raises(RuntimeError, match="direct_rgb"):
            rt.film.set(s, q, n, None if rt.has_direct else d)
        # files
        good = tmp_path / "good.film"
        fio.write(good, w, h, n, s, q, d, seed=1, flags=0)
        raw = good.read_bytes()
        files = {"length_short": raw[:-4], "length_long": raw + bytes(4), "magic": b"X" + raw[1:], "version": raw[:8] + struct.pack("<I", 2) + raw[12:]}
        for word, data in files.items():
            p = tmp_path / (word + ".film"); p.write_bytes(data)
            files[word] = p
        other = tmp_path / "width.film"
        xo = random_film(fio, w + 1, h, 4, True)
        fio.write(other, w + 1, h, xo["n"], xo["sum"], xo["sumsq"], xo["direct"])
        files["width"] = other
        tall = tmp_path / "height.film"
        xt = random_film(fio, w, h - 1, 5, True)
        fio.write(tall, w, h - 1, xt["n"], xt["sum"], xt["sumsq"], xt["direct"])
        files["height"] = tall
        fix = tmp_path / "FIX_ROW_INDEX.film"
        fio.write(fix, w, h, n, s, q, d, flags=pkg.FLAG_FIX_ROW_INDEX)
        files["FIX_ROW_INDEX"] = fix
        files["cannot open"] = tmp_path / "absent.film"
        if rt.has_direct:
            nod = tmp_path / "direct.film"
            fio.write(nod, w, h, n, s, q)
            files["direct plane"] = nod
        for word, p in files.items():
            for add in (0, 1):
                assert L.mi355rt_film_load(rt._h, os.fsencode(p), add) == E_LOAD, word
                assert word.split("_")[0] in last_error(pkg, rt) and "mi355rt_film_load" in last_error(pkg, rt), (word, last_error(pkg, rt))
                assert_same_film(f0, film_of(fio, rt))
        with pytest.raises(RuntimeError, match="length"):
            rt.film.load(files["length_short"])
        assert L.mi355rt_film_load(rt._h, None, 0) == E_INVALID and L.mi355rt_film_save(rt._h, None) == E_INVALID
        assert L.mi355rt_film_save(rt._h, os.fsencode(tmp_path / "no_such_dir" / "f.film")) == E_LOAD and "cannot write" in last_error(pkg, rt)
        assert_same_film(f0, film_of(fio, rt))
        # the FIX_ROW_INDEX check follows the handle's CURRENT flag
        rt.set_flags(pkg.FLAG_FIX_ROW_INDEX | (pkg.FLAG_DIRECT_FILM if rt.has_direct else 0))
        assert L.mi355rt_film_load(rt._h, os.fsencode(good), 0) == E_LOAD and "FIX_ROW_INDEX" in last_error(pkg, rt)
        rt.film.load(fix)
        assert_same_film(x, film_of(fio, rt), direct=rt.has_direct)
    # a file WITH a direct plane loads into a handle without the flag (above: `plain` took fix, which has one); one without loads too
    fio.write(tmp_path / "nod.film", w, h, n, q, s, flags=pkg.FLAG_FIX_ROW_INDEX)
    plain.film.load(tmp_path / "nod.film")
    assert_same_film(fio.film(w, h, n, q, s), film_of(fio, plain))


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------------------------
def read_png_rgb(data):
    """the pixels (uint8[npix, 3]) of an 8-bit RGB PNG whose scanlines all use filter type 0, as the CLI writes them"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            size = struct.unpack(">II", body[:8]); assert body[8:10] == b"\x08\x02"
        if kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h = size
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return (w, h), raw[:, 1:].reshape(-1, 3)


def rgb_of(px):
    return np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], axis=1).astype(np.uint8)


def test_cli_saves_loads_and_merges_films(pkg, fio, dn, scenes, tmp_path):
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    w, h = 64, 48
    base = [exe, "-f", os.path.join(SCENES, "thai2.scene"), "--width", str(w), "--height", str(h), "--seed", "17"]

    def run(*args):
        r = subprocess.run(base + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r
    fa, fb = tmp_path / "a.film", tmp_path / "b.film"
    run("--spp", 3, "--save-film", fa)
    rt = make(pkg, scenes, "thai2", w, h, seed=17)
    rt.render(3)
    a = fio.read(fa)                                                  # a file the CLI wrote reads in film_io
    assert_same_film(film_of(fio, rt), a)
    assert a["direct"] is None and (a["seed"], a["flags"]) == (17, 0)
    # resume: 3 samples from the file, 5 more
    run("--load-film", fa, "--spp", 5, "--out", tmp_path / "a.png")
    rt.render(5)
    size, rgb = read_png_rgb((tmp_path / "a.png").read_bytes())
    assert size == (w, h) and np.array_equal(rgb, rgb_of(rt.get_tonemapped_pixels()))
    # merge only: a file film_io wrote (another seed's film) joins the CLI's
    other = make(pkg, scenes, "thai2", w, h, seed=18); other.render(2)
    b = film_of(fio, other)
    fio.write(fb, w, h, b["n"], b["sum"], b["sumsq"], seed=18)
    r = run("--load-film", fa, "--load-film", fb, "-i", 0, "--out", tmp_path / "x.png", "--save-film", tmp_path / "m.film")
    assert "frame:" not in r.stdout                                   # nothing was rendered
    m = fio.merge(a, b)
    size, rgb = read_png_rgb((tmp_path / "x.png").read_bytes())
    assert size == (w, h) and np.array_equal(rgb, rgb_of(dn.pack(dn.film_inputs(m["sum"], m["sumsq"], m["n"])[0])))
    assert_same_film(m, fio.read(tmp_path / "m.film"))
    # a file that does not fit is an error, not an image
    r = subprocess.run(base[:3] + ["--width", str(w + 1), "--height", str(h), "--load-film", str(fa), "-i", "0", "--out", str(tmp_path / "bad.png")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "width" in r.stderr and not (tmp_path / "bad.png").exists()
