"""Every film read-out on hand-made films no render produces (include/mi355rt.h: "The values are data: they are not validated").

mi355rt_film_set / _add / _load put any (n, sum, sumsq, direct) in front of the kernels that read the film: the tone-mapper, the mean and the
variance, the adaptive verdict, the denoiser (plain and split) and film add itself.  A render only ever makes small n, non-negative finite sums
and sumsq >= sum^2 / n; edge_film() below makes the rest: n = 0, n = 1, negative variance, n where the reference's u32 product n * (n - 1) wraps,
n that rounds in f32, n with the sign bit set, denormals, -0.0, negative sums, a mean of exactly -1, overflowing products, and (kind
"nonfinite") NaNs of two payloads and both infinities -- at image shapes from 1 x 1 over single rows and columns to just around the 64 x 4
denoise block and the 8 x 8 adaptive tile.  isolated_film() puts each catalogue pixel alone into an adaptive tile of settled pixels, so that
the tile's verdict is that pixel's.

ONE RULE for every comparison (same()): no tolerance.  An f32 the expectation holds as a non-NaN must come back bit for bit; where the
expectation is NaN the result must be NaN, its bits are not compared (the sign and payload of a NaN born of an invalid operation, or carried
through an addition, differ between an x86 host and the device, and are not in the header's contract).  Integers compare with array_equal.

CPU tests (a-c) pin the statements themselves: the oracle (given the film through oracle_film_set) against an independent per-operation float64
statement, the conditions that keep the GPU tests from being vacuous (asserted on the numpy statements, never on the library), and the film
file round trip.  GPU tests (d-h) compare the library with those statements.  Nothing here renders; that is also why no test asks
debug_check_guards() for anything (assert_only_read)."""
import functools
import importlib

import numpy as np
import pytest

gpu = pytest.mark.gpu
F = np.float32
MISS = 0xFFFFFFFF
SHAPES = [(1, 1), (1, 9), (9, 1), (8, 8), (63, 3), (64, 4), (65, 5), (129, 2), (67, 13)]
KINDS = ["finite", "nonfinite"]
BIG = (67, 13)                                                        # more than one denoise block and adaptive tile each way, both clipped
PARAMS = [dict(normal_power_log2=7, sigma_luminance=1.0, sigma_depth=0.1, sigma_albedo=0.1),          # = tests/test_gpu_denoise.py::PARAMS
          dict(normal_power_log2=0, sigma_luminance=0.5, sigma_depth=1.0, sigma_albedo=2.0),
          dict(normal_power_log2=10, sigma_luminance=40.0, sigma_depth=0.01, sigma_albedo=0.02)]
SCENE = "ico2"

# (n, sum, sumsq) per channel.  Nothing here makes the mean of a pixel with n >= 1 non-finite.
CATALOGUE = [(0, 0.0, 0.0), (0, 1.5, 2.0),                            # empty pixels, one with sums left in it
             (1, 0.7, 0.49),                                          # unknown variance
             (2, 1.0, 0.4),                                           # negative variance: n q < s^2
             (65536, 3e4, 2e4), (65537, 3e4, 2e4),                    # n (n - 1) in u32: about to wrap, wrapped
             (1 << 24, 1e7, 1e7), ((1 << 24) + 1, 1e7, 1e7),          # (float)n rounds
             (0x80000000, 1e9, 1e9), (0xFFFFFFFF, 4e9, 5e9),          # the sign bit of n
             (3, 1e-40, 1e-44),                                       # denormals
             (3, -0.0, 0.0),                                          # negative zero
             (5, -2.0, 1.0),                                          # negative sums
             (4, -4.0, 4.0),                                          # a mean of exactly -1: c / (1 + c) divides by zero
             (4, 1e19, 3e38),                                         # fn * q overflows
             (7, 3e38, 3e38),
             (2, 1e-30, 0.0)]
REPEATS = 3
POISON = [0x7FC12345, 0xFFA00001, 0x7F800000, 0xFF800000]             # a quiet NaN, a signalling negative NaN with another payload, +inf, -inf
N_POISON = 12


# ---- the comparison rule -------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what=""):
    """THE comparison of this file (see the module text): exact; a NaN expectation asks for a NaN, any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if want.dtype != np.float32:
        assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8].tolist())
        return
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), (what, "NaN expected", np.argwhere(nan & ~np.isnan(got))[:8].tolist())
    bad = ~nan & (bits(got) != bits(want))
    assert not bad.any(), (what, np.argwhere(bad)[:8].tolist(), got[bad][:8].tolist(), want[bad][:8].tolist())


def same_film(got, want, what=""):
    for k in ("n", "sum", "sumsq") + (("direct",) if want["direct"] is not None else ()):
        same(got[k], want[k], what + " " + k)


def same_bits(got, want, what=""):
    """a film that was only stored: every bit, a NaN's payload included"""
    for k in ("n", "sum", "sumsq") + (("direct",) if want["direct"] is not None else ()):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)


# ---- the films -----------------------------------------------------------------------------------------------------------------------------
def _fio():
    return importlib.import_module("raytracer_rs_amd.film_io")


def _freeze(f):
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def background_film(w, h, direct, seed=1):
    """what a render could have made: n in 2..39, means in [0, 3), sumsq = 1.3 sum^2 / n (shared, read-only)"""
    return _freeze(_fio().film(w, h, *_background(w, h, direct, np.random.default_rng([seed, w, h]))))


def _background(w, h, direct, rng, n_range=(2, 40)):
    npix = w * h
    n = rng.integers(*n_range, npix).astype(np.uint32)
    s = (rng.random((npix, 3)) * 3.0 * n[:, None]).astype(np.float32)
    q = (1.3 * s.astype(np.float64) ** 2 / n[:, None]).astype(np.float32)
    d = (s * (rng.random((npix, 3)) * 0.9).astype(np.float32)).astype(np.float32)
    d[::7] = -0.0
    return n, s, q, (d if direct else None)


def _place(n, s, q, d, p, slot, seed):
    """pixel p becomes placement `slot` of the catalogue (see edge_film)"""
    ne = len(CATALOGUE)
    e, rep = (slot + 3 * seed) % ne, slot // ne
    n[p] = CATALOGUE[e][0]
    for ch, other in enumerate((e, (e + 5 * rep) % ne, (e + 11 * rep) % ne)):
        s[p, ch], q[p, ch] = CATALOGUE[other][1], CATALOGUE[other][2]
    how = slot % 4
    if n[p] == 0 or how == 1:
        d[p] = s[p] + F(0.5)                                          # larger than the sum; non-zero where n = 0
    elif how == 2:
        d[p] = s[p] * F(1.125)                                        # 3e38 * 1.125 is still finite
    elif how == 3:
        d[p] = -0.0
    else:
        d[p] = s[p] * F(0.25)


def poison_columns(w):
    return max(1, 3 * w // 10)


def nan_share_bound(w, iterations):
    """the largest share of an image's columns a poisoned value of edge_film() can reach in `iterations` iterations (steps 1, 2, 4, ..., two
    taps each way)"""
    return min(1.0, (poison_columns(w) + 2 * ((1 << iterations) - 1)) / w)


@functools.lru_cache(maxsize=None)
def edge_film(w, h, kind, direct, seed=1):
    """The film of the module text as a film_io.film dict (shared, read-only): a background with the catalogue scattered over it, every entry
    REPEATS times at seeded positions (an image too small for that is filled with the catalogue in order).  The first placement of an entry
    gives all three channels its (sum, sumsq); the later ones give green and blue those of two other entries under the entry's n.
    direct: a fraction of the sum on the background, -0.0 on every seventh pixel; on catalogue pixels in turn a fraction, more than the sum
    (a negative indirect part) two ways, and -0.0; non-zero on an n = 0 pixel.
    kind "nonfinite": the same film with N_POISON single values replaced by the POISON bit patterns, one per pixel, over all planes, at seeded
    pixels of the image's left three tenths (poison_columns): a value reaches 6 columns further in two iterations (2 + 4), so on an image
    of 30 columns or more every read-out keeps at least half of its pixels numbers."""
    assert kind in KINDS
    rng = np.random.default_rng([seed, w, h])
    npix, slots = w * h, len(CATALOGUE) * REPEATS
    n, s, q, d = _background(w, h, True, rng)
    where = rng.permutation(npix)[:slots] if npix > slots else np.arange(npix)
    for slot, p in enumerate(where.tolist()):
        _place(n, s, q, d, p, slot, seed)
    if kind == "nonfinite":
        prng = np.random.default_rng([seed, w, h, 99])
        planes = [s, q, d] if direct else [s, q]
        left = np.flatnonzero(np.arange(npix) % w < poison_columns(w))
        for i, p in enumerate(prng.permutation(left)[:N_POISON].tolist()):
            planes[i % len(planes)].view(np.uint32)[p, int(prng.integers(0, 3))] = POISON[(i // len(planes)) % 4]
    return _freeze(_fio().film(w, h, n, s, q, d if direct else None))


TILE = 8
ISOLATED = (TILE * len(CATALOGUE), TILE * REPEATS)


@functools.lru_cache(maxsize=None)
def isolated_film(seed=1):
    """For the adaptive verdict, where a tile of edge_film() is nearly always busy whatever one pixel says: ISOLATED is one tile per catalogue
    placement, the placement at a seeded pixel of its tile, all other pixels a background that every configuration of adaptive_cfgs() settles
    (n in 40..56; 0.3 s^2 <= 0.04 (n - 1) s^2) and that a batch of 8 takes to max_spp = 64 at the most.  A tile is busy exactly when its one
    catalogue pixel is not settled."""
    w, h = ISOLATED
    rng = np.random.default_rng([seed, w, h])
    n, s, q, d = _background(w, h, True, rng, n_range=(40, 57))
    for slot in range(len(CATALOGUE) * REPEATS):
        tx, ty = slot % len(CATALOGUE), slot // len(CATALOGUE)
        x, y = rng.integers(0, TILE, 2)
        _place(n, s, q, d, int((ty * TILE + y) * w + tx * TILE + x), slot, seed)
    return _freeze(_fio().film(w, h, n, s, q, d))


def test_the_builder_builds_what_the_module_text_says(pkg):
    f, g = edge_film(*BIG, "finite", True), edge_film(*BIG, "nonfinite", True)
    for e in CATALOGUE:
        hit = (f["n"] == e[0]) & (bits(f["sum"][:, 0]) == bits(F(e[1]))) & (bits(f["sumsq"][:, 0]) == bits(F(e[2])))
        assert hit.sum() >= REPEATS, e
        assert (hit & (bits(f["sum"][:, 1]) != bits(F(e[1])))).any(), e           # channels of one pixel from different entries
    assert np.isfinite(f["sum"]).all() and np.isfinite(f["sumsq"]).all() and np.isfinite(f["direct"]).all()
    with np.errstate(all="ignore"):
        ind = f["sum"] - f["direct"]
    assert (ind < 0).any() and (bits(f["direct"]) == 0x80000000).any() and f["direct"][f["n"] == 0].any()
    changed = [bits(f[k]) != bits(g[k]) for k in ("sum", "sumsq", "direct")]
    assert [int(c.sum()) for c in changed] == [4, 4, 4] and np.array_equal(f["n"], g["n"])
    assert (changed[0] | changed[1] | changed[2]).any(axis=1).sum() == N_POISON                  # one per pixel
    for k, c in zip(("sum", "sumsq", "direct"), changed):
        assert sorted(bits(g[k])[c].tolist()) == sorted(POISON), k
    assert [int((bits(edge_film(*BIG, "nonfinite", False)[k]) != bits(f[k])).sum()) for k in ("sum", "sumsq")] == [6, 6]
    one = edge_film(1, 1, "finite", True)
    assert one["n"].tolist() == [2] and one["sum"].tolist() == [[1.0, 1.0, 1.0]]                 # the catalogue fills a small image


# ---- the statements ------------------------------------------------------------------------------------------------------------------------
def r32(x):
    """one rounding to f32 of a float64 value"""
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


def f64(x):
    with np.errstate(all="ignore"):                                   # a signalling NaN raises "invalid" when it is widened
        return np.asarray(x).astype(np.float64)


def statement_mean(s, n):
    """film.rs:43-47 per operation: every f32 operation in float64, rounded to f32 once (for + - * / of f32 operands that IS the correctly
    rounded f32 result: 53 >= 2 * 24 + 2)"""
    with np.errstate(all="ignore"):
        fn = r32(f64(n))
        inv = r32(1.0 / f64(fn))
        return r32(f64(s) * f64(inv)[:, None])


def statement_variance(s, q, n):
    """film.rs:51-67 per operation; n * (n - 1) modulo 2^32 in Python integers, then converted to f32"""
    nn1_int = np.array([(int(k) * (int(k) - 1)) % (1 << 32) for k in n], np.uint64)
    with np.errstate(all="ignore"):
        nn1 = r32(f64(nn1_int))[:, None]
        n2n1 = r32(f64(r32(f64(n)))[:, None] * f64(nn1))
        a = r32(f64(q) / f64(nn1))
        b = r32(f64(r32(f64(s) * f64(s))) / f64(n2n1))
        return r32(f64(r32(f64(a) - f64(b))) * 50.0)


def statement_pack(c):
    """tonemap.rs:4-10 + color.rs:85-95 per operation: c / (1 + c), Rust's min / max (the non-NaN operand), * 255, truncated"""
    with np.errstate(all="ignore"):
        m = r32(f64(c) / f64(r32(1.0 + f64(c))))
        x = np.where(np.isnan(m), F(1), m)
        x = np.where(x > 1, F(1), x)
        x = np.where(x > 0, x, F(0))
        u = np.floor(f64(r32(f64(x) * 255.0))).astype(np.uint32)
    return (u[:, 2] | (u[:, 1] << np.uint32(8)) | (u[:, 0] << np.uint32(16)) | np.uint32(0xFF000000)).astype(np.uint32)


def numpy_variance(s, q, n):
    """the same in plain numpy f32"""
    with np.errstate(all="ignore"):
        nn1 = (n * (n - np.uint32(1))).astype(np.float32)[:, None]
        n2n1 = n.astype(np.float32)[:, None] * nn1
        return (q / nn1 - s * s / n2n1) * F(50)


def statement_merge(*films):
    """((0 + f0) + f1) + ...: one addition per value, in float64 rounded once; n modulo 2^32 (the planes every film has)"""
    keys = ("sum", "sumsq") + (("direct",) if all(f["direct"] is not None for f in films) else ())
    out = {k: np.zeros_like(films[0][k]) for k in keys}
    total = np.zeros(films[0]["n"].size, np.uint64)
    for f in films:
        total = (total + f["n"].astype(np.uint64)) % np.uint64(1 << 32)
        for k in keys:
            out[k] = r32(f64(out[k]) + f64(f[k]))
    return dict(out, n=total.astype(np.uint32), direct=out.get("direct"))


def statement_add(a, b):
    """mi355rt_film_add of b onto a handle that holds a: a + b per value (the handle's value on the left), n in u32"""
    keys = ("sum", "sumsq") + (("direct",) if a["direct"] is not None and b["direct"] is not None else ())
    out = {k: r32(f64(a[k]) + f64(b[k])) for k in keys}
    return dict(out, n=((a["n"].astype(np.uint64) + b["n"].astype(np.uint64)) % np.uint64(1 << 32)).astype(np.uint32), direct=out.get("direct"))


def tri_normals(scene):
    """calc_normal (mod.rs:198-205) in vecmath.rs order (as tests/test_gpu_denoise.py states it)"""
    v = np.asarray(scene["tri_verts"], np.float32).reshape(-1, 9)
    a = v[:, 3:6] - v[:, 0:3]; b = v[:, 6:9] - v[:, 0:3]
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.stack([cx / ln, cy / ln, cz / ln], axis=1).astype(np.float32)


class Oracles:
    """one oracle per shape, shared by the tests of this file (every use sets its film first), and the guide buffers made from it"""

    def __init__(self, oracle, scenes):
        self._oracle, self._scene, self._made, self._guides = oracle, scenes(SCENE), {}, {}

    def get(self, w, h):
        if (w, h) not in self._made:
            self._made[(w, h)] = self._oracle.Oracle(self._scene, w, h, seed=1)
        return self._made[(w, h)]

    def readouts(self, f):
        """(mean, variance, packed) of the film f"""
        orc = self.get(f["width"], f["height"])
        orc.film_set(f["sum"], f["sumsq"], f["n"])
        return orc.get_pixels(), orc.get_estimated_variances(), orc.get_tonemapped_pixels()

    def guides(self, w, h):
        """the guide buffers of the handle's default view from the oracle (untextured scenes; tests/test_gpu_denoise.py checks the device's
        against the same construction)"""
        if (w, h) not in self._guides:
            scene = self._scene
            assert not (np.asarray(scene["mat_kind"]) == 1).any()
            orc = self.get(w, h)
            p = np.arange(w * h)
            rays = np.stack([orc.get_ray(int(a), int(b), 0.5, 0.5) for a, b in zip(p % w, p // h)])
            tuv, prim = orc.intersect(rays, nthreads=4)
            hit = prim != MISS
            g = dict(depth=np.zeros(w * h, np.float32), normal=np.zeros((w * h, 3), np.float32), albedo=np.zeros((w * h, 3), np.float32),
                     prim=prim.astype(np.uint32))
            pi = prim[hit].astype(np.int64)
            g["depth"][hit] = tuv[hit, 0]
            g["normal"][hit] = tri_normals(scene)[pi]
            g["albedo"][hit] = np.asarray(scene["mat_rgb"], np.float32)[np.asarray(scene["tri_geom"], np.int64)[pi]]
            self._guides[(w, h)] = g
        return self._guides[(w, h)]

    def close(self):
        for orc in self._made.values():
            orc.close()
        self._made.clear()


@pytest.fixture(scope="module")
def oracles(oracle, scenes):
    o = Oracles(oracle, scenes)
    yield o
    o.close()


@pytest.fixture(scope="module")
def fio(pkg):
    return importlib.import_module("raytracer_rs_amd.film_io")


@pytest.fixture(scope="module")
def dn(pkg):
    return importlib.import_module("raytracer_rs_amd.denoise")


@pytest.fixture(scope="module")
def ad(pkg):
    return importlib.import_module("raytracer_rs_amd.adaptive")


def adaptive_cfgs():
    """min_spp below and above the background's n (2..39); max_spp 64, 2^24 + 8 and 2^32 - 1 with batches of 1 and 8, so that max n + batch lands on
    (2^24 + 8), just under (2^24 + 1, 2^31 + 8) and just over (2^24 + 9, 2^32, 2^32 + 7) the cap; abs_floor 0 and 0.01.  rel_error 0.2 settles the
    background pixels with n >= 9 (0.3 s^2 <= 0.04 (n - 1) s^2) and no other."""
    return [dict(min_spp=mn, max_spp=mx, batch_spp=b, max_rounds=0, rel_error=0.2, abs_floor=fl)
            for mn in (2, 40) for mx in (64, (1 << 24) + 8, 0xFFFFFFFF) for b in (1, 8) for fl in (0.0, 0.01)]


def want_mask(ad, f, cfg, owned=None):
    return ad.tile_mask(f["sum"], f["sumsq"], f["n"], f["width"], f["height"], owned_rows=owned, **cfg)


# ---- a. the oracle against the float64 statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 1), (9, 1), BIG])
def test_a_oracle_equals_the_float64_statement(pkg, oracles, dn, shape, kind):
    f = edge_film(*shape, kind, False)
    orc = oracles.get(*shape)
    orc.film_set(f["sum"], f["sumsq"], f["n"])
    s, q, n = orc.film()
    same_bits(dict(sum=s, sumsq=q, n=n), f, "oracle_film_set")                    # bits unchanged, payloads included
    mean, var, px = orc.get_pixels(), orc.get_estimated_variances(), orc.get_tonemapped_pixels()
    want_mean = statement_mean(f["sum"], f["n"])
    same(mean, want_mean, "mean")
    same(var, statement_variance(f["sum"], f["sumsq"], f["n"]), "variance")
    same(px, statement_pack(want_mean), "packed")
    # the numpy statements the library is held to say the same
    same(numpy_variance(f["sum"], f["sumsq"], f["n"]), statement_variance(f["sum"], f["sumsq"], f["n"]), "numpy f32 variance")
    same(dn.film_inputs(f["sum"], f["sumsq"], f["n"])[0], want_mean, "denoise.film_inputs mean")
    same(dn.pack(want_mean), px, "denoise.pack")
    if shape == BIG:                                                              # what the catalogue is there for
        first = {e[0]: int(np.flatnonzero((f["n"] == e[0]) & (f["sum"][:, 1] == F(e[1])))[0]) for e in CATALOGUE[4:6]}
        # 65536 * 65535 = 2^32 - 65536 still fits; 65537 * 65536 wraps to 65536, and the variance is 65535 times the unwrapped one
        assert var[first[65537], 0] > 6e4 * var[first[65536], 0] > 0
        assert (px[f["n"] == 0] == 0xFFFFFFFF).any()                              # NaN packs to white
        assert np.isnan(mean[f["n"] == 0]).any() and np.isinf(mean[f["n"] == 0]).any()


# ---- b. the statements on these films: what keeps the GPU tests from being vacuous ---------------------------------------------------------
def test_b_reference_behaviour_on_edge_films(pkg, oracles, dn, ad):
    w, h = BIG
    g = oracles.guides(w, h)
    assert (g["prim"] != MISS).any() and (g["prim"] == MISS).any()
    f = edge_film(w, h, "finite", True)
    some = f["n"] >= 1
    for it in (0, 1, 5):
        for prm in PARAMS:
            rgb, _ = dn.denoise(f["sum"], f["sumsq"], f["n"], g, w, h, iterations=it, **prm)
            assert np.isfinite(rgb[some]).all(), ("denoise", it, prm)
            assert not np.isfinite(rgb[~some]).any()
            rgb, _ = dn.denoise_split(f["sum"], f["sumsq"], f["n"], f["direct"], g, w, h, iterations=it, **prm)
            assert np.isfinite(rgb[some]).all(), ("denoise_split", it, prm)
    for direct in (False, True):
        x = edge_film(w, h, "nonfinite", direct)
        for it in (1, 2):
            rgb, _ = dn.denoise(x["sum"], x["sumsq"], x["n"], g, w, h, iterations=it, **PARAMS[0])
            share = float(np.isnan(rgb).any(axis=1).mean())
            print("nonfinite film, direct %d, %d iterations: %.1f %% of the pixels are NaN" % (direct, it, 100 * share))
            assert 0 < share <= nan_share_bound(w, it) <= 0.5, (direct, it, share)
            if direct:
                rgb, _ = dn.denoise_split(x["sum"], x["sumsq"], x["n"], x["direct"], g, w, h, iterations=it, **PARAMS[0])
                share = float(np.isnan(rgb).any(axis=1).mean())
                print("    the split read-out: %.1f %%" % (100 * share))
                assert 0 < share <= nan_share_bound(w, it) <= 0.5, ("split", it, share)
    cfgs = adaptive_cfgs()
    masks = [want_mask(ad, f, cfg) for cfg in cfgs]
    assert all(m.any() and not m.all() for m in masks)                            # both active and inactive tiles
    # ... but there nearly every tile is busy whatever one pixel says; isolated_film() is where each knob moves a tile
    iso = isolated_film()
    imasks = {tuple(sorted(cfg.items())): want_mask(ad, iso, cfg, None) for cfg in cfgs}
    assert all(m.any() and not m.all() for m in imasks.values())

    def differ(key, a, b):
        """configurations that differ in `key` alone (a against b) and give different masks"""
        return sum(not np.array_equal(imasks[tuple(sorted(dict(cfg, **{key: a}).items()))], imasks[tuple(sorted(dict(cfg, **{key: b}).items()))])
                   for cfg in cfgs if cfg[key] == a)
    assert differ("min_spp", 2, 40) >= 1 and differ("abs_floor", 0.0, 0.01) >= 1 and differ("batch_spp", 1, 8) >= 1
    assert differ("max_spp", 64, (1 << 24) + 8) >= 1 and differ("max_spp", (1 << 24) + 8, 0xFFFFFFFF) >= 1
    # max n + batch in 64 bits: a tile holding n = 2^32 - 1 is inactive under every cap, though its u32 sum would pass
    tiles = ad.pixel_tiles(w, h).reshape(-1)
    top = np.unique(tiles[f["n"] == 0xFFFFFFFF])
    assert top.size and not any(m.reshape(-1)[top].any() for m in masks)
    itop = np.unique(ad.pixel_tiles(*ISOLATED).reshape(-1)[iso["n"] == 0xFFFFFFFF])
    busy = want_mask(ad, dict(iso, n=np.where(iso["n"] == 0xFFFFFFFF, np.uint32(40), iso["n"])), cfgs[-1]).reshape(-1)[itop]
    assert busy.any() and not any(m.reshape(-1)[itop].any() for m in imasks.values())        # busy, and inactive for the cap alone
    # a striped handle: catalogue pixels in rows it does not own would change the verdict if they counted
    for rank in (0, 1):
        own = np.array([r for r in range(h) if (r // 4) % 2 == rank])
        assert any((want_mask(ad, f, cfg, own) & ~m).any() for cfg, m in zip(cfgs, masks)), rank     # a large n next door caps no tile


# ---- c. the film file round trip ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_c_film_files_round_trip_and_merge(pkg, fio, tmp_path, kind, direct):
    w, h = BIG
    f, b = edge_film(w, h, kind, direct), background_film(w, h, direct, seed=2)
    path = tmp_path / "edge.film"
    fio.write(path, w, h, f["n"], f["sum"], f["sumsq"], f["direct"], seed=3, flags=0)
    back = fio.read(path)
    same_bits(back, f, "write -> read")
    assert (back["direct"] is None) == (not direct) and (back["width"], back["height"], back["seed"]) == (w, h, 3)
    same_film(fio.merge(back, back), statement_merge(f, f), "merge with itself")
    same_film(fio.merge(back, b), statement_merge(f, b), "merge with a background")
    same_film(fio.merge(b, back, back), statement_merge(b, f, f), "merge of three")
    m = fio.merge(back, back)
    assert (m["n"][f["n"] == 0x80000000] == 0).all() and (m["n"][f["n"] == 0xFFFFFFFF] == 0xFFFFFFFE).all()      # n wraps in u32
    if kind == "nonfinite":
        assert np.isnan(m["sum"]).any() and np.isinf(m["sumsq"]).any()


# ---- the handles ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles(pkg, scenes):
    """handle(w, h, direct, **stripes): one small handle per shape, shared by the tests of this file (each sets the film it reads)"""
    made = {}

    def get(w, h, direct, **kw):
        key = (w, h, direct, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = pkg.create_raytracer_from_arrays(scenes(SCENE), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=1,
                                                         flags=pkg.FLAG_DIRECT_FILM if direct else 0, **kw)
        return made[key]
    yield get
    for rt in made.values():
        rt.close()


def put(rt, f, add=False):
    """f has a direct plane exactly when the handle keeps one"""
    (rt.film.add if add else rt.film.set)(f["sum"], f["sumsq"], f["n"], f["direct"])


def film_of(fio, rt, direct):
    s, q, n = rt.film.pixel_datas()
    return fio.film(rt.width, rt.height, n, s, q, rt.film.direct_sums() if direct else None)


def assert_only_read(fio, rt, f):
    """h: the film is still what was stored, bit for bit.  (The guard bytes of MI355RT_DEBUG_GUARD sit behind the render pass buffers only, which
    a handle that never rendered does not have: debug_check_guards() could not fail here, so it is not asserted.)"""
    same_bits(film_of(fio, rt, f["direct"] is not None), f, "the film after the read-outs")


def check_plain(rt, oracles, dn, f):
    """d on the film f the handle holds"""
    want_mean, want_var, want_px = oracles.readouts(f)
    mean = rt.film.get_pixels()
    same(mean, want_mean, "get_pixels")
    same(mean, statement_mean(f["sum"], f["n"]), "get_pixels against the float64 statement")
    same(rt.film.get_estimated_variances(), want_var, "get_estimated_variances")
    px = rt.get_tonemapped_pixels()
    same(px, want_px, "get_tonemapped_pixels")
    same(px, dn.pack(want_mean), "get_tonemapped_pixels against denoise.pack")
    for split in ([False, True] if f["direct"] is not None else [False]):
        rgb0, px0 = rt.get_denoised_pixels(iterations=0, split=split)
        same(rgb0, want_mean, "iterations = 0, split %d" % split)
        same(px0, want_px, "iterations = 0 packed, split %d" % split)


def check_adaptive(rt, ad, f, owned=None):
    """e on the film f the handle holds"""
    for cfg in adaptive_cfgs():
        same(rt.adaptive_tile_mask(**cfg), want_mask(ad, f, cfg, owned), "tile mask %r" % (cfg,))


# ---- d. plain read-outs ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_d_plain_read_outs_equal_the_oracle(pkg, fio, dn, oracles, handles, shape, kind, direct):
    rt = handles(*shape, direct)
    f = edge_film(*shape, kind, direct)
    put(rt, f)
    check_plain(rt, oracles, dn, f)
    assert_only_read(fio, rt, f)


# ---- e. the adaptive verdict ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_e_tile_mask_equals_the_numpy_statement(pkg, fio, ad, handles, shape, kind):
    rt = handles(*shape, True)
    f = edge_film(*shape, kind, True)
    put(rt, f)
    check_adaptive(rt, ad, f)
    assert_only_read(fio, rt, f)


@gpu
def test_e_tile_mask_follows_single_catalogue_pixels(pkg, fio, ad, handles):
    """one catalogue pixel per tile in a settled background (isolated_film): every tile's verdict is that pixel's"""
    rt = handles(*ISOLATED, True)
    f = isolated_film()
    put(rt, f)
    check_adaptive(rt, ad, f)
    assert_only_read(fio, rt, f)


@gpu
@pytest.mark.parametrize("rank", [0, 1])
def test_e_rows_of_another_stripe_do_not_count(pkg, fio, ad, handles, rank):
    w, h = BIG
    rt = handles(w, h, True, stripe_rows=4, stripe_rank=rank, stripe_world=2)
    f = edge_film(w, h, "finite", True)
    put(rt, f)
    owned = rt.owned_rows()
    assert np.array_equal(owned, [r for r in range(h) if (r // 4) % 2 == rank])
    foreign = np.ones(h, bool); foreign[owned] = False
    assert (f["n"].reshape(h, w)[foreign] > 39).any()                             # catalogue pixels in rows the handle does not own
    check_adaptive(rt, ad, f, owned)
    got = film_of(fio, rt, True)
    assert not got["n"].reshape(h, w)[foreign].any() and np.array_equal(got["n"].reshape(h, w)[owned], f["n"].reshape(h, w)[owned])


# ---- f. the denoiser ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_f_denoised_read_out_equals_the_numpy_statement(pkg, fio, dn, handles, shape, kind, split):
    w, h = shape
    rt = handles(w, h, True)
    f = edge_film(w, h, kind, True)
    put(rt, f)
    g = rt.guides()
    rt.get_denoised_pixels(iterations=1, split=split)                             # the filter's buffers exist from here on
    hbm = rt.hbm_allocated_bytes()
    some = f["n"] >= 1
    for prm in PARAMS:
        for it in ((0, 1, 2, 5, 8) if kind == "finite" else (1, 2)):              # step 128 at the 8th: every tap but the centre is outside
            if split:
                want_rgb, want_px = dn.denoise_split(f["sum"], f["sumsq"], f["n"], f["direct"], g, w, h, iterations=it, **prm)
            else:
                want_rgb, want_px = dn.denoise(f["sum"], f["sumsq"], f["n"], g, w, h, iterations=it, **prm)
            if kind == "finite":
                assert np.isfinite(want_rgb[some]).all(), (prm, it)                # of the statement: the comparison below is on numbers
            elif w >= 30:                                                         # narrower images lie inside one value's footprint
                assert np.isnan(want_rgb).any(axis=1).mean() <= nan_share_bound(w, it) <= 0.5, (prm, it)
            rgb, px = rt.get_denoised_pixels(iterations=it, split=split, **prm)
            same(rgb, want_rgb, "rgb %r, %d iterations" % (prm, it))
            same(px, want_px, "packed %r, %d iterations" % (prm, it))
    _, only_px = rt.get_denoised_pixels(rgb=False, iterations=2, split=split, **PARAMS[1])
    only_rgb, _ = rt.get_denoised_pixels(packed=False, iterations=2, split=split, **PARAMS[1])
    want_rgb, want_px = (dn.denoise_split(f["sum"], f["sumsq"], f["n"], f["direct"], g, w, h, iterations=2, **PARAMS[1]) if split else
                         dn.denoise(f["sum"], f["sumsq"], f["n"], g, w, h, iterations=2, **PARAMS[1]))
    same(only_px, want_px, "packed only"); same(only_rgb, want_rgb, "rgb only")
    assert rt.hbm_allocated_bytes() == hbm
    assert_only_read(fio, rt, f)


# ---- g. add ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_g_add_equals_one_addition_per_value(pkg, fio, dn, ad, oracles, handles, shape, direct):
    """inf + -inf, NaN operands, denormal sums, -0.0 + 0.0 and -0.0 + -0.0, n past 2^32"""
    rt = handles(*shape, direct)
    a, b = edge_film(*shape, "nonfinite", direct, seed=1), edge_film(*shape, "nonfinite", direct, seed=2)
    put(rt, a); put(rt, b, add=True)
    same_film(film_of(fio, rt, direct), statement_add(a, b), "add onto a film that was set")
    rt.film.clear()
    put(rt, a, add=True); put(rt, b, add=True)
    m = fio.merge(a, b)
    got = film_of(fio, rt, direct)
    same_film(got, m, "add, twice, onto an empty film")
    same_film(got, statement_merge(a, b), "add, twice, against the float64 statement")
    if shape == BIG:
        assert (m["n"] < np.minimum(a["n"], b["n"])).any()                        # n went past 2^32
        assert np.isnan(m["sum"]).any() or np.isnan(m["sumsq"]).any()
    # the read-outs on the film the handle now holds
    check_plain(rt, oracles, dn, got)
    check_adaptive(rt, ad, got)
    assert_only_read(fio, rt, got)


@gpu
def test_g_add_of_two_finite_films_and_through_files(pkg, fio, dn, ad, oracles, handles, tmp_path):
    w, h = BIG
    rt = handles(w, h, True)
    a, b = edge_film(w, h, "finite", True, seed=1), edge_film(w, h, "nonfinite", True, seed=2)
    pa, pb = tmp_path / "a.film", tmp_path / "b.film"
    fio.write(pa, w, h, a["n"], a["sum"], a["sumsq"], a["direct"])
    fio.write(pb, w, h, b["n"], b["sum"], b["sumsq"], b["direct"])
    rt.film.load(pa)
    same_bits(film_of(fio, rt, True), a, "load")
    rt.film.load(pb, add=True)
    got = film_of(fio, rt, True)
    same_film(got, statement_add(a, b), "load, then load with add")
    check_plain(rt, oracles, dn, got)
    check_adaptive(rt, ad, got)
    # two finite films: sums that cancel, overflow and leave the denormal range
    c = edge_film(w, h, "finite", True, seed=3)
    put(rt, a); put(rt, c, add=True)
    got = film_of(fio, rt, True)
    same_film(got, statement_add(a, c), "add of finite films")
    check_plain(rt, oracles, dn, got)
    check_adaptive(rt, ad, got)
    assert_only_read(fio, rt, got)


# ---- h. read-outs only read ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_h_read_outs_only_read(pkg, fio, dn, ad, oracles, handles, kind):
    """every read-out of d to f in a row on one film: the film keeps every bit set gave it, and the device memory the handle holds is
    what it was after the first denoised read-out (guard bytes: see assert_only_read)"""
    w, h = BIG
    rt = handles(w, h, True)
    f = edge_film(w, h, kind, True)
    put(rt, f)
    rt.get_denoised_pixels(iterations=1)
    hbm = rt.hbm_allocated_bytes()
    check_plain(rt, oracles, dn, f)
    check_adaptive(rt, ad, f)
    for split in (False, True):
        for it in (1, 5, 8):
            rt.get_denoised_pixels(iterations=it, split=split, **PARAMS[it % 3])
    rt.guides()
    assert_only_read(fio, rt, f)
    assert rt.hbm_allocated_bytes() == hbm
