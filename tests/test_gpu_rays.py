"""Caller-supplied rays on the device (include/mi355rt.h, "caller-supplied rays").

The yardstick is the CPU oracle, unchanged: a sample's colour depends only on its ray, its hits and its key (pixel, sampleno), so the primary rays of an
oracle B whose camera was MOVED, fed to a handle A whose camera was not, must give B's colours bit for bit — A's own camera could not have made them.
Every comparison is on the bits (array_equal of uint32 views), in the three intersector semantics (sem3) unless noted."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_gpu_display import read_png, rgb_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
W, H, SEED = 37, 21, 5
N = W * H                      # 777 rays: 4 chunks of 256 (the last one partial), 13 waves (the last one partial)
SNO = 3                        # the sample number of the rays of tests 1-4
MISS = 0xFFFFFFFF
ALL = ("rgb", "direct", "tuv", "prim")
E_INVALID = -1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cams(pkg):
    return importlib.import_module("raytracer_rs_amd.cameras")


def make(pkg, scenes, name, w=W, h=H, **kw):
    kw.setdefault("seed", SEED)
    return pkg.create_raytracer_from_arrays(scenes(name), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, **kw)


def moved_oracle(oracle, scenes, name, flags):
    b = oracle.Oracle(scenes(name), W, H, seed=SEED, flags=flags)
    b.camera_move_rel(0.3, -0.2, 0.5); b.camera_add_y_angle(0.2); b.camera_add_x_angle(-0.1)
    return b


_REF = {}


def reference(oracle, scenes, name, orc_flags):
    """Oracle B's rays (p, SNO) with their keys and what B computes along them; computed once per (scene, oracle semantics) and never written to"""
    key = (name, orc_flags)
    if key not in _REF:
        b = moved_oracle(oracle, scenes, name, orc_flags)
        rays = np.array([b.primary_ray(p, SNO) for p in range(N)], np.float32)
        keys = np.stack([np.arange(N, dtype=np.uint32), np.full(N, SNO, np.uint32)], axis=1)
        dbg = [b.sample_debug(p, SNO) for p in range(N)]
        ref = dict(rays=rays, keys=np.ascontiguousarray(keys), rgb=np.array([d[0] for d in dbg], np.float32), direct=np.array([d[1][0] for d in dbg], np.float32),
                   hit=np.array([d[2][0] for d in dbg], bool))
        b.close()
        for v in ref.values():
            v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def assert_worth_something(ref):
    """the input decides something: enough hits, enough misses, and enough rays whose colour is more than the root light sum (the bounce tree matters)"""
    hits = ref["hit"].mean()
    deeper = np.any(bits(ref["rgb"]) != bits(ref["direct"]), axis=1).mean()
    assert hits >= 0.15 and 1.0 - hits >= 0.15 and deeper >= 0.02, (hits, deeper)


@pytest.fixture(scope="module")
def handles(pkg, scenes):
    made = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = make(pkg, scenes, name, **kw)
        return made[key]
    yield get
    for rt in made.values():
        rt.close()


def film_of(rt, direct=False):
    s, q, n = rt.film.pixel_datas()
    return (bits(s).copy(), bits(q).copy(), n.copy()) + ((bits(rt.film.direct_sums()).copy(),) if direct else ())


def same_film(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. trace_rays equals the oracle on rays the handle's camera never made -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["thai2", "ico2", "ico3_tex"])
def test_trace_rays_equals_the_oracle_on_foreign_rays(pkg, oracle, scenes, handles, sem3, name):
    ref = reference(oracle, scenes, name, sem3.orc)
    assert_worth_something(ref)
    a = handles(name, flags=sem3.gpu)
    own = np.array([a.camera.get_ray(p % W, p // H, 0.5, 0.5) for p in (0, N // 2, N - 1)], np.float32)
    assert not np.allclose(own[:, :3], ref["rays"][0, :3])                     # A stands elsewhere: these are not its rays
    got = a.trace_rays(ref["rays"], ref["keys"], want=ALL)
    assert np.array_equal(bits(got["rgb"]), bits(ref["rgb"]))
    assert np.array_equal(bits(got["direct"]), bits(ref["direct"]))
    tuv, prim = a.intersect_rays(ref["rays"])
    assert np.array_equal(got["prim"], prim) and np.array_equal(bits(got["tuv"]), bits(tuv))
    assert np.array_equal(prim != MISS, ref["hit"])
    c = a.last_counts()
    assert (c.primary, c.primary_hits, c.primary_culled) == (N, int(ref["hit"].sum()), 0)
    # a miss is black in both colour outputs
    assert not bits(got["rgb"])[~ref["hit"]].any() and not bits(got["direct"])[~ref["hit"]].any()


# ---- 2. sizes around the wave and the chunk --------------------------------------------------------------------------------------------------------
GUARD = 16


def raw_trace(pkg, rt, rays, keys, n, want=ALL, where=0, sentinel=0xA5A5A5A5):
    """mi355rt_trace_rays through ctypes into sentinel-filled outputs with GUARD extra entries each; returns (code, {name: uint32 array incl. guard})"""
    o, arrs = pkg.RayOutputs(), {}
    for w in want:
        arrs[w] = np.full((n + GUARD) * (1 if w == "prim" else 3), sentinel, np.uint32)
        setattr(o, w, arrs[w].ctypes.data)
    code = pkg.lib().mi355rt_trace_rays(rt._h, None if rays is None else rays.ctypes.data, None if keys is None else keys.ctypes.data, n, where, C.byref(o))
    return code, arrs


def test_sizes_around_the_wave_and_the_chunk(pkg, oracle, scenes, handles, sem3):
    ref = reference(oracle, scenes, "thai2", sem3.orc)
    a = handles("thai2", flags=sem3.gpu)
    full = a.trace_rays(ref["rays"], ref["keys"], want=ALL)
    code, arrs = raw_trace(pkg, a, ref["rays"], ref["keys"], 0)
    assert code == 0 and all(np.all(v == 0xA5A5A5A5) for v in arrs.values())      # n == 0 succeeds and writes nothing
    assert pkg.lib().mi355rt_trace_rays(a._h, None, None, 0, 0, C.byref(pkg.RayOutputs(rgb=arrs["rgb"].ctypes.data))) == 0
    for n in (1, 63, 64, 65, 255, 256, 257, 777):
        rays, keys = np.ascontiguousarray(ref["rays"][:n]), np.ascontiguousarray(ref["keys"][:n])
        code, arrs = raw_trace(pkg, a, rays, keys, n)
        assert code == 0, a._check(code)
        for w in ALL:
            k = 1 if w == "prim" else 3
            assert np.all(arrs[w][n * k:] == 0xA5A5A5A5), (n, w)                      # the guard entries behind each output
            want = full[w][:n].reshape(-1).view(np.uint32)
            if w == "tuv":                                                          # untouched on a miss: the sentinel stays
                want = np.where(np.repeat(full["prim"][:n] == MISS, 3), np.uint32(0xA5A5A5A5), want)
            assert np.array_equal(arrs[w][:n * k], want), (n, w)                     # ray i does not depend on n
        assert a.last_counts().primary == n


def test_a_call_spans_as_many_passes_as_it_needs(pkg, oracle, scenes, sem3):
    """config.samples_per_pass = 1 on a 16 x 12 handle bounds a pass at 192 rays: 777 rays are five passes (the last of 9 rays), and keys=None must
    number the rays by the CALL's index"""
    ref = reference(oracle, scenes, "ico2", sem3.orc)
    small = make(pkg, scenes, "ico2", 16, 12, flags=sem3.gpu, samples_per_pass=1)
    got = small.trace_rays(ref["rays"], ref["keys"], want=ALL)
    assert np.array_equal(bits(got["rgb"]), bits(ref["rgb"])) and np.array_equal(bits(got["direct"]), bits(ref["direct"]))
    tuv, prim = small.intersect_rays(ref["rays"])
    assert np.array_equal(got["prim"], prim) and np.array_equal(bits(got["tuv"]), bits(tuv))
    assert small.last_counts().primary == N
    explicit = np.ascontiguousarray(np.stack([np.arange(N, dtype=np.uint32), np.zeros(N, np.uint32)], axis=1))
    assert np.array_equal(bits(small.trace_rays(ref["rays"])["rgb"]), bits(small.trace_rays(ref["rays"], explicit)["rgb"]))
    small.close()


# ---- 3. keys ---------------------------------------------------------------------------------------------------------------------------------------
def test_keys(pkg, oracle, scenes, handles, sem3):
    ref = reference(oracle, scenes, "thai2", sem3.orc)
    a = handles("thai2", flags=sem3.gpu)
    base = a.trace_rays(ref["rays"], ref["keys"], want=ALL)
    # keys=None is (i, 0)
    explicit = np.ascontiguousarray(np.stack([np.arange(N, dtype=np.uint32), np.zeros(N, np.uint32)], axis=1))
    none, expl = a.trace_rays(ref["rays"], None, want=ALL), a.trace_rays(ref["rays"], explicit, want=ALL)
    assert all(np.array_equal(none[w].view(np.uint32), expl[w].view(np.uint32)) for w in ALL)
    # Keys far outside the image.  The oracle cannot restate them (its pixel makes the ray AND keys the hashes), so: the call succeeds, everything of the
    # first level — which draws no random number — is unchanged, and the colour of rays with a bounce tree does change somewhere
    far = np.ascontiguousarray(np.stack([(0xFFFFFFF0 + np.arange(N, dtype=np.uint64)).astype(np.uint32), np.full(N, 2 ** 31, np.uint32)], axis=1))
    got = a.trace_rays(ref["rays"], far, want=ALL)
    for w in ("direct", "tuv", "prim"):
        assert np.array_equal(got[w].view(np.uint32), base[w].view(np.uint32)), w
    changed = np.any(bits(got["rgb"]) != bits(base["rgb"]), axis=1)
    assert changed.any() and not changed[~ref["hit"]].any()
    assert np.all(np.isfinite(got["rgb"]))
    # permuting rays together with their keys permutes the results
    perm = np.random.default_rng(7).permutation(N)
    pr = a.trace_rays(np.ascontiguousarray(ref["rays"][perm]), np.ascontiguousarray(ref["keys"][perm]), want=ALL)
    assert all(np.array_equal(pr[w].view(np.uint32), base[w][perm].view(np.uint32)) for w in ALL)
    # two rays with one key draw the same numbers: a ray keyed like ray 0 equals ray 0 traced under that key
    same = np.ascontiguousarray(np.tile(ref["keys"][:1], (N, 1)))
    one = a.trace_rays(ref["rays"], same, want=("rgb",))["rgb"]
    assert np.array_equal(bits(one[0]), bits(base["rgb"][0]))


# ---- 4. trace_rays only reads ------------------------------------------------------------------------------------------------------------------------
def test_trace_rays_only_reads(pkg, oracle, scenes, sem3):
    """Across the call stay: the film, the direct film, current_row, the guides, the next get_tonemapped_pixels and the handle's device memory.  The
    counters: the header states that mi355rt_last_counts afterwards reports THIS call (primary == n), so what stays is the counters the previous call
    returned to its caller; last_counts is checked to hold the new call's."""
    ref = reference(oracle, scenes, "ico2", sem3.orc)
    a = make(pkg, scenes, "ico2", flags=sem3.gpu | pkg.FLAG_DIRECT_FILM)
    a.trace_frame_additive()
    a.synchronize()
    prev_counts = a.render(3)
    prev = prev_counts.as_dict()
    before = film_of(a, direct=True)
    row, guides, ldr = a.current_row, a.guides(), a.get_tonemapped_pixels().copy()
    hbm = a.hbm_allocated_bytes()
    got = a.trace_rays(ref["rays"], ref["keys"], want=ALL)
    assert np.array_equal(bits(got["rgb"]), bits(ref["rgb"]))
    assert a.hbm_allocated_bytes() == hbm
    assert same_film(film_of(a, direct=True), before)
    assert a.current_row == row
    after = a.guides()
    assert all(np.array_equal(after[k].view(np.uint32), guides[k].view(np.uint32)) for k in guides)
    assert np.array_equal(a.get_tonemapped_pixels(), ldr)
    now = a.last_counts()
    assert now.primary == N and now.primary_hits == int(ref["hit"].sum())
    assert prev["primary"] == N * 3 and prev_counts.as_dict() == prev
    # the guard of render_rays is not set by it
    a.get_denoised_pixels()
    a.close()


def test_trace_rays_after_render_async_and_inside_a_frame_loop(pkg, oracle, scenes, sem3):
    ref = reference(oracle, scenes, "ico2", sem3.orc)
    x, y = make(pkg, scenes, "ico2", flags=sem3.gpu), make(pkg, scenes, "ico2", flags=sem3.gpu)
    # behind a queued frame
    x.render(3); x.render(2, wait=False)
    got = x.trace_rays(ref["rays"], ref["keys"], want=ALL)
    assert np.array_equal(bits(got["rgb"]), bits(ref["rgb"])) and np.array_equal(bits(got["direct"]), bits(ref["direct"]))
    y.render(3); y.render(2)
    assert same_film(film_of(x), film_of(y))
    # in the middle of a trace_frame_additive loop: the speculative next frame is settled, given back, and the loop goes on as if nothing had happened
    x.film.clear(); y.film.clear()
    for _ in range(2):
        assert x.trace_frame_additive() == y.trace_frame_additive()
    row = x.current_row
    got = x.trace_rays(ref["rays"], ref["keys"], want=ALL)
    assert np.array_equal(bits(got["rgb"]), bits(ref["rgb"])) and x.current_row == row == y.current_row
    assert same_film(film_of(x), film_of(y))
    for _ in range(2):
        assert x.trace_frame_additive() == y.trace_frame_additive()
    assert same_film(film_of(x), film_of(y)) and np.array_equal(x.get_tonemapped_pixels(), y.get_tonemapped_pixels())
    x.close(); y.close()


# ---- 5. render_rays with the camera's own rays is render ------------------------------------------------------------------------------------------------
def own_rays(cams, rt, spp, flags=0):
    return cams.pinhole(rt.camera.matrices(), W, H, spp, SEED, film_n=rt.film.pixel_datas()[2], flags=flags)


def assert_counts_like_render(got, want):
    for k in ("primary", "bounce", "shadow", "primary_hits"):
        assert getattr(got, k) == getattr(want, k), k
    assert got.primary_culled == 0


@pytest.mark.parametrize("variant", ["plain", "passes_of_2", "continues_a_film", "direct_film", "fix_row_index"])
def test_render_rays_with_the_cameras_own_rays_is_render(pkg, oracle, cams, scenes, sem3, variant):
    kw, pre, direct, fix = {}, 0, False, 0
    if variant == "passes_of_2":
        kw["samples_per_pass"] = 2                       # passes of 2 + 2 + 1: the buffer must be indexed by the call's sample number
    if variant == "continues_a_film":
        pre = 3
    if variant == "direct_film":
        direct = True
    if variant == "fix_row_index":
        fix = pkg.FLAG_FIX_ROW_INDEX
    flags = sem3.gpu | (pkg.FLAG_DIRECT_FILM if direct else 0) | fix
    a, b = make(pkg, scenes, "ico2", flags=flags, **kw), make(pkg, scenes, "ico2", flags=flags, **kw)
    orc = oracle.Oracle(scenes("ico2"), W, H, seed=SEED, flags=sem3.orc | (oracle.FLAG_FIX_ROW_INDEX if fix else 0))
    if pre:
        a.render(pre); b.render(pre); orc.render(pre)
    ca = a.render_rays(own_rays(cams, a, 5, flags=fix), 5)
    cb = b.render(5)
    orc.render(5)
    assert_counts_like_render(ca, cb)
    assert ca.primary == N * 5
    fa = film_of(a, direct)
    assert same_film(fa, film_of(b, direct))
    os_, oq, on = orc.film()
    assert np.array_equal(fa[0], bits(os_)) and np.array_equal(fa[1], bits(oq)) and np.array_equal(fa[2], on) and np.all(on == pre + 5)
    assert np.array_equal(a.get_tonemapped_pixels(), b.get_tonemapped_pixels())
    assert np.array_equal(a.get_tonemapped_pixels(), orc.get_tonemapped_pixels())
    a.close(); b.close(); orc.close()


def test_render_rays_on_striped_handles(pkg, cams, scenes, sem3):
    whole = make(pkg, scenes, "ico2", flags=sem3.gpu)
    rays = own_rays(cams, whole, 5)
    whole.render(5)
    fw = film_of(whole)
    total = [np.zeros_like(fw[0], np.float32), np.zeros_like(fw[1], np.float32), np.zeros_like(fw[2])]
    for rank in (0, 1):
        st = make(pkg, scenes, "ico2", flags=sem3.gpu, stripe_world=2, stripe_rank=rank)
        owned = np.zeros(H, bool); owned[st.owned_rows()] = True
        poisoned = rays.reshape(5, H, W, 6).copy()
        poisoned[:, ~owned] = np.nan                                       # rows the handle does not own are not read ...
        c = st.render_rays(np.ascontiguousarray(poisoned.reshape(-1, 6)), 5)
        assert c.primary == int(owned.sum()) * W * 5 and c.primary_culled == 0
        s, q, n = st.film.pixel_datas()
        mask = np.repeat(owned, W)
        assert not bits(s)[~mask].any() and not bits(q)[~mask].any() and not n[~mask].any()      # ... nor written
        assert np.array_equal(bits(s)[mask], fw[0][mask]) and np.array_equal(bits(q)[mask], fw[1][mask]) and np.all(n[mask] == 5)
        total[0] += s; total[1] += q; total[2] += n
        # a striped handle serves trace_rays too: rays belong to no row
        assert st.trace_rays(rays[:65])["rgb"].shape == (65, 3)
        st.close()
    assert np.array_equal(bits(total[0]), fw[0]) and np.array_equal(bits(total[1]), fw[1]) and np.array_equal(total[2], fw[2])
    whole.close()


# ---- 6. render_rays with a moved oracle's rays on the unmoved handle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["thai2", "ico2"])
def test_render_rays_with_foreign_rays_equals_the_moved_oracle(pkg, oracle, scenes, handles, sem3, name):
    b = moved_oracle(oracle, scenes, name, sem3.orc)
    rays = np.array([[b.primary_ray(p, s) for p in range(N)] for s in range(4)], np.float32).reshape(-1, 6)
    oc = b.render(4)
    a = handles(name, flags=sem3.gpu)
    a.film.clear()
    c = a.render_rays(rays, 4)
    s, q, n = a.film.pixel_datas()
    os_, oq, on = b.film()
    assert np.array_equal(bits(s), bits(os_)) and np.array_equal(bits(q), bits(oq)) and np.array_equal(n, on)
    assert (c.primary, c.bounce, c.shadow, c.primary_hits, c.primary_culled) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"], 0)
    assert np.array_equal(a.get_tonemapped_pixels(), b.get_tonemapped_pixels())
    a.film.clear()
    b.close()


# ---- 7. device input ------------------------------------------------------------------------------------------------------------------------------------
def test_device_tensors_give_the_bits_of_host_arrays(pkg, oracle, cams, scenes, handles, sem3):
    import torch
    ref = reference(oracle, scenes, "ico2", sem3.orc)
    a = handles("ico2", flags=sem3.gpu)
    host = a.trace_rays(ref["rays"], ref["keys"], want=ALL)
    dev = torch.device("cuda", 0)
    rays_t = torch.from_numpy(ref["rays"].copy()).to(dev)
    keys_t = torch.from_numpy(ref["keys"].copy().view(np.int32)).to(dev)
    got = a.trace_rays(rays_t, keys_t, want=ALL)
    for w in ALL:
        assert isinstance(got[w], torch.Tensor) and got[w].device == dev
        assert np.array_equal(got[w].cpu().numpy().view(np.uint32), host[w].view(np.uint32)), w
    nokeys = a.trace_rays(rays_t, None, want=("rgb",))["rgb"].cpu().numpy()
    assert np.array_equal(bits(nokeys), bits(a.trace_rays(ref["rays"])["rgb"]))
    with pytest.raises(ValueError, match="GPU"):
        a.trace_rays(rays_t.cpu(), None)
    with pytest.raises(TypeError, match="dtype"):
        a.trace_rays(rays_t.double(), None)
    with pytest.raises(ValueError, match="keys must live where rays6 lives"):
        a.trace_rays(rays_t, ref["keys"])
    # render_rays
    a.film.clear()
    rays = own_rays(cams, a, 3)
    a.render_rays(rays, 3)
    want = film_of(a)
    a.film.clear()
    c = a.render_rays(torch.from_numpy(rays).to(dev), 3)
    assert c.primary == N * 3 and same_film(film_of(a), want)
    with pytest.raises(ValueError, match="GPU"):
        a.render_rays(torch.from_numpy(rays), 3)
    a.film.clear()


# ---- 8. the guard ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_guard(pkg, cams, scenes):
    a = make(pkg, scenes, "ico2", flags=pkg.FLAG_DIRECT_FILM)
    guarded = [lambda: a.get_denoised_pixels(), lambda: a.get_denoised_pixels(split=True), lambda: a.get_display_pixels(source=1),
               lambda: a.get_display_pixels(source=2), lambda: a.display_histogram(source=1), lambda: a.display_histogram(source=2),
               lambda: a.render_adaptive(max_rounds=1)]
    a.render(2)
    a.trace_rays(own_rays(cams, a, 1)[:100])               # never sets it
    for call in guarded:
        call()
    film_before = None
    for lift in ("clear", "set"):
        a.film.clear()
        a.render_rays(own_rays(cams, a, 2), 2)
        film_before = film_of(a, direct=True)
        for call in guarded:
            with pytest.raises(RuntimeError, match="mi355rt_render_rays"):
                call()
        assert same_film(film_of(a, direct=True), film_before)                  # a refused call changed nothing
        # the film, variance, tone-mapped and SOURCE_FILM display read-outs, and film add / save work as always
        a.film.get_pixels(); a.film.get_estimated_variances(); a.get_tonemapped_pixels(); a.get_display_pixels(source=0); a.display_histogram(source=0)
        s, q, n = a.film.pixel_datas()
        a.film.add(s, q, n, a.film.direct_sums())
        with pytest.raises(RuntimeError, match="mi355rt_render_rays"):           # add keeps the mark
            a.get_denoised_pixels()
        if lift == "clear":
            a.film.clear()
        else:
            a.film.set(s, q, n, a.film.direct_sums())
        for call in guarded:
            call()
    a.close()


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_argument_and_write_nothing(pkg, cams, scenes):
    a = make(pkg, scenes, "ico2")
    a.render(1)
    film = film_of(a)
    lib = pkg.lib()
    rays = own_rays(cams, a, 2)
    err = lambda: (lib.mi355rt_last_error(a._h) or b"").decode()

    def refused(code, arrs, *names):
        assert code == E_INVALID
        assert all(nm in err() for nm in names), err()
        assert all(np.all(v == 0xA5A5A5A5) for v in arrs.values())
        assert same_film(film_of(a), film)

    code, arrs = raw_trace(pkg, a, None, None, 10)
    refused(code, arrs, "mi355rt_trace_rays", "rays6")
    sentinel = np.full(30, 0xA5A5A5A5, np.uint32)
    assert lib.mi355rt_trace_rays(a._h, rays.ctypes.data, None, 10, 0, C.byref(pkg.RayOutputs())) == E_INVALID and "out" in err()
    assert lib.mi355rt_trace_rays(a._h, rays.ctypes.data, None, 10, 0, None) == E_INVALID and "out" in err()
    code, arrs = raw_trace(pkg, a, rays, None, 10, where=2)
    refused(code, arrs, "mi355rt_trace_rays", "where")
    counts = pkg.RayCounts()
    counts.primary = 12345
    for nrays, spp, names in ((N * 2 - 1, 2, ("nrays",)), (N * 2 + 1, 2, ("nrays",)), (0, 0, ("spp",)), (N * 2, 0, ("spp",))):
        assert lib.mi355rt_render_rays(a._h, rays.ctypes.data, nrays, spp, 0, C.byref(counts)) == E_INVALID
        refused(E_INVALID, {}, "mi355rt_render_rays", *names)
    assert lib.mi355rt_render_rays(a._h, None, N * 2, 2, 0, C.byref(counts)) == E_INVALID
    refused(E_INVALID, {}, "mi355rt_render_rays", "rays6")
    assert lib.mi355rt_render_rays(a._h, rays.ctypes.data, N * 2, 2, 7, C.byref(counts)) == E_INVALID
    refused(E_INVALID, {}, "mi355rt_render_rays", "where")
    assert counts.primary == 12345 and np.all(sentinel == 0xA5A5A5A5)
    a.get_denoised_pixels()                                  # a refused render_rays did not set the guard
    a.close()
    # a device group (here: two members sharing the one GPU)
    g = make(pkg, scenes, "ico2", device_count=2, flags=pkg.FLAG_GROUP_SHARES_DEVICE)
    g.render(1)
    gfilm = film_of(g)
    code, arrs = raw_trace(pkg, g, rays, None, 10)
    assert code == E_INVALID and "device group" in (lib.mi355rt_last_error(g._h) or b"").decode() and all(np.all(v == 0xA5A5A5A5) for v in arrs.values())
    assert lib.mi355rt_render_rays(g._h, rays.ctypes.data, N * 2, 2, 0, None) == E_INVALID
    assert "device group" in (lib.mi355rt_last_error(g._h) or b"").decode() and same_film(film_of(g), gfilm)
    g.close()


# ---- 10. custom cameras end to end: sanity, not parity -------------------------------------------------------------------------------------------------------
def facing_cam(max_xy=(0.36, 0.27)):
    """a camera at (0, 0, -6) looking along +z at the face z = -1 of the cube [-1, 1]^3 of 4boxes (x right, y up): the face is 5 units away, parallel to
    the image plane and turned towards the scene's light (at z = -4.2), and nothing stands in front of it"""
    rot = np.eye(4, dtype=np.float32).reshape(-1)
    orient = np.eye(4, dtype=np.float32); orient[3, :3] = (0.0, 0.0, -6.0)
    return rot, orient.reshape(-1), np.array(max_xy, np.float32)


def test_orthographic_rays_reach_a_parallel_face_at_one_distance(pkg, cams, scenes):
    w, h = 16, 12
    a = make(pkg, scenes, "4boxes", w, h)
    rays = cams.orthographic(facing_cam(), w, h, 1, SEED, 1.6)               # 1.6 x 1.2 world units: inside the 2 x 2 face
    got = a.trace_rays(rays, want=("tuv", "prim", "rgb"))
    assert np.all(got["prim"] != MISS)
    for row in got["tuv"][:, 0].reshape(h, w):
        assert np.all(np.abs(row - row[0]) <= 1e-5 * abs(row[0]))
    assert np.all(np.abs(got["tuv"][:, 0] - 5.0) <= 5e-5)
    # through render_rays: every pixel gets its samples
    c = a.render_rays(cams.orthographic(facing_cam(), w, h, 3, SEED, 1.6), 3)
    assert c.primary == c.primary_hits == w * h * 3 and np.all(a.film.pixel_datas()[2] == 3)
    a.close()


def phong_direct_sum(rays, spp, npix):
    """The direct term of rays that hit the face z = -1 of the cube of 4boxes (material (0.8, 0, 0), one light of colour 10, nothing in the way), summed over
    the channels and averaged over each pixel's samples: mod.rs:214-257 restated in numpy f64.  The only view-dependent part is the specular term."""
    light, n = np.array([1.887555, 1.433935, -4.194364]), np.array([0.0, 0.0, -1.0])
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    p = o + ((-1.0 - o[:, 2]) / d[:, 2])[:, None] * d
    ln = (light - p) / np.linalg.norm(light - p, axis=1)[:, None]
    ndl = ln @ n
    refl = 2.0 * ndl[:, None] * n - ln
    spec = np.sum(d / np.linalg.norm(d, axis=1)[:, None] * refl, axis=1) ** 32
    return (10.0 * (0.8 * ndl + 3.0 * spec)).reshape(spp, npix).mean(axis=0)


def test_thin_lens_keeps_the_focus_plane_and_blurs_the_rest(pkg, cams, scenes):
    """The face z = -1 of the cube fills the middle of the view at t = 5 (d_z = 1).  Focused there (focus 5), a lens sends every ray through the plane
    point its pinhole ray hits: the mean over the pixels well inside the face stays within the sampling noise of the pinhole image, measured as the
    difference of two pinhole seeds, times three.  Focused at 2.5 the face is off the focus depth, and its edge spills into pixels that were empty.

    The radius.  Same hit point, same bounce tree (the reflection rays hang on the hit point, the normal and the key): all a lens can change in the region
    is the Phong specular term pow32(view . refl), which follows the ray's direction — physics, not error.  phong_direct_sum above gives that shift from
    the rays alone: +0.02221 for radius 0.3 (a first version of this test used it; the device's film gave +0.022215 against a noise of 0.0050, so the
    film follows the model to 3e-7 and it was the radius that asked the wrong question) and +0.00081 for radius 0.1, an order below the noise.  Radius 0.1
    it is, and the film's shift is also held to the model: the two must agree to 1e-4 (f32 sums of 64 samples of size 7, against f64)."""
    w, h, spp, radius = 32, 24, 64, 0.1
    cam = facing_cam()
    a = make(pkg, scenes, "4boxes", w, h)
    centre = cams.pinhole(cam, w, h, 1, 0)                     # region: pixels whose rays all land well inside the face (|x|, |y| <= 0.7 at t = 5)
    tuv, prim = a.intersect_rays(centre)
    at = centre[:, :3] + 5.0 * centre[:, 3:]
    inside = (prim != MISS) & (np.abs(tuv[:, 0] - 5.0) < 1e-3) & (np.abs(at[:, 0]) <= 0.7) & (np.abs(at[:, 1]) <= 0.7)
    assert 60 <= inside.sum() <= w * h // 2

    def mean_image(rays):
        a.film.clear()
        a.render_rays(rays, spp)
        return a.film.get_pixels().astype(np.float64).sum(axis=1)

    pin_rays, lens_rays = cams.pinhole(cam, w, h, spp, 11), cams.thin_lens(cam, w, h, spp, 11, radius, 5.0)
    pin1 = mean_image(pin_rays)
    pin2 = mean_image(cams.pinhole(cam, w, h, spp, 12))
    lens = mean_image(lens_rays)
    noise = abs(pin1[inside].mean() - pin2[inside].mean())
    shift = lens[inside].mean() - pin1[inside].mean()
    model = phong_direct_sum(lens_rays, spp, w * h)[inside].mean() - phong_direct_sum(pin_rays, spp, w * h)[inside].mean()
    print("thin lens: region of %d pixels, pinhole means %.6f / %.6f (noise %.3g), lens mean %.6f (shift %.3g, the Phong model's %.3g)"
          % (inside.sum(), pin1[inside].mean(), pin2[inside].mean(), noise, lens[inside].mean(), shift, model))
    assert pin1[inside].mean() > 0.0 and noise > 0.0
    assert abs(shift) <= 3.0 * noise
    assert abs(shift - model) <= 1e-4
    assert np.any(bits(lens_rays) != bits(pin_rays))
    blurred = mean_image(cams.thin_lens(cam, w, h, spp, 11, 0.3, 2.5))      # a blur circle of 0.3 world units, 2.7 pixels, at the face
    empty = pin1 == 0.0
    assert empty.sum() > 50 and (blurred[empty] > 0.0).sum() >= 8           # the face's edge spilled into empty pixels
    a.film.clear()
    a.close()


# ---- 11. CLI ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_ortho_width(pkg, cams, scenes, tmp_path):
    exe = os.path.join(ROOT, "raytracer-rs_amd", "bin", "raytracer")
    w, h = 64, 48
    base = [exe, "-f", os.path.join(SCENES, "4boxes.scene"), "--width", str(w), "--height", str(h), "--seed", "17", "--spp", "4"]
    out = tmp_path / "x.png"
    r = subprocess.run(base + ["--ortho-width", "9.5", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rt = pkg.create_raytracer_from_arrays(scenes("4boxes"), pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=17)
    c = rt.render_rays(cams.orthographic(rt.camera.matrices(), w, h, 4, 17, 9.5), 4)
    want = rt.get_tonemapped_pixels()
    assert 0 < c.primary_hits < c.primary                     # the view shows something and not only that
    assert read_png(out)[:2] == (w, h) and np.array_equal(read_png(out)[2], rgb_of(want))
    # without the option the CLI writes what it always wrote
    plain = tmp_path / "y.png"
    r = subprocess.run(base + ["--out", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rt.film.clear()
    rt.render(4)
    assert np.array_equal(read_png(plain)[2], rgb_of(rt.get_tonemapped_pixels())) and not np.array_equal(rt.get_tonemapped_pixels(), want)
    r = subprocess.run(base[:-2] + ["--ortho-width", "9.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--ortho-width needs --spp" in r.stderr
    rt.close()
