"""The proofs that were sharpened together — finer depth maps around the lights (MI355RT_LIGHT_MAP_RES: 512 shipped, 1024 and 2048 behind the switch), 16 bins
per face edge in the reflection masks (MI355RT_REFLECT_MASK_BINS: 16 shipped, 8 behind the switch) and the culling verdicts cached per pixel block
(MI355RT_NO_CULL_CACHE) — only ever remove work whose outcome is known: every film, every packed pixel and every ray counter but the two that count
the rays never made (shadow_skipped, bounce_skipped) is the same bit for bit under every setting, and equals the CPU oracle's.

The switches are read when a handle is created, so every setting runs the same battery of renders in a fresh child process (this file, run as a script, is
that child); the children of all settings run side by side, once per session."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SETTINGS = {
    "default": {},
    "L512": {"MI355RT_LIGHT_MAP_RES": "512"},
    "L1024": {"MI355RT_LIGHT_MAP_RES": "1024"},
    "L2048": {"MI355RT_LIGHT_MAP_RES": "2048"},
    "B8": {"MI355RT_REFLECT_MASK_BINS": "8"},
    "B16": {"MI355RT_REFLECT_MASK_BINS": "16"},
    "NOCACHE": {"MI355RT_NO_CULL_CACHE": "1"},
}
SWITCHES = sorted({k for env in SETTINGS.values() for k in env})
SEMANTICS = ("reference_default", "true_closest")
# 96x40 x 3: sample groups of one sample (3 has no power-of-two divisor), 15 chunks of 256; 64x48 x 8: groups of 8, 12 pixel blocks in one sample group
FRAMES = [(name, w, h, spp, sem) for name in ("ico2", "thai2") for (w, h, spp) in ((96, 40, 3), (64, 48, 8)) for sem in SEMANTICS]
SEED = 9
MOVE = ((0.3, -0.1, 0.4), 0.12, -0.05)          # move_rel, add_y_angle, add_x_angle: far enough that other pixel blocks are live afterwards
EDGE_YAW = 0.33                                 # the 24x8 image: the object leaves the image at the edge
COUNTERS = ("primary", "bounce", "shadow", "primary_hits", "primary_culled", "shadow_skipped", "bounce_skipped")


def frame_key(name, w, h, spp, sem):
    return "%s_%dx%dx%d_%s" % (name, w, h, spp, sem)


def move(cam):
    cam.move_rel(*MOVE[0]); cam.add_y_angle(MOVE[1]); cam.add_x_angle(MOVE[2])


# ---- the child: one setting (its switches are in the environment), the whole battery ---------------------------------
def battery(out_path):
    sys.path.insert(0, ROOT)
    import importlib
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    scenes = {n: scene_io.load_scene_file(os.path.join(ge.SCENES, n + ".scene")) for n in ("ico2", "thai2")}
    flags = {"reference_default": 0, "true_closest": pkg.FLAG_TRUE_CLOSEST_HIT}
    out = {}

    def keep(key, rt, c):
        s, q, n = rt.film.pixel_datas()
        out[key + ".sum"] = np.ascontiguousarray(s, np.float32).view(np.uint32); out[key + ".sumsq"] = np.ascontiguousarray(q, np.float32).view(np.uint32)
        out[key + ".n"] = np.asarray(n, np.uint32); out[key + ".ldr"] = np.asarray(rt.get_tonemapped_pixels(), np.uint32)
        out[key + ".counts"] = np.asarray([getattr(c, k) for k in COUNTERS], np.uint64)

    for name, w, h, spp, sem in FRAMES:
        rt = pkg.create_raytracer_from_arrays(scenes[name], pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=SEED, flags=flags[sem])
        if name == "thai2" and w == 64 and sem == "reference_default":
            out["mask_bins"] = np.asarray([rt.reflect_mask_info()["bins"]], np.uint32)
        keep(frame_key(name, w, h, spp, sem), rt, rt.render(spp))
        if w == 64:
            # a camera move between two renders of one handle: the cached verdicts are the old camera's
            move(rt.camera)
            keep(frame_key(name, w, h, spp, sem) + ".moved", rt, rt.render(spp))
        del rt
    # a striped handle: 2-row stripes, rank 1 of 2 (20 rows of 96 pixels, 8 spp: 60 pixel blocks); a move; then 3 spp, where chunks do not hold whole blocks
    rt = pkg.create_raytracer_from_arrays(scenes["thai2"], pkg.DEFAULT_TRIANGLES_PER_LEAF, 96, 40, seed=SEED, stripe_rows=2, stripe_rank=1, stripe_world=2)
    out["stripe.rows"] = np.asarray(rt.owned_rows(), np.uint32)
    keep("stripe.a", rt, rt.render(8))
    move(rt.camera)
    keep("stripe.b", rt, rt.render(8))
    keep("stripe.c", rt, rt.render(3))
    del rt
    # fewer pixels than a chunk has samples (24x8 = 192): 8 spp makes 6 pixel blocks; 3 spp has no cached verdicts
    for name in ("ico2", "thai2"):
        rt = pkg.create_raytracer_from_arrays(scenes[name], pkg.DEFAULT_TRIANGLES_PER_LEAF, 24, 8, seed=SEED)
        rt.camera.add_y_angle(EDGE_YAW)
        keep("tiny.%s.a" % name, rt, rt.render(8))
        keep("tiny.%s.b" % name, rt, rt.render(3))
        del rt
    np.savez(out_path, **out)


if __name__ == "__main__":
    battery(sys.argv[1])
    sys.exit(0)


# ---- the tests ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(pkg, tmp_path_factory):
    """every setting's battery, each in a child process of its own, all started together"""
    d = tmp_path_factory.mktemp("proofs")
    procs = {}
    for name, extra in SETTINGS.items():
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(extra); env["MI355RT_DEBUG_CULL"] = "1"
        with open(str(d / (name + ".log")), "w") as log:          # (a file, not a pipe: nobody reads while the children run)
            procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / (name + ".npz"))], env=env, stdout=log, stderr=subprocess.STDOUT)
    out = {}
    try:
        for name, p in procs.items():
            code = p.wait(timeout=600)
            with open(str(d / (name + ".log"))) as log:
                err = log.read()
            assert code == 0, (name, err[-2000:])
            out[name] = (dict(np.load(str(d / (name + ".npz")))), err)
    finally:
        # a child that failed or ran out of time takes its siblings with it: nothing of this fixture stays on the GPU
        for p in procs.values():
            if p.poll() is None:
                p.kill()
        for p in procs.values():
            p.wait()
    return out


@pytest.fixture(scope="module")
def expected(oracle, scenes):
    """the oracle's films and counters of the whole battery, computed once"""
    flags = {"reference_default": 0, "true_closest": oracle.FLAG_BRUTE_FORCE}
    out = {}

    def keep(key, orc, c):
        s, q, n = orc.film()
        out[key] = (s.view(np.uint32).copy(), q.view(np.uint32).copy(), n.copy(), orc.get_tonemapped_pixels().copy(), (c["primary"], c["bounce"], c["shadow"], c["primary_hits"]))

    def omove(orc):
        orc.camera_move_rel(*MOVE[0]); orc.camera_add_y_angle(MOVE[1]); orc.camera_add_x_angle(MOVE[2])

    for name, w, h, spp, sem in FRAMES:
        orc = oracle.Oracle(scenes(name), w, h, seed=SEED, flags=flags[sem])
        keep(frame_key(name, w, h, spp, sem), orc, orc.render(spp, nthreads=8))
        if w == 64:
            omove(orc)
            keep(frame_key(name, w, h, spp, sem) + ".moved", orc, orc.render(spp, nthreads=8))
    orc = oracle.Oracle(scenes("thai2"), 96, 40, seed=SEED)
    keep("stripe.a", orc, orc.render(8, nthreads=8))
    omove(orc)
    keep("stripe.b", orc, orc.render(8, nthreads=8))
    keep("stripe.c", orc, orc.render(3, nthreads=8))
    for name in ("ico2", "thai2"):
        orc = oracle.Oracle(scenes(name), 24, 8, seed=SEED)
        orc.camera_add_y_angle(EDGE_YAW)
        keep("tiny.%s.a" % name, orc, orc.render(8, nthreads=8))
        keep("tiny.%s.b" % name, orc, orc.render(3, nthreads=8))
    return out


def keys_of(run):
    return sorted(k[:-len(".counts")] for k in run if k.endswith(".counts"))


def counts(run, key):
    return dict(zip(COUNTERS, (int(x) for x in run[key + ".counts"])))


def assert_same_frames(a, b, what):
    assert keys_of(a) == keys_of(b)
    for key in keys_of(a):
        for plane in ("sum", "sumsq", "n", "ldr"):
            assert np.array_equal(a[key + "." + plane], b[key + "." + plane]), (what, key, plane)
        ca, cb = counts(a, key), counts(b, key)
        for k in COUNTERS:
            if k not in ("shadow_skipped", "bounce_skipped"):
                assert ca[k] == cb[k], (what, key, k, ca, cb)


def test_the_switches_are_read(runs):
    for name, res in (("L512", 512), ("L1024", 1024), ("L2048", 2048)):
        assert "%u texels per face edge" % res in runs[name][1]
        assert runs[name][0]["mask_bins"][0] == runs["default"][0]["mask_bins"][0]
    assert runs["B8"][0]["mask_bins"][0] == 8 and runs["B16"][0]["mask_bins"][0] == 16
    assert "16 bins per face edge" in runs["B16"][1] and "16 bins per face edge" not in runs["B8"][1]


def test_light_map_resolutions_never_change_a_frame(runs):
    assert_same_frames(runs["L512"][0], runs["L1024"][0], "512 / 1024")
    assert_same_frames(runs["L512"][0], runs["L2048"][0], "512 / 2048")
    # a finer texel sees a part of what its parent sees: on thai2 no frame loses a proof, and the frames together gain some
    gained = 0
    for key in keys_of(runs["L512"][0]):
        if "thai2" in key or key.startswith("stripe"):
            s = [counts(runs[k][0], key)["shadow_skipped"] for k in ("L512", "L1024", "L2048")]
            b = [counts(runs[k][0], key)["bounce_skipped"] for k in ("L512", "L1024", "L2048")]
            print(key, "shadow_skipped", s, "of", counts(runs["L512"][0], key)["shadow"])
            assert s[0] <= s[1] <= s[2], (key, s)
            assert b[0] == b[1] == b[2], (key, b)
            gained += s[2] - s[0]
    assert gained > 0


def test_mask_bins_never_change_a_frame(runs):
    assert_same_frames(runs["B8"][0], runs["B16"][0], "8 / 16 bins")
    gained = 0
    for key in keys_of(runs["B8"][0]):
        if "thai2" in key or key.startswith("stripe"):
            c8, c16 = counts(runs["B8"][0], key), counts(runs["B16"][0], key)
            print(key, "bounce_skipped", c8["bounce_skipped"], c16["bounce_skipped"], "of", c8["bounce"])
            assert c8["bounce_skipped"] <= c16["bounce_skipped"], key
            assert c8["shadow_skipped"] == c16["shadow_skipped"], key      # (the reflection rays never made hit nothing: the shadow rays are the same)
            gained += c16["bounce_skipped"] - c8["bounce_skipped"]
    assert gained > 0


def test_cached_verdicts_never_change_a_frame(runs):
    a, b = runs["default"][0], runs["NOCACHE"][0]
    assert_same_frames(a, b, "NOCACHE")
    for key in keys_of(a):
        assert counts(a, key) == counts(b, key), key                         # here the two skipped counters agree as well
    # chunks were culled, on the full and on the striped handle
    for key in (frame_key("thai2", 64, 48, 8, "reference_default"), "stripe.a"):
        assert counts(a, key)["primary_culled"] > 0, key


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_every_setting_matches_the_oracle(runs, expected, setting):
    run = runs[setting][0]
    assert keys_of(run) == sorted(expected)
    rows = run["stripe.rows"]
    for key in keys_of(run):
        s, q, n, ldr, c = expected[key]
        got = counts(run, key)
        if key.startswith("stripe"):
            w = 96
            for plane, ref in (("sum", s.reshape(-1, w, 3)), ("sumsq", q.reshape(-1, w, 3)), ("n", n.reshape(-1, w))):
                assert np.array_equal(run[key + "." + plane].reshape(ref.shape)[rows], ref[rows]), (setting, key, plane)
            assert int(run[key + ".n"].sum()) == int(n.reshape(-1, w)[rows].sum())      # nothing outside the handle's rows
            continue
        assert np.array_equal(run[key + ".n"], n), (setting, key)
        assert np.array_equal(run[key + ".sum"].reshape(s.shape), s), (setting, key)
        assert np.array_equal(run[key + ".sumsq"].reshape(q.shape), q), (setting, key)
        assert np.array_equal(run[key + ".ldr"], ldr), (setting, key)
        assert (got["primary"], got["bounce"], got["shadow"], got["primary_hits"]) == c, (setting, key, got, c)
    # the object at the edge of the small image: some pixels hit it, most do not
    for name in ("ico2", "thai2"):
        got = counts(run, "tiny.%s.a" % name)
        assert 0 < got["primary_hits"] < got["primary"] // 2, (name, got)
