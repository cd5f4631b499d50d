"""Whole frames on scenes far from the origin, and under lights far from the scene, held to the CPU oracle bit for bit.

Every shortcut of the render path rests on a padding that is a fraction of the scene's diagonal and knows nothing of the size of the coordinates
(DESIGN.md §3a): the BVH's boxes, the lights' depth maps and tail2, the reflection masks, the cull rectangles, the coverage mask, the tile bins.  The
cases of tests/far_cases.py move 4boxes and ico2 up to 60 000 units away (camera and lights along) and carry light 0 up to 1e4 diagonals off.  For every
case the film sums, sums of squares, counts, packed pixels and the four ray counters of

  37 x 21 at 3 samples per pixel (sample groups of one, four chunks, the last one partial, no cached verdicts),
  64 x 48 at 8 (groups of eight: tile bins and cached block verdicts), rendered again on the same handle after a camera move,
  three trace_frame_additive calls on a 64 x 48 handle (the fused 50-row kernel),

in reference_default and true_closest, the closest hits and the shadow predicate of 4 096 rays (half random, half aimed next to triangle edges) in all
three semantics, and the denoiser's guide buffers equal the oracle's.  One translated case is also built on the device (FLAG_DEVICE_LBVH).

To tell WHICH shortcut is wrong when something differs, the whole battery runs under the default settings and with one shortcut off at a time.  The
switches are read when a handle is created, so every setting is a child process of its own (this file, run as a script), all started together, once per
session; a failure names the case, the frame, the semantics, the first differing pixel and the settings that do agree with the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import far_cases as fc  # noqa: E402
from test_gpu_proofs import MOVE, move  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = {
    "default": {},
    "NO_LIGHT_MAP": {"MI355RT_NO_LIGHT_MAP": "1"},
    "NO_REFLECT_MASK": {"MI355RT_NO_REFLECT_MASK": "1"},
    "NO_CULL": {"MI355RT_NO_CULL": "1"},
    "NO_CULL_MASK": {"MI355RT_NO_CULL_MASK": "1"},
    "NO_RASTER": {"MI355RT_NO_RASTER": "1"},
    "NO_CULL_CACHE": {"MI355RT_NO_CULL_CACHE": "1"},
}
SWITCHES = sorted({k for env in SETTINGS.values() for k in env})
SEMANTICS = ("reference_default", "true_closest")
SEMANTICS3 = ("reference_default", "octree_walk", "true_closest")
SMALL = (37, 21, 3)
LARGE = (64, 48, 8)
SEED = 9
N_RAYS = 4096
MISS = 0xFFFFFFFF
PLANES = ("sum", "sumsq", "n", "ldr", "counts")
CASE_KEYS = [c[0] for c in fc.GPU_CASES]


def case_rays(scene, seed):
    """N_RAYS rays with origins within two diagonals of the scene's box: half random (origins in the box widened by one unit, as
    tests/test_gpu_wide_variant.py draws them), half aimed at a point of a triangle one of whose barycentrics was multiplied by 1e-3 — next to an edge"""
    rng = np.random.default_rng(seed)
    lo, hi, diag = fc.box_of(scene)
    half = N_RAYS // 2
    o1 = rng.uniform(lo - 1.0, hi + 1.0, (half, 3))
    d1 = rng.normal(size=(half, 3))
    v = np.asarray(scene["tri_verts"], np.float64).reshape(-1, 3, 3)
    t = rng.integers(0, v.shape[0], half)
    b = rng.uniform(0.05, 1.0, (half, 3))
    b[np.arange(half), rng.integers(0, 3, half)] *= 1e-3
    b /= b.sum(1, keepdims=True)
    target = (b[:, :, None] * v[t]).sum(1)
    o2 = rng.uniform(lo - diag, hi + diag, (half, 3)).astype(np.float32).astype(np.float64)
    d2 = target - o2
    return np.concatenate([np.concatenate([o1, d1], 1), np.concatenate([o2, d2], 1)]).astype(np.float32)


def scene_of(base, key):
    _, name, offset, diagonals = next(c for c in fc.GPU_CASES if c[0] == key)
    sc = fc.case_scene(base(name), offset, diagonals)
    assert fc.is_finite(sc), key                                     # nothing non-finite ever reaches a tracing call
    return sc


def film_planes(out, key, s, q, n, ldr, counts):
    out[key + ".sum"] = np.ascontiguousarray(s, np.float32).reshape(-1).view(np.uint32).copy()
    out[key + ".sumsq"] = np.ascontiguousarray(q, np.float32).reshape(-1).view(np.uint32).copy()
    out[key + ".n"] = np.asarray(n, np.uint32).reshape(-1).copy()
    out[key + ".ldr"] = np.asarray(ldr, np.uint32).reshape(-1).copy()
    if counts is not None:
        out[key + ".counts"] = np.asarray(counts, np.uint64)


def ray_planes(out, key, tuv, prim, occ):
    tuv = np.array(tuv, np.float32, copy=True)
    tuv[prim == MISS] = 0.0                                          # a miss has no t, u, v
    out[key + ".prim"] = np.asarray(prim, np.uint32).copy()
    out[key + ".tuv"] = tuv.reshape(-1).view(np.uint32)
    out[key + ".occ"] = np.asarray(occ, np.uint8).astype(bool)


def guide_planes(out, key, g):
    out[key + ".gprim"] = np.asarray(g["prim"], np.uint32).copy()
    for k in ("depth", "normal", "albedo"):
        out[key + ".g" + k] = np.ascontiguousarray(g[k], np.float32).reshape(-1).view(np.uint32).copy()


# ---- the child: one setting (its switches are in the environment), the whole battery ---------------------------------
def battery(out_path):
    sys.path.insert(0, ROOT)
    import importlib
    import __graft_entry__ as ge
    pkg = ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    loaded = {}

    def base(name):
        if name not in loaded:
            loaded[name] = scene_io.load_scene_file(os.path.join(ge.SCENES, name + ".scene"))
        return loaded[name]

    flags = {"reference_default": 0, "octree_walk": pkg.FLAG_OCTREE_SEMANTICS, "true_closest": pkg.FLAG_TRUE_CLOSEST_HIT}
    out = {}

    def keep(key, rt, c):
        s, q, n = rt.film.pixel_datas()
        film_planes(out, key, s, q, n, rt.get_tonemapped_pixels(), (c.primary, c.bounce, c.shadow, c.primary_hits) if c is not None else None)
        if c is not None:
            out[key + ".skips"] = np.asarray([c.shadow_skipped, c.bounce_skipped, c.primary_culled], np.uint64)

    def frames(sc, prefix, sem, extra):
        (w, h, spp) = SMALL
        rt = pkg.create_raytracer_from_arrays(sc, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=SEED, flags=flags[sem] | extra)
        if extra:
            assert rt.bvh_build_info()["on_device"], pkg.lib().mi355rt_last_error(rt._h).decode()
        keep("%s|%dx%dx%d|%s" % (prefix, w, h, spp, sem), rt, rt.render(spp))
        del rt
        (w, h, spp) = LARGE
        rt = pkg.create_raytracer_from_arrays(sc, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=SEED, flags=flags[sem] | extra)
        keep("%s|%dx%dx%d|%s" % (prefix, w, h, spp, sem), rt, rt.render(spp))
        move(rt.camera)                                              # the cached verdicts and the bins are the old camera's
        keep("%s|%dx%dx%d.moved|%s" % (prefix, w, h, spp, sem), rt, rt.render(spp))
        del rt

    for key in CASE_KEYS:
        sc = scene_of(base, key)
        rays = case_rays(sc, SEED)
        for sem in SEMANTICS:
            frames(sc, key, sem, 0)
            rt = pkg.create_raytracer_from_arrays(sc, pkg.DEFAULT_TRIANGLES_PER_LEAF, LARGE[0], LARGE[1], seed=SEED, flags=flags[sem])
            for _ in range(3):                                       # the drop-in loop's 50-row frames: the fused kernel
                rt.trace_frame_additive()
            keep("%s|additive|%s" % (key, sem), rt, None)
            del rt
        for sem in SEMANTICS3:
            rt = pkg.create_raytracer_from_arrays(sc, pkg.DEFAULT_TRIANGLES_PER_LEAF, SMALL[0], SMALL[1], seed=SEED, flags=flags[sem])
            guide_planes(out, "%s|guides|%s" % (key, sem), rt.guides())
            tuv, prim = rt.intersect_rays(rays)
            ray_planes(out, "%s|rays|%s" % (key, sem), tuv, prim, rt.occluded_rays(rays))
            del rt
        if key == fc.LBVH_CASE:
            for sem in SEMANTICS:
                frames(sc, key + " lbvh", sem, pkg.FLAG_DEVICE_LBVH)
    np.savez(out_path, **out)


if __name__ == "__main__":
    battery(sys.argv[1])
    sys.exit(0)


# ---- the tests ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def children(pkg, tmp_path_factory):
    """every setting's battery, each in a child process of its own, all started together (seven: below the sixteen processes a GPU serves)"""
    d = tmp_path_factory.mktemp("far")
    procs = {}
    try:
        for name, extra in SETTINGS.items():
            env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            env.update(extra)
            with open(str(d / (name + ".log")), "w") as log:      # (a file, not a pipe: nobody reads while the children run)
                procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / (name + ".npz"))], env=env, stdout=log, stderr=subprocess.STDOUT)
        yield d, procs
    finally:
        # a child that failed or ran out of time takes its siblings with it: nothing of this fixture stays on the GPU
        for p in procs.values():
            if p.poll() is None:
                p.kill()
        for p in procs.values():
            p.wait()


@pytest.fixture(scope="module")
def runs(children, expected):
    """what the children wrote, by setting (`expected` is asked for first: the oracle's side is computed while the children run)"""
    d, procs = children
    out = {}
    try:
        for name, p in procs.items():
            code = p.wait(timeout=600)
            with open(str(d / (name + ".log"))) as log:
                err = log.read()
            assert code == 0, (name, err[-2000:])
            out[name] = dict(np.load(str(d / (name + ".npz"))))
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
        for p in procs.values():
            p.wait()
    return out


@pytest.fixture(scope="module")
def expected(children, oracle, scenes):
    """the oracle's side of the whole battery, computed once: the same keys and planes as a child writes"""
    from test_gpu_denoise import oracle_guides
    oflags = {"reference_default": 0, "octree_walk": 0, "true_closest": oracle.FLAG_BRUTE_FORCE}
    out = {}

    def keep(key, orc, c):
        s, q, n = orc.film()
        film_planes(out, key, s, q, n, orc.get_tonemapped_pixels(), (c["primary"], c["bounce"], c["shadow"], c["primary_hits"]) if c is not None else None)

    for key in CASE_KEYS:
        sc = scene_of(scenes, key)
        rays = case_rays(sc, SEED)
        for sem in SEMANTICS3:
            brute = sem == "true_closest"
            (w, h, spp) = SMALL
            orc = oracle.Oracle(sc, w, h, seed=SEED, flags=oflags[sem])
            guide_planes(out, "%s|guides|%s" % (key, sem), oracle_guides(orc, sc, w, h, False, brute))
            tuv, prim = orc.intersect(rays, brute=brute)
            ray_planes(out, "%s|rays|%s" % (key, sem), tuv, prim, (prim != MISS) & (tuv[:, 0] > np.float32(0.01)) & (tuv[:, 0] < np.float32(1.0)))
            if sem == "octree_walk":
                continue
            prefixes = (key, key + " lbvh") if key == fc.LBVH_CASE else (key,)
            c = orc.render(spp, nthreads=8)
            for p in prefixes:
                keep("%s|%dx%dx%d|%s" % (p, w, h, spp, sem), orc, c)
            (w, h, spp) = LARGE
            orc = oracle.Oracle(sc, w, h, seed=SEED, flags=oflags[sem])
            c = orc.render(spp, nthreads=8)
            for p in prefixes:
                keep("%s|%dx%dx%d|%s" % (p, w, h, spp, sem), orc, c)
            orc.camera_move_rel(*MOVE[0]); orc.camera_add_y_angle(MOVE[1]); orc.camera_add_x_angle(MOVE[2])
            c = orc.render(spp, nthreads=8)
            for p in prefixes:
                keep("%s|%dx%dx%d.moved|%s" % (p, w, h, spp, sem), orc, c)
            orc = oracle.Oracle(sc, w, h, seed=SEED, flags=oflags[sem])
            for _ in range(3):
                orc.trace_frame_additive()
            keep("%s|additive|%s" % (key, sem), orc, None)
    return out


def where(name, i, want):
    """the first differing element in words a reader can use"""
    case, frame, sem = name.rsplit(".", 1)[0].split("|")
    plane = name.rsplit(".", 1)[1]
    if frame in ("rays", "guides"):
        per = max(want.size // (N_RAYS if frame == "rays" else SMALL[0] * SMALL[1]), 1)
        return "%s %d" % ("ray" if frame == "rays" else "pixel", i // per)
    if plane == "counts":
        return "counter %s" % ("primary", "bounce", "shadow", "primary_hits")[i]
    w, h = (SMALL if frame.startswith("%dx%d" % SMALL[:2]) else LARGE)[:2]
    p = i // max(want.size // (w * h), 1)
    return "pixel %d (x %d, y %d)" % (p, p % w, p // w)


def differences(runs, expected, prefix):
    """one line per plane of the case (or the lbvh frames) that some setting gets wrong: which, where first, and who agrees"""
    lines = []
    for name in sorted(k for k in expected if k.split("|")[0] == prefix):
        want = expected[name]
        agree, differ, first = [], [], None
        for setting in SETTINGS:
            got = runs[setting].get(name)
            if got is not None and got.shape == want.shape and np.array_equal(got, want):
                agree.append(setting)
            else:
                differ.append(setting)
                if first is None and got is not None and got.shape == want.shape:
                    i = int(np.nonzero(got != want)[0][0])
                    first = "%s: %s has %r, the oracle %r; %d of %d elements differ" % (where(name, i, want), setting, got[i], want[i], int((got != want).sum()), want.size)
        if differ:
            case, frame, sem = name.rsplit(".", 1)[0].split("|")
            lines.append("case %s, frame %s, %s, plane %s: %s.  Differ: %s.  Agree with the oracle: %s" % (
                case, frame, sem, name.rsplit(".", 1)[1], first or "missing or another shape", ", ".join(differ), ", ".join(agree) or "none"))
    return lines


def test_the_children_wrote_what_the_oracle_wrote(runs, expected):
    for setting in SETTINGS:
        assert sorted(k for k in runs[setting] if not k.endswith(".skips")) == sorted(expected), setting


@pytest.mark.parametrize("key", CASE_KEYS)
def test_every_setting_equals_the_oracle(runs, expected, key):
    """films, packed pixels, the four counters, hit records, the shadow predicate and the guides of one case, under every setting"""
    share = {}
    for sem in SEMANTICS:
        primary, bounce, shadow, hits = (int(x) for x in expected["%s|%dx%dx%d|%s.counts" % ((key,) + LARGE + (sem,))])
        share[sem] = hits / primary
        # the case does look at the object, and at more than the object
        assert 0.15 <= share[sem] <= 0.95, (key, sem, share)
        assert shadow > 0 and bounce > 0, (key, sem, shadow, bounce)
        prim = expected["%s|rays|%s.prim" % (key, sem)]
        assert 0.05 < float((prim != MISS).mean()) < 0.95, (key, sem)
    skips = {f: [int(x) for x in runs["default"]["%s|%s|reference_default.skips" % (key, f)]] for f in ("%dx%dx%d" % SMALL, "%dx%dx%d" % LARGE)}
    lines = differences(runs, expected, key)
    print("\n[%s] oracle hit share %r; default setting, reference_default: (shadow_skipped, bounce_skipped, primary_culled) %r; %s" % (
        key, {k: round(v, 3) for k, v in share.items()}, skips, "every setting agrees" if not lines else "%d planes differ" % len(lines)))
    assert not lines, "\n" + "\n".join(lines[:40])


def test_device_built_tree_far_away_equals_the_oracle(runs, expected):
    lines = differences(runs, expected, fc.LBVH_CASE + " lbvh")
    assert any(k.split("|")[0] == fc.LBVH_CASE + " lbvh" for k in expected)
    assert not lines, "\n" + "\n".join(lines[:40])


def test_the_shortcuts_were_engaged(runs):
    """at the origin the shortcuts do remove work under the default setting and not with their switch set: the settings are what they say"""
    key = "ico2+0|%dx%dx%d|reference_default.skips" % LARGE
    shadow_skipped, bounce_skipped, culled = (int(x) for x in runs["default"][key])
    assert shadow_skipped > 0 and bounce_skipped > 0 and culled > 0, (shadow_skipped, bounce_skipped, culled)
    assert int(runs["NO_LIGHT_MAP"][key][0]) == 0 and int(runs["NO_REFLECT_MASK"][key][1]) == 0 and int(runs["NO_CULL"][key][2]) == 0
