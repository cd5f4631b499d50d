"""Gather without a GPU (include/mi355rt.h "GATHER"): the entry points and structs are what the header says, the host side of the shared walk
(mi355rt_gather_ray, csrc/gather_walk.hpp — the header gather_rays_kernel compiles) equals the numpy statement (raytracer_rs_amd.gather) bit for bit, the
walk is BOUNDED (a zero normal returns, void), and the statement's reduce accumulates as one shot does.  tests/test_gpu_gather.py runs the kernels; its void
test relies on what is shown here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_gather_default_config", "mi355rt_gather", "mi355rt_gather_ray"]
F = np.float32
SEED = 7


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ga(pkg):
    import importlib
    return importlib.import_module("raytracer_rs_amd.gather")


@pytest.fixture(scope="module")
def table(oracle, scenes):
    return oracle.Oracle(scenes("4boxes"), 8, 8, seed=SEED).sample_table()


def gather_ray(pkg, table, seed, point, normal, pid, sampleno):
    """mi355rt_gather_ray -> (ray6, valid)"""
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    point = np.ascontiguousarray(point, F)
    normal = None if normal is None else np.ascontiguousarray(normal, F)
    ray = np.full(6, np.nan, F); valid = C.c_uint32(99)
    assert pkg.lib().mi355rt_gather_ray(fp(table), seed, fp(point), None if normal is None else fp(normal), int(pid), int(sampleno), fp(ray), C.byref(valid)) == 0
    return ray, valid.value


def c_rays(pkg, table, seed, points, normals, ids, first, spp):
    """the layout of gather.rays() from one mi355rt_gather_ray call per sample"""
    n = len(points)
    rays = np.zeros((spp, n, 6), F); valid = np.zeros((spp, n), np.uint8)
    for s in range(spp):
        for i in range(n):
            rays[s, i], valid[s, i] = gather_ray(pkg, table, seed, points[i], None if normals is None else normals[i], i if ids is None else ids[i], first + s)
    return rays.reshape(-1, 6), valid


def test_gather_symbols_structs_and_defaults(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)
        assert re.search(r"\b%s\(" % name, header), name
    for name, value in (("MI355RT_GATHER_MEAN", pkg.GATHER_MEAN), ("MI355RT_GATHER_COSINE", pkg.GATHER_COSINE)):
        m = re.search(r"#define\s+%s\s+(\d+)u" % name, header)
        assert m and int(m.group(1)) == value, name
    assert pkg.GATHER_WEIGHTS == {"mean": 0, "cosine": 1}
    # typedef struct mi355rt_gather_config { uint32_t spp, first_sample, weight, accumulate; float near_distance; }: five 4-byte fields, no padding
    assert C.sizeof(pkg.GatherConfig) == 20
    assert [(n, getattr(pkg.GatherConfig, n).offset) for n, _ in pkg.GatherConfig._fields_] == [("spp", 0), ("first_sample", 4), ("weight", 8), ("accumulate", 12), ("near_distance", 16)]
    # typedef struct mi355rt_gather_outputs { uint32_t *n, *hits, *near; float *sum, *sumsq, *direct; }: six pointers
    assert C.sizeof(pkg.GatherOutputs) == 48
    assert [(n, getattr(pkg.GatherOutputs, n).offset) for n, _ in pkg.GatherOutputs._fields_] == [("n", 0), ("hits", 8), ("near", 16), ("sum", 24), ("sumsq", 32), ("direct", 40)]
    assert re.search(r"typedef struct mi355rt_gather_config\s*\{ uint32_t spp, first_sample, weight, accumulate; float near_distance; \}", header)
    assert re.search(r"typedef struct mi355rt_gather_outputs\s*\{ uint32_t \*n, \*hits, \*near; float \*sum, \*sumsq, \*direct; \}", header)
    cfg = pkg.GatherConfig(1, 2, 3, 4, 5.0)
    pkg.lib().mi355rt_gather_default_config(C.byref(cfg))
    assert (cfg.spp, cfg.first_sample, cfg.weight, cfg.accumulate) == (16, 0, pkg.GATHER_MEAN, 0)
    assert cfg.near_distance == float("inf")
    pkg.lib().mi355rt_gather_default_config(None)        # tolerated
    assert pkg.lib().mi355rt_gather(None, None, None, None, 0, C.byref(cfg), 0, None) == -1
    ray = np.zeros(6, F)
    assert pkg.lib().mi355rt_gather_ray(None, 0, ray.ctypes.data_as(C.POINTER(C.c_float)), None, 0, 0, ray.ctypes.data_as(C.POINTER(C.c_float)), None) == -1


def test_gather_ray_equals_the_statement(pkg, ga, table):
    rng = np.random.default_rng(11)
    n, spp, first = 64, 5, 3
    points = rng.uniform(-4, 4, (n, 3)).astype(F)
    normals = rng.normal(size=(n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1)[:, None]).astype(F)
    normals[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    ids = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    ids[10] = ids[11]; normals[11] = normals[10]         # same id, same normal: the same directions
    for nrm, use_ids in ((normals, ids), (normals, None), (None, ids)):
        rays, keys, valid, w = ga.rays(table, SEED, points, nrm, use_ids, first, spp)
        crays, cvalid = c_rays(pkg, table, SEED, points, nrm, use_ids, first, spp)
        assert np.array_equal(bits(rays), bits(crays))
        assert np.array_equal(valid, cvalid) and valid.all()
        want_ids = np.arange(n, dtype=np.uint32) if use_ids is None else use_ids
        assert keys.dtype == np.uint32 and np.array_equal(keys.reshape(spp, n, 2)[:, :, 0], np.broadcast_to(want_ids, (spp, n)))
        assert np.array_equal(keys.reshape(spp, n, 2)[:, :, 1], np.broadcast_to(first + np.arange(spp, dtype=np.uint32)[:, None], (spp, n)))
        d = rays.reshape(spp, n, 6)[:, :, 3:]
        start = ga.table_index(pkg_hash(pkg, keys, SEED))
        if nrm is None:                                  # sphere mode: the ray is the start entry
            assert np.array_equal(bits(d.reshape(-1, 3)), bits(table[start]))
        else:                                            # every accepted direction lies in the normal's hemisphere, in the walk's own arithmetic
            dots = d[..., 0] * nrm[None, :, 0] + d[..., 1] * nrm[None, :, 1] + d[..., 2] * nrm[None, :, 2]
            assert dots.dtype == F and (dots > 0).all()
            assert np.array_equal(bits(d[:, 10]), bits(d[:, 11])) == (use_ids is not None)      # the same id and normal: the same directions
            assert (w == 1).all()
            w2 = ga.rays(table, SEED, points, nrm, use_ids, first, spp, weight="cosine")[3]
            assert np.array_equal(bits(w2), bits(F(2.0) * dots))
        # origin = point + 0.00001f * d in f32
        o = rays.reshape(spp, n, 6)[:, :, :3]
        assert np.array_equal(bits(o), bits(points[None] + F(0.00001) * d))


def pkg_hash(pkg, keys, seed):
    import importlib
    cams = importlib.import_module("raytracer_rs_amd.cameras")
    return cams.pcg4d(keys[:, 0], keys[:, 1], np.uint32(0xFFFFFFFE), np.uint32(seed))[0]


def test_the_walk_is_bounded_void_and_nan(pkg, ga, table):
    """A zero normal never satisfies dot > 0: the walk stops after one full turn and the sample is void (valid 0), with the harmless ray of the start entry.
    (1e-45, 0, 0): the issue's candidate for a denormal normal whose products underflow.  Under IEEE f32 they do not all underflow: an entry with
    |x| > 0.5 times the smallest denormal rounds to the smallest denormal again, so the statement accepts the first entry with x > 0.5 — checked here as what
    the statement says, on both sides.  A NaN normal accepts the start entry."""
    p = np.array([1, 2, 3], F)
    for sampleno in range(4):
        start = int(ga.table_index(pkg_hash(pkg, np.array([[5, sampleno]], np.uint32), SEED))[0])
        for zero in ([0, 0, 0], [-0.0, 0.0, -0.0]):
            ray, valid = gather_ray(pkg, table, SEED, p, zero, 5, sampleno)
            srays, _, svalid, _ = ga.rays(table, SEED, p[None], np.array([zero], F), np.array([5], np.uint32), sampleno, 1)
            assert valid == 0 and svalid[0, 0] == 0
            assert np.array_equal(bits(ray), bits(srays[0])) and np.isfinite(ray).all()
            assert np.array_equal(bits(ray[3:]), bits(table[start]))
        tiny = np.array([1e-45, 0, 0], F)
        assert tiny[0] > 0 and tiny[0] == np.nextafter(F(0), F(1))
        ray, valid = gather_ray(pkg, table, SEED, p, tiny, 5, sampleno)
        srays, _, svalid, _ = ga.rays(table, SEED, p[None], tiny[None], np.array([5], np.uint32), sampleno, 1)
        assert valid == svalid[0, 0] == 1 and np.array_equal(bits(ray), bits(srays[0]))
        assert ray[3] * tiny[0] > 0 and ray[3] > 0.5
        # ... and every entry the walk passed over was rejected: its product is not positive
        j, steps = start, 0
        while not np.array_equal(bits(table[j]), bits(ray[3:])):
            assert not (table[j, 0] * tiny[0] + table[j, 1] * tiny[1] + table[j, 2] * tiny[2] > 0)
            j = (j + 1) % 65535; steps += 1
            assert steps < 65535
        ray, valid = gather_ray(pkg, table, SEED, p, [np.nan, 0, 0], 5, sampleno)
        srays, _, svalid, _ = ga.rays(table, SEED, p[None], np.array([[np.nan, 0, 0]], F), np.array([5], np.uint32), sampleno, 1)
        assert valid == svalid[0, 0] == 1 and np.array_equal(bits(ray), bits(srays[0]))
        assert np.array_equal(bits(ray[3:]), bits(table[start]))


def test_a_long_walk_ends_at_the_only_accepted_entry(pkg, ga):
    """A hand-made table in which exactly one entry of the walk's cycle lies in the normal's hemisphere: from every start the walk ends there, on both sides,
    however far it is (up to a full turn), and entry 65535, which the walk's modulus never reaches, is not taken."""
    t = np.zeros((65536, 3), F); t[:, 2] = -1
    t[65535] = [0, 0, 1]
    n = np.array([0, 0, 1], F); p = np.zeros(3, F)
    ray, valid = gather_ray(pkg, t, 1, p, n, 0, 0)
    srays, _, svalid, _ = ga.rays(t, 1, p[None], n[None], None, 0, 1)
    assert valid == 0 and svalid[0, 0] == 0 and np.array_equal(bits(ray), bits(srays[0]))
    for only in (0, 12345, 65534):
        t2 = t.copy(); t2[only] = [0.6, 0, 0.8]
        for pid in range(3):
            ray, valid = gather_ray(pkg, t2, 1, p, n, pid, 0)
            srays, _, svalid, _ = ga.rays(t2, 1, p[None], n[None], np.array([pid], np.uint32), 0, 1)
            assert valid == 1 and svalid[0, 0] == 1
            assert np.array_equal(bits(ray), bits(srays[0])) and np.array_equal(bits(ray[3:]), bits(t2[only]))


def test_the_mean_cosine_of_the_hemisphere_sampler(pkg, ga, table):
    """One fixed normal, 4096 samples: dot(d, n) of a uniform hemisphere has mean 1/2 and variance 1/12, so the mean of 4096 lies in 0.5 +- 4 sigma = 0.5 +- 0.018."""
    n = np.array([[0.6, 0.0, 0.8]], F)
    rays, keys, valid, w = ga.rays(table, SEED, np.zeros((1, 3), F), n, None, 0, 4096, weight="cosine")
    assert valid.all()
    d = rays[:, 3:].astype(np.float64)
    m = float((d @ n[0].astype(np.float64)).mean())
    print("mean of dot(d, n) over 4096 samples, seed %d: %.5f" % (SEED, m))
    assert abs(m - 0.5) <= 0.018
    assert abs(float(w.astype(np.float64).mean()) / 2 - m) < 1e-6
    crays, cvalid = c_rays(pkg, table, SEED, np.zeros((1, 3), F), n, None, 0, 256)
    assert np.array_equal(bits(crays), bits(rays[:256]))


def test_reduce_with_prev_equals_one_shot(ga):
    rng = np.random.default_rng(3)
    npts, spp = 7, 8
    rgb = rng.normal(size=(spp * npts, 3)).astype(F)               # negative values
    rgb[5] = [1e-40, -1e-42, 1e-45]                                 # denormals
    rgb[11] = [-0.0, 0.0, 1e-30]
    t = rng.uniform(0.1, 5, spp * npts).astype(F)
    hit = rng.random(spp * npts) < 0.6
    valid = (rng.random((spp, npts)) < 0.8).astype(np.uint8)
    valid[:, 2] = 0                                                 # a point whose every sample is void
    valid[:3, 4] = 0                                                # n crosses from 0 in the second call only
    w = rng.uniform(0, 2, (spp, npts)).astype(F)
    one = ga.reduce(rgb, t, hit, valid, w, 2.5)
    a = ga.reduce(rgb[:3 * npts], t[:3 * npts], hit[:3 * npts], valid[:3], w[:3], 2.5)
    assert a["n"][4] == 0 and a["n"][2] == 0
    keep = {k: v.copy() for k, v in a.items()}
    b = ga.reduce(rgb[3 * npts:], t[3 * npts:], hit[3 * npts:], valid[3:], w[3:], 2.5, prev=a)
    for k in keep:
        assert np.array_equal(keep[k], a[k]), k                    # prev is not written
    for k in ("n", "hits", "near"):
        assert b[k].dtype == np.uint32 and np.array_equal(b[k], one[k]), k
    for k in ("sum", "sumsq"):
        assert np.array_equal(bits(b[k]), bits(one[k])), k
    # by hand, point by point, in sample order
    for i in range(npts):
        s = np.zeros(3, F); q = np.zeros(3, F); n = h = nr = 0
        for k in range(spp):
            if not valid[k, i]:
                continue
            v = w[k, i] * rgb[k * npts + i]
            s = s + v; q = q + v * v; n += 1
            if hit[k * npts + i]:
                h += 1; nr += int(t[k * npts + i] < F(2.5))
        assert (one["n"][i], one["hits"][i], one["near"][i]) == (n, h, nr)
        assert np.array_equal(bits(one["sum"][i]), bits(s)) and np.array_equal(bits(one["sumsq"][i]), bits(q))
    assert one["n"][2] == 0 and not one["sum"][2].any()
    m = ga.mean(one)
    assert np.isnan(m[2]).all() and np.array_equal(bits(m[0]), bits(one["sum"][0] / F(one["n"][0])))
    assert np.array_equal(bits(ga.irradiance(one)[0]), bits(F(np.pi) * m[0]))


def test_shadow_rays_and_direct_by_hand(ga):
    pts = np.array([[0, 0, 0], [1, 0, 0]], F)
    nrm = np.array([[0, 0, 1], [0, 0, 1]], F)
    lights = np.array([[0, 0, 2, 1, 0.5, 0.25], [0, 0, -3, 9, 9, 9], [3, 0, 4, 0.5, 0.5, 0.5]], F)      # the second lies behind the surface: skipped
    sr = ga.shadow_rays(pts, lights)
    assert sr.shape == (6, 6)
    l = lights[2, :3] - pts[1]
    assert np.array_equal(bits(sr[2 * 2 + 1]), bits(np.concatenate([pts[1] + l * F(0.01), l])))
    blocked = np.zeros(6, np.uint8); blocked[2 * 2 + 0] = 1                                             # light 2 is blocked for point 0
    d = ga.direct(pts, nrm, lights, blocked)
    assert np.array_equal(bits(d[0]), bits(lights[0, 3:] * F(1.0)))
    ln = l / np.sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2])
    l0 = lights[0, :3] - pts[1]
    ln0 = l0 / np.sqrt(l0[0] * l0[0] + l0[1] * l0[1] + l0[2] * l0[2])
    want = (np.zeros(3, F) + lights[0, 3:] * (nrm[1, 0] * ln0[0] + nrm[1, 1] * ln0[1] + nrm[1, 2] * ln0[2])) + lights[2, 3:] * (nrm[1, 0] * ln[0] + nrm[1, 1] * ln[1] + nrm[1, 2] * ln[2])
    assert np.array_equal(bits(d[1]), bits(want))
