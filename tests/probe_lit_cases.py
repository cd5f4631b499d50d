"""Scenes, volumes and rays for probe-lit shading (include/mi355rt.h "PROBE-LIT"), shared by tests/test_probe_lit_abi.py (the host side of
csrc/probe_lit_math.hpp against the numpy statement, and the statement against the CPU oracle) and tests/test_gpu_probe_lit.py (the kernels against the same
statement).  Not a test module."""
import ctypes as C

import numpy as np

import probe_vis_cases as pv

F = np.float32
MISS = 0xFFFFFFFF
W, H = 16, 12
SEED = 5
FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)
# the lights tests/test_gpu_light_films.py adds to a scene's own first light (with_lights' recipe, written out again)
EXTRA_LIGHTS = np.array([[-3.0, 4.0, 2.0, 1.0, 0.25, 0.5], [0.5, -2.0, 6.0, 0.75, 1.5, 0.125], [4.0, 0.5, -1.5, 0.5, 0.5, 2.0], [-2.0, -3.0, -4.0, 2.0, 1.0, 0.0],
                         [2.0, 2.0, -6.0, 6.0, 0.5, 3.0], [-1.0, 7.0, 1.0, 1.0, 2.0, 7.0], [5.0, 5.0, 5.0, 2.5, 2.5, 2.5], [-6.0, 1.0, -1.0, 3.5, 0.25, 1.5]], F)
SCENES = ("4boxes", "ico3_tex", "4boxes_3lights")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def scene_of(scenes, name):
    """4boxes, ico3_tex, or 4boxes with three lights: its own first, then the first two of EXTRA_LIGHTS"""
    if name != "4boxes_3lights":
        return scenes(name)
    sc = dict(scenes("4boxes"))
    sc["lights"] = np.concatenate([sc["lights"][:1], EXTRA_LIGHTS])[:3].astype(F).copy()
    return sc


def offsets_for(grid, kind, seed=9):
    """None, zeros, or fixed-seed offsets within 0.4 of a cell"""
    counts = [int(c) for c in np.asarray(grid["counts"]).reshape(3)]
    nprobes = counts[0] * counts[1] * counts[2]
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros((nprobes, 3), F)
    sp = np.asarray(grid["spacing"], F).reshape(3)
    return np.ascontiguousarray((np.random.default_rng(seed).uniform(-0.4, 0.4, (nprobes, 3)) * sp[None, :]).astype(F))


def c_volume(pkg, vol):
    """(mi355rt_probe_volume over the host arrays of a probe_lit.volume dict, what it points to)"""
    g = pkg.ProbeGrid.from_dict(vol["grid"])
    n = np.ascontiguousarray(vol["n"], np.uint32); sh = np.ascontiguousarray(vol["sh"], F)
    keep = [g, n, sh]
    v = pkg.ProbeVolume()
    v.grid = C.pointer(g); v.n = n.ctypes.data; v.sh = sh.ctypes.data
    if vol["usable"] is not None:
        u = np.ascontiguousarray(vol["usable"], np.uint8); keep.append(u); v.usable = u.ctypes.data
    if vol["depth"] is not None:
        d = vol["depth"]
        cnt = np.ascontiguousarray(d["count"], np.uint32); mom = np.ascontiguousarray(d["moments"], F)
        pd = pkg.ProbeDepth(int(d["res"]), float(d["max_distance"]), cnt.ctypes.data, mom.ctypes.data)
        vc = pkg.ProbeVisConfig((1 if vol["chebyshev"] else 0) | (2 if vol["facing"] else 0), float(vol["normal_bias"]))
        keep += [cnt, mom, pd, vc]
        v.depth = C.pointer(pd); v.vc = C.pointer(vc)
        if vol["offsets"] is not None:
            o = np.ascontiguousarray(vol["offsets"], F); keep.append(o); v.offsets = o.ctypes.data
    return v, keep


def c_hemi(pkg, vol, points, normals, clamp=True):
    """one mi355rt_probe_lit_one call per query -> (indirect, ok)"""
    v, _keep = c_volume(pkg, vol)
    points = np.ascontiguousarray(points, F).reshape(-1, 3); normals = np.ascontiguousarray(normals, F).reshape(-1, 3)
    out = np.full((len(points), 3), np.nan, F); ok = np.zeros(len(points), np.uint8)
    one = C.c_uint32(99)
    fn = pkg.lib().mi355rt_probe_lit_one
    for q in range(len(points)):
        assert fn(C.byref(v), points[q].ctypes.data_as(FP), normals[q].ctypes.data_as(FP), 1 if clamp else 0, out[q].ctypes.data_as(FP), C.byref(one)) == 0
        ok[q] = one.value
    return out, ok


def lookup_volumes(plit):
    """(name, volume, points, normals) over every case of probe_vis_cases.lookup_cases(): NULL, zero and fixed-seed offsets, every flag combination (the
    normal_bias cycling through 0, 0.05 and -0.02), and once without depth films"""
    out = []
    for k, (name, g, res, depth, usable, pts, dirs, nrm) in enumerate(pv.lookup_cases()):
        for o, kind in enumerate((None, "zero", "seeded")):
            for f, (cheb, facing) in enumerate(pv.FLAGS):
                bias = (0.0, 0.05, -0.02)[(k + o + f) % 3]
                out.append(("%s off=%s cheb=%d facing=%d" % (name, kind, cheb, facing),
                            plit.volume(g, res, depth=depth, usable=usable, offsets=offsets_for(g, kind, 9 + k), chebyshev=cheb, facing=facing, normal_bias=bias), pts, nrm))
        out.append((name + " no depth", plit.volume(g, res, usable=usable), pts, nrm))
    return out


def hand_volume(plit, seed=3):
    """A 3x2x2 volume no gather makes: probes 1 and 8 have n == 0 and probe 6 is not usable, and all three hold infinities and NaNs in every coefficient
    and film texel — a skipped probe is never read, and one that were would show; every probe holds an infinity in coefficients 4 .. 8.  Negative coefficients
    are present, so the unclamped mean is negative for some queries."""
    rng = np.random.default_rng(seed)
    counts = (3, 2, 2)
    grid = dict(origin=np.array([-2.5, -1.0, -2.0], F), spacing=np.array([2.5, 3.0, 4.0], F), counts=np.array(counts, np.uint32))
    nprobes = 12
    n = rng.integers(1, 40, nprobes).astype(np.uint32)
    sh = (rng.normal(size=(nprobes, 9, 3)) * n[:, None, None]).astype(F)
    sh[:, 4:, :] = np.inf
    sh[::2, 6, 1] = np.nan
    usable = np.ones(nprobes, np.uint8)
    depth = pv.film(4, nprobes, 77, D=6.0)
    n[[1, 8]] = 0
    usable[6] = 0
    for p in (1, 6, 8):
        sh[p] = np.inf; sh[p, 1] = np.nan
        depth["moments"][p] = np.nan
    return plit.volume(grid, dict(n=n, sh=np.ascontiguousarray(sh)), depth=depth, usable=usable, offsets=offsets_for(grid, "seeded", 5), normal_bias=0.02)


def hand_rays(origin, inside):
    """rays that are data: misses, origins inside a box, a zero direction component, a zero direction, a NaN ray.  origin: the camera's position; inside: a
    point inside a box of the scene"""
    o, p = np.asarray(origin, F), np.asarray(inside, F)
    to = (p - o).astype(F)
    r = [np.concatenate([o, -to]), np.concatenate([o, [0.0, 1e3, 1.0]]),                       # misses
         np.concatenate([p, [1.0, 0.5, 0.25]]), np.concatenate([p, [-0.3, -1.0, 0.2]]), np.concatenate([p, to]),      # from inside a box
         np.concatenate([o, [to[0], 0.0, to[2]]]), np.concatenate([o, [0.0, to[1], to[2]]]), np.concatenate([o, [0.0, 0.0, to[2]]]),      # zero components
         np.concatenate([o, [0.0, 0.0, 0.0]]), np.concatenate([o, [-0.0, 0.0, -0.0]]),          # zero directions
         np.concatenate([o, [np.nan, 0.0, 1.0]]), np.concatenate([[np.nan, 0.0, 0.0], to]), np.full(6, np.nan),      # NaN rays
         np.concatenate([o, to]), np.concatenate([o, to * F(1e-3)]), np.concatenate([o, to * F(1e3)])]               # the same ray at three lengths
    return np.ascontiguousarray(np.array(r, F))
