"""Probe placement without a GPU (include/mi355rt.h "PROBE PLACEMENT"): the entry points and structs are what the header says, the host side
of the shared arithmetic (mi355rt_probe_place_one, mi355rt_probes_lookup_placed_one: csrc/probe_place.hpp, the header the kernels compile) equals the numpy
statement (raytracer_rs_amd.probes) bit for bit on hand-made surveys, offsets and queries, and the statement itself is held to hand-written samples, to one
probe worked in Python floats, to the lookups it must collapse to, and to the outcomes it must have on four hand-made scenes traced by the CPU oracle.
tests/test_gpu_probes_place.py runs the kernels against the same statement."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import probe_cases as pc
import probe_place_cases as pp
import probe_vis_cases as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355rt_probes_survey_default_config", "mi355rt_probes_place_default_config", "mi355rt_probes_survey", "mi355rt_probes_place", "mi355rt_probe_place_one",
       "mi355rt_probes_lookup_placed", "mi355rt_probes_lookup_placed_one"]
F = np.float32
FP = C.POINTER(C.c_float)
UP = C.POINTER(C.c_uint32)
fp = lambda a: a.ctypes.data_as(FP)
up = lambda a: a.ctypes.data_as(UP)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pr(pkg):
    return importlib.import_module("raytracer_rs_amd.probes")


def c_place(pkg, grid, sv, offsets, back_share=0.25, max_offset=0.45, min_front=pp.MIN_FRONT):
    """one mi355rt_probe_place_one call per probe -> (offsets, verdict, state)"""
    g = pkg.ProbeGrid.from_dict(grid)
    cfg = pkg.ProbePlaceConfig(back_share, max_offset, min_front, float(sv["max_distance"]))
    nprobes = len(sv["n"])
    out = np.full((nprobes, 3), 7.0, F); verdict = np.zeros(nprobes, np.uint8); state = np.zeros(nprobes, np.uint8)
    v, s = C.c_uint32(99), C.c_uint32(99)
    for i in range(nprobes):
        counts = np.array([sv["n"][i], sv["back"][i], sv["front"][i]], np.uint32)
        recs = np.ascontiguousarray(np.concatenate([sv["near_back"][i], sv["near_front"][i], sv["far"][i]]), F)
        off = None if offsets is None else fp(np.ascontiguousarray(offsets[i]))
        assert pkg.lib().mi355rt_probe_place_one(C.byref(g), C.byref(cfg), up(counts), fp(recs), off, fp(out[i]), C.byref(v), C.byref(s)) == 0
        verdict[i], state[i] = v.value, s.value
    return out, verdict, state


def c_lookup_placed(pkg, g, res, depth, usable, offsets, points, dirs, nrm, mode, cheb, facing, bias):
    """one mi355rt_probes_lookup_placed_one call per query -> (rgb, ok)"""
    grid = pkg.ProbeGrid.from_dict(g)
    n = np.ascontiguousarray(res["n"], np.uint32); sh = np.ascontiguousarray(res["sh"], F)
    d = pkg.ProbeDepth(int(depth["res"]), float(depth["max_distance"]), depth["count"].ctypes.data, depth["moments"].ctypes.data)
    vc = pkg.ProbeVisConfig((1 if cheb else 0) | (2 if facing and nrm is not None else 0), bias)
    usp = None if usable is None else usable.ctypes.data_as(C.POINTER(C.c_uint8))
    ofp = None if offsets is None else fp(offsets)
    rgb = np.full((len(points), 3), np.nan, F); ok = np.zeros(len(points), np.uint8)
    one = C.c_uint32(99)
    for q in range(len(points)):
        assert pkg.lib().mi355rt_probes_lookup_placed_one(C.byref(grid), up(n), fp(sh), usp, C.byref(d), C.byref(vc), ofp, fp(points[q]), fp(dirs[q]),
                                                          None if nrm is None else fp(nrm[q]), pkg.SH_MODES[mode], fp(rgb[q]), C.byref(one)) == 0
        ok[q] = one.value
    return rgb, ok


# ---- symbols, structs, defaults, refusals ---------------------------------------------------------------------------------------------------------------------
def test_place_symbols_structs_defaults_and_refusals(pkg, pr, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "mi355rt.h")).read()
    assert "PROBE PLACEMENT" in header
    for name in NEW:
        assert " T %s\n" % name in out, name
        assert name in [n for n, _, _ in pkg.ABI]
        assert hasattr(pkg.lib(), name)
        assert re.search(r"\b%s\(" % name, header), name
    consts = dict(MI355RT_SURVEY_FLIP=pkg.SURVEY_FLIP, MI355RT_PROBE_UNKNOWN=pkg.PROBE_UNKNOWN, MI355RT_PROBE_BURIED=pkg.PROBE_BURIED, MI355RT_PROBE_IDLE=pkg.PROBE_IDLE,
                  MI355RT_PROBE_ACTIVE=pkg.PROBE_ACTIVE, MI355RT_PLACE_UNSAMPLED=pkg.PLACE_UNSAMPLED, MI355RT_PLACE_THROUGH=pkg.PLACE_THROUGH, MI355RT_PLACE_AWAY=pkg.PLACE_AWAY,
                  MI355RT_PLACE_STAY=pkg.PLACE_STAY, MI355RT_PLACE_BACK=pkg.PLACE_BACK, MI355RT_PLACE_REST=pkg.PLACE_REST, MI355RT_PLACE_REFUSED=pkg.PLACE_REFUSED)
    for name, value in consts.items():
        m = re.search(r"#define\s+%s\s+(\d+)u" % name, header)
        assert m and int(m.group(1)) == value, name
    assert (pr.UNKNOWN, pr.BURIED, pr.IDLE, pr.ACTIVE) == (0, 1, 2, 3) == (pkg.PROBE_UNKNOWN, pkg.PROBE_BURIED, pkg.PROBE_IDLE, pkg.PROBE_ACTIVE)
    assert (pr.PLACE_UNSAMPLED, pr.PLACE_THROUGH, pr.PLACE_AWAY, pr.PLACE_STAY, pr.PLACE_BACK, pr.PLACE_REST, pr.PLACE_REFUSED) == (0, 1, 2, 3, 4, 5, 8)
    assert (pr.BACK_SHARE, pr.MAX_OFFSET, pr.SURVEY_FLIP) == (0.25, 0.45, 1)
    assert C.sizeof(pkg.ProbeSurveyConfig) == 20 and C.sizeof(pkg.ProbeSurvey) == 48 and C.sizeof(pkg.ProbePlaceConfig) == 16
    assert [(n, getattr(pkg.ProbeSurveyConfig, n).offset) for n, _ in pkg.ProbeSurveyConfig._fields_] == [("spp", 0), ("first_sample", 4), ("accumulate", 8), ("flags", 12),
                                                                                                          ("max_distance", 16)]
    assert [(n, getattr(pkg.ProbeSurvey, n).offset) for n, _ in pkg.ProbeSurvey._fields_] == [("n", 0), ("back", 8), ("front", 16), ("near_back", 24), ("near_front", 32), ("far", 40)]
    assert [(n, getattr(pkg.ProbePlaceConfig, n).offset) for n, _ in pkg.ProbePlaceConfig._fields_] == [("back_share", 0), ("max_offset", 4), ("min_front", 8), ("max_distance", 12)]
    assert (C.sizeof(pkg.ProbeConfig), C.sizeof(pkg.ProbeOutputs), C.sizeof(pkg.ProbeGrid), C.sizeof(pkg.ProbeDepth), C.sizeof(pkg.ProbeVisConfig)) == (16, 32, 36, 24, 8)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355rt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %u %u %u\\n",'
                   'sizeof(mi355rt_probe_survey_config),sizeof(mi355rt_probe_survey),sizeof(mi355rt_probe_place_config),offsetof(mi355rt_probe_survey_config,flags),'
                   'offsetof(mi355rt_probe_survey_config,max_distance),offsetof(mi355rt_probe_survey,near_back),offsetof(mi355rt_probe_survey,far),'
                   'offsetof(mi355rt_probe_place_config,min_front),MI355RT_SURVEY_FLIP,MI355RT_PROBE_ACTIVE,MI355RT_PLACE_REFUSED);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [20, 48, 16, 12, 16, 24, 40, 8, 1, 3, 8]
    lib = pkg.lib()
    sc = pkg.ProbeSurveyConfig(1, 2, 3, 4, 5.0)
    lib.mi355rt_probes_survey_default_config(C.byref(sc))
    assert (sc.spp, sc.first_sample, sc.accumulate, sc.flags, sc.max_distance) == (64, 0, 0, 0, 0.0)
    cfg = pkg.ProbePlaceConfig(9.0, 9.0, 9.0, 9.0)
    lib.mi355rt_probes_place_default_config(C.byref(cfg))
    assert (cfg.back_share, cfg.max_offset, cfg.min_front, cfg.max_distance) == (0.25, F(0.45), 0.0, 0.0)            # min_front has no default: 0 is refused
    lib.mi355rt_probes_survey_default_config(None); lib.mi355rt_probes_place_default_config(None)                   # tolerated
    # NULL handles
    assert lib.mi355rt_probes_survey(None, None, None, 0, C.byref(sc), 0, None) == -1
    assert lib.mi355rt_probes_place(None, None, None, None, None, 0, None, None, None) == -1
    assert lib.mi355rt_probes_lookup_placed(None, None, None, None, None, None, None, None, None, None, None, 0, 0, 0, None, None) == -1
    err = lambda: lib.mi355rt_last_error(None).decode()
    # mi355rt_probe_place_one
    g = pkg.ProbeGrid.from_dict(pp.GRID)
    counts = np.array([8, 8, 0], np.uint32); recs = np.array([0.05, 1, 0, 0] + pp.EMPTY_NEAR + pp.EMPTY_FAR, F); off = np.zeros(3, F)
    new = np.full(3, 7.0, F); v, s = C.c_uint32(99), C.c_uint32(99)
    good = pkg.ProbePlaceConfig(0.25, 0.45, 0.2, 3.0)

    def one(grid=g, cfg_=good, counts_=counts, recs_=recs, off_=off, new_=new, v_=v, s_=s):
        a = lambda x, conv: None if x is None else conv(x)
        return lib.mi355rt_probe_place_one(a(grid, C.byref), a(cfg_, C.byref), a(counts_, up), a(recs_, fp), a(off_, fp), a(new_, fp), a(v_, C.byref), a(s_, C.byref))

    assert one() == 0 and v.value == pkg.PLACE_THROUGH and s.value == pkg.PROBE_BURIED and np.array_equal(new, np.array([F(F(0.05) + F(0.5) * F(0.2)), 0, 0], F))
    new[:] = 7.0; v.value = s.value = 99
    bad_cfgs = [(pkg.ProbePlaceConfig(-0.1, 0.45, 0.2, 3.0), "back_share"), (pkg.ProbePlaceConfig(1.5, 0.45, 0.2, 3.0), "back_share"),
                (pkg.ProbePlaceConfig(float("nan"), 0.45, 0.2, 3.0), "back_share"), (pkg.ProbePlaceConfig(0.25, -1.0, 0.2, 3.0), "max_offset"),
                (pkg.ProbePlaceConfig(0.25, float("inf"), 0.2, 3.0), "max_offset"), (pkg.ProbePlaceConfig(0.25, 0.45, 0.0, 3.0), "min_front"),
                (pkg.ProbePlaceConfig(0.25, 0.45, float("nan"), 3.0), "min_front"), (pkg.ProbePlaceConfig(0.25, 0.45, float("inf"), 3.0), "min_front"),
                (pkg.ProbePlaceConfig(0.25, 0.45, 0.2, 0.0), "max_distance"), (pkg.ProbePlaceConfig(0.25, 0.45, 0.2, float("nan")), "max_distance"),
                (pkg.ProbePlaceConfig(0.25, 0.45, 0.2, 2e12), "max_distance")]
    for c, word in bad_cfgs:
        assert one(cfg_=c) == -1 and word in err() and "mi355rt_probe_place_one" in err(), word
    bad = pkg.ProbeGrid.from_dict(pp.GRID); bad.spacing[1] = 0.0
    for kw, word in ((dict(grid=None), "grid"), (dict(grid=bad), "spacing"), (dict(cfg_=None), "cfg"), (dict(counts_=None), "counts3"), (dict(recs_=None), "records12"),
                     (dict(new_=None, v_=None, s_=None), "all NULL"), (dict(off_=np.array([0, np.nan, 0], F)), "offset"), (dict(off_=np.array([np.inf, 0, 0], F)), "offset")):
        assert one(**kw) == -1 and word in err(), (kw, err())
    assert np.array_equal(new, np.full(3, 7.0, F)) and v.value == 99 and s.value == 99                               # a refusal writes nothing
    # what each output needs of the config: the state alone asks for no min_front, the move alone for no max_distance; a NULL offset is zero
    assert one(cfg_=pkg.ProbePlaceConfig(0.25, 0.45, 0.0, 3.0), new_=None, v_=None) == 0 and s.value == pkg.PROBE_BURIED
    assert one(cfg_=pkg.ProbePlaceConfig(0.25, 0.45, 0.2, 0.0), s_=None, off_=None) == 0 and v.value == pkg.PLACE_THROUGH and new[0] == F(F(0.05) + F(0.5) * F(0.2))
    # mi355rt_probes_lookup_placed_one: the refusals of mi355rt_probes_lookup_vis_one, and the offsets
    g1 = pkg.ProbeGrid.from_dict(pc.grid((1, 1, 1)))
    n = np.ones(1, np.uint32); sh = np.zeros(27, F); v3 = np.array([0.0, 0.0, 1.0], F); rgb = np.full(3, 7.0, F)
    f = pv.film(3, 1, 1)
    depth = pkg.ProbeDepth(3, 3.0, f["count"].ctypes.data, f["moments"].ctypes.data)
    vc = pkg.ProbeVisConfig(3, 0.0)

    def look(grid=g1, n_=n, sh_=sh, depth_=depth, vc_=vc, off_=None, point=v3, dir_=v3, normal=v3, mode=0, rgb_=rgb):
        a = lambda x, conv: None if x is None else conv(x)
        return lib.mi355rt_probes_lookup_placed_one(a(grid, C.byref), a(n_, up), a(sh_, fp), None, a(depth_, C.byref), a(vc_, C.byref), a(off_, fp), a(point, fp), a(dir_, fp),
                                                    a(normal, fp), mode, a(rgb_, fp), None)

    assert look() == 0 and look(off_=np.zeros(3, F)) == 0 and not np.array_equal(rgb, np.full(3, 7.0, F))
    rgb[:] = 7.0
    for kw, word in ((dict(grid=None), "grid"), (dict(n_=None), "n is NULL"), (dict(sh_=None), "sh"), (dict(depth_=None), "depth"), (dict(vc_=None), "vc"),
                     (dict(point=None), "point"), (dict(dir_=None), "dir"), (dict(rgb_=None), "rgb"), (dict(mode=2), "mode"), (dict(normal=None), "normals3"),
                     (dict(vc_=pkg.ProbeVisConfig(4, 0.0)), "flags"), (dict(vc_=pkg.ProbeVisConfig(3, float("nan"))), "normal_bias"),
                     (dict(depth_=pkg.ProbeDepth(1, 3.0, f["count"].ctypes.data, f["moments"].ctypes.data)), "res"),
                     (dict(off_=np.array([0, 0, np.nan], F)), "offsets"), (dict(off_=np.array([-np.inf, 0, 0], F)), "offsets")):
        assert look(**kw) == -1 and word in err(), (kw, err())
        assert "mi355rt_probes_lookup_placed_one" in err()
    assert np.array_equal(rgb, np.full(3, 7.0, F))
    # the statement refuses what the library refuses
    sv = pr.survey_empty(48, 3.0)
    for kw in (dict(min_front=None), dict(min_front=0.0), dict(min_front=np.inf), dict(min_front=0.2, back_share=1.5), dict(min_front=0.2, max_offset=-1.0)):
        with pytest.raises(ValueError):
            pr.place(sv, None, pp.GRID, **kw)
    with pytest.raises(ValueError, match="offsets"):
        pr.place(sv, np.full((48, 3), np.nan, F), pp.GRID, min_front=0.2)
    for D in (0.0, -1.0, np.nan, np.inf, 2e12):
        with pytest.raises(ValueError, match="max_distance"):
            pr.survey(np.zeros(2, F), np.zeros(2, np.uint32), np.zeros((2, 3), F), np.zeros((1, 3), F), 2, D)
    assert pr.grid_min_front(pp.GRID) == float(F(0.2) * F(0.5)) and pr.grid_min_front(pp.FLAT) == float(F(0.2))
    assert pr.grid_min_front(pc.grid((1, 1, 1))) == float(F(0.2))
    assert np.array_equal(pr.usable_states(np.array([0, 1, 2, 3], np.uint8)), np.array([0, 0, 1, 1], np.uint8))


# ---- the survey ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_survey_by_hand(pr):
    t, prim, d, N, D = pp.hand_samples()
    sv = pr.survey(t, prim, d, N, 2, D)
    assert all(sv[k].dtype == np.uint32 and sv[k].shape == (2,) for k in ("n", "back", "front"))
    assert all(sv[k].dtype == F and sv[k].shape == (2, 4) for k in ("near_back", "near_front", "far")) and sv["max_distance"] == 2.0
    rec = lambda dist, v: bits(np.array([dist] + list(v), F))
    # point 0: front 1.5 (0, .6, -.8); back 0.7 (.6, 0, .8); front 1.5 again: the first keeps the record; NaN, 0, negative and infinite t are misses: far is D
    # by the first of them; the last back hit at 0.7 again: the first keeps near_back
    assert (sv["n"][0], sv["back"][0], sv["front"][0]) == (8, 2, 2)
    assert np.array_equal(bits(sv["near_front"][0]), rec(1.5, [0.0, 0.6, -0.8])) and np.array_equal(bits(sv["near_back"][0]), rec(0.7, [0.6, 0.0, 0.8]))
    assert np.array_equal(bits(sv["far"][0]), rec(2.0, [0.0, 0.6, -0.8]))                                            # the NaN t (sample 3): the first miss
    # point 1: the NaN normal is a front hit (0.9); a hit exactly at D and one beyond it both record D in far, the first keeps it; the miss after them does not
    # replace it; the nearer front hit 0.4 (-x normal, ray +x: dot -1) replaces near_front, the same t again does not; one back hit (0.25 along +z normal)
    assert (sv["n"][1], sv["back"][1], sv["front"][1]) == (8, 1, 5)
    assert np.array_equal(bits(sv["near_front"][1]), rec(0.4, [1.0, 0.0, 0.0])) and np.array_equal(bits(sv["near_back"][1]), rec(0.25, [0.6, 0.0, 0.8]))
    assert np.array_equal(bits(sv["far"][1]), rec(2.0, [0.0, 0.6, -0.8]))
    # flip negates the normals: front and back trade places, the NaN normal stays front
    fl = pr.survey(t, prim, d, N, 2, D, flip=True)
    assert (fl["back"][0], fl["front"][0]) == (2, 2) and np.array_equal(bits(fl["near_back"][0]), rec(1.5, [0.0, 0.6, -0.8]))
    assert np.array_equal(bits(fl["near_front"][0]), rec(0.7, [0.6, 0.0, 0.8])) and np.array_equal(bits(fl["far"][0]), rec(2.0, [0.0, 0.6, -0.8]))     # 0.7, then the first miss
    assert np.array_equal(bits(pr.survey(t[:6], prim[:6], d[:6], N, 2, D, flip=True)["far"][0]), rec(0.7, [0.6, 0.0, 0.8]))                         # before that miss
    assert (fl["back"][1], fl["front"][1]) == (4, 2) and np.array_equal(bits(fl["near_front"][1]), rec(0.25, [0.6, 0.0, 0.8]))
    assert np.array_equal(bits(fl["near_back"][1]), rec(0.4, [1.0, 0.0, 0.0]))
    # an empty survey
    e = pr.survey(t[:0], prim[:0], d[:0], N, 2, D)
    assert not e["n"].any() and np.array_equal(e["near_back"], np.array([pp.EMPTY_NEAR] * 2, F)) and np.array_equal(e["far"], np.array([pp.EMPTY_FAR] * 2, F))
    # prev= split at every sample boundary equals the unsplit state on every bit, and prev is not written
    for flip in (False, True):
        whole = pr.survey(t, prim, d, N, 2, D, flip)
        for k in range(9):
            a = pr.survey(t[:2 * k], prim[:2 * k], d[:2 * k], N, 2, D, flip)
            keep = {key: np.array(v).copy() for key, v in a.items()}
            b = pr.survey(t[2 * k:], prim[2 * k:], d[2 * k:], N, 2, D, flip, prev=a)
            assert all(np.array_equal(bits(keep[key]) if keep[key].dtype == F else keep[key], bits(a[key]) if keep[key].dtype == F else a[key]) for key in pp_keys())
            for key in pp_keys():
                assert np.array_equal(b[key].view(np.uint32), whole[key].view(np.uint32)), (flip, k, key)
    with pytest.raises(ValueError, match="max_distance"):
        pr.survey(t, prim, d, N, 2, 3.0, prev=sv)


def pp_keys():
    return ("n", "back", "front", "near_back", "near_front", "far")


# ---- placement and states ---------------------------------------------------------------------------------------------------------------------------------------
def test_place_one_equals_the_statement_on_every_branch(pkg, pr):
    names, sv, off = pp.place_cases()
    want, verdict = pr.place(sv, off, pp.GRID, min_front=pp.MIN_FRONT, want_verdict=True)
    state = pr.classify(sv)
    got, gv, gs = c_place(pkg, pp.GRID, sv, off)
    assert want.dtype == F and verdict.dtype == np.uint8 and state.dtype == np.uint8
    assert np.array_equal(gv, verdict) and np.array_equal(gs, state) and np.array_equal(bits(got), bits(want))
    by = dict(zip(names, zip(verdict.tolist(), state.tolist(), want.tolist(), off.tolist())))
    R = pr.PLACE_REFUSED
    expect = {"unsampled": (pr.PLACE_UNSAMPLED, pr.UNKNOWN), "through": (pr.PLACE_THROUGH, pr.BURIED), "through refused": (pr.PLACE_THROUGH | R, pr.BURIED),
              "through at the share": (pr.PLACE_REST, pr.ACTIVE), "through on the bound": (pr.PLACE_THROUGH | R, pr.BURIED), "away": (pr.PLACE_AWAY, pr.ACTIVE),
              "away short far": (pr.PLACE_AWAY, pr.ACTIVE), "away refused": (pr.PLACE_AWAY | R, pr.ACTIVE), "stay": (pr.PLACE_STAY, pr.ACTIVE),
              "at 60 degrees": (pr.PLACE_AWAY, pr.ACTIVE), "inside 60 degrees": (pr.PLACE_STAY, pr.ACTIVE), "away zero far": (pr.PLACE_AWAY | R, pr.ACTIVE), "back part": (pr.PLACE_BACK, pr.ACTIVE),
              "back whole": (pr.PLACE_BACK, pr.ACTIVE), "back empty": (pr.PLACE_BACK, pr.IDLE), "back at min_front": (pr.PLACE_BACK, pr.ACTIVE), "rest": (pr.PLACE_REST, pr.ACTIVE),
              "rest idle": (pr.PLACE_REST, pr.IDLE), "rest front at D": (pr.PLACE_REST, pr.IDLE), "through overflow": (pr.PLACE_THROUGH | R, pr.BURIED),
              "through denormal": (pr.PLACE_THROUGH, pr.BURIED), "away denormal": (pr.PLACE_AWAY | R, pr.ACTIVE), "nan share record": (pr.PLACE_AWAY, pr.BURIED),
              "buried no way": (pr.PLACE_THROUGH, pr.BURIED), "back negative zero": (pr.PLACE_REST, pr.IDLE)}
    assert set(expect) == set(names)
    lf = np.sqrt(F(F(0.5) * F(0.5)) + F(F(0.8660254) * F(0.8660254)))
    assert F(0.5) <= F(F(0.5) * F(1.0)) * lf                                                                        # "at 60 degrees": <= holds in f32, so it steps away
    for name, (v, s) in expect.items():
        assert by[name][:2] == (v, s), (name, by[name])
    # every branch occurs, accepted, and the three that make a candidate also refused
    assert {pr.PLACE_UNSAMPLED, pr.PLACE_THROUGH, pr.PLACE_AWAY, pr.PLACE_STAY, pr.PLACE_BACK, pr.PLACE_REST, pr.PLACE_THROUGH | R, pr.PLACE_AWAY | R} <= set(verdict.tolist())
    for name in names:
        moved, refused = by[name][2] != by[name][3], bool(by[name][0] & R)
        assert not (moved and refused), name                                                                       # a refused candidate leaves the offset as it was
        if by[name][0] in (pr.PLACE_UNSAMPLED, pr.PLACE_STAY, pr.PLACE_REST):
            assert not moved, name
    assert by["back whole"][2] == [0.0, 0.0, 0.0] and by["back empty"][2] == [0.0, 0.0, 0.0]                       # the whole way is exactly the grid point
    assert by["back at min_front"][2] == by["back at min_front"][3]
    assert by["buried no way"][2][2] == F(F(0.6) + F(0.5) * F(0.2))
    # a candidate exactly ON the bound is refused, one ulp inside it accepted
    assert F(F(0.35) + F(0.5) * F(0.2)) == F(F(0.45) * F(1.0))
    inside = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sv.items()}
    i = names.index("through on the bound")
    inside["near_back"][i, 0] = np.nextafter(F(0.35), F(0))
    w2, v2 = pr.place(inside, off, pp.GRID, min_front=pp.MIN_FRONT, want_verdict=True)
    g2, gv2, _ = c_place(pkg, pp.GRID, inside, off)
    assert v2[i] == pr.PLACE_THROUGH and w2[i, 0] < F(0.45) and np.array_equal(bits(g2), bits(w2)) and np.array_equal(gv2, v2)
    # a BACK candidate can be refused too: an offset outside the bound (as a caller with a smaller max_offset than last time has it) cannot come part of the way
    o3 = off.copy(); o3[names.index("back part")] = [0.9, 0.0, 0.0]
    w3, v3 = pr.place(sv, o3, pp.GRID, min_front=pp.MIN_FRONT, want_verdict=True)
    g3, gv3, _ = c_place(pkg, pp.GRID, sv, o3)
    assert v3[names.index("back part")] == pr.PLACE_BACK | R and np.array_equal(bits(g3), bits(w3)) and np.array_equal(gv3, v3)
    # a single-probe axis accepts only 0 on it: the same surveys in a grid whose y axis has one probe
    names6, sv6, off6 = pp.place_cases(6)
    off6 = off6.copy(); off6[:, 1] = 0
    w6, v6 = pr.place(sv6, off6, pp.FLAT, min_front=pp.MIN_FRONT, want_verdict=True)
    g6, gv6, gs6 = c_place(pkg, pp.FLAT, sv6, off6)
    assert np.array_equal(bits(g6), bits(w6)) and np.array_equal(gv6, v6) and np.array_equal(gs6, pr.classify(sv6))
    assert v6[names6.index("through")] == pr.PLACE_THROUGH | R                                                     # its step has a y component
    assert v6[names6.index("through on the bound")] == pr.PLACE_THROUGH | R and v6[names6.index("away")] == pr.PLACE_AWAY | R
    assert not w6[:, 1].any()
    only_x = {k: (v[:6].copy() if isinstance(v, np.ndarray) else v) for k, v in sv6.items()}
    only_x["near_back"][1] = [0.05, 1.0, 0.0, 0.0]
    w7, v7 = pr.place(only_x, off6, pp.FLAT, min_front=pp.MIN_FRONT, want_verdict=True)
    assert v7[1] == pr.PLACE_THROUGH and w7[1, 0] > 0 and np.array_equal(bits(c_place(pkg, pp.FLAT, only_x, off6)[0]), bits(w7))      # along x alone: accepted
    # NULL offsets are zero offsets
    zero = np.zeros_like(off)
    wz, vz = pr.place(sv, None, pp.GRID, min_front=pp.MIN_FRONT, want_verdict=True)
    gz, gvz, _ = c_place(pkg, pp.GRID, sv, None)
    assert np.array_equal(bits(wz), bits(pr.place(sv, zero, pp.GRID, min_front=pp.MIN_FRONT))) and np.array_equal(bits(gz), bits(wz)) and np.array_equal(gvz, vz)
    # other configs, and fixed-seed surveys around every decision
    seen = set()
    for seed, grid in ((1, pp.GRID), (2, pp.GRID), (3, pp.FLAT)):
        nprobes = int(np.prod(grid["counts"]))
        svr, offr = pp.random_surveys(nprobes * 40, seed, grid)
        for k in range(40):
            part = {key: (v[k * nprobes:(k + 1) * nprobes] if isinstance(v, np.ndarray) else v) for key, v in svr.items()}
            o = np.ascontiguousarray(offr[k * nprobes:(k + 1) * nprobes])
            bs, mo, mf = (0.25, 0.45, 0.2) if k % 2 else (0.1, 0.3, 0.35)
            w, v = pr.place(part, o, grid, bs, mo, mf, want_verdict=True)
            g, gv, gs = c_place(pkg, grid, part, o, bs, mo, mf)
            assert np.array_equal(bits(g), bits(w)) and np.array_equal(gv, v) and np.array_equal(gs, pr.classify(part, bs)), (seed, k)
            seen |= set(v.tolist()) | {10 + s for s in gs.tolist()}
    assert seen >= {0, 1, 2, 3, 4, 5, 9, 10, 12, 10, 11, 12, 13}


def test_place_by_hand(pkg, pr):
    """One probe against a surface, in Python floats rounded per step: the AWAY branch, every number written out."""
    nf = [F(0.03), F(0.6), F(0.0), F(-0.8)]
    fr = [F(1.7), F(-0.28), F(0.0), F(0.96)]
    o = [F(0.05), F(-0.02), F(0.1)]
    mf = F(0.2)
    sv = dict(n=np.full(8, 64, np.uint32), back=np.full(8, 3, np.uint32), front=np.full(8, 40, np.uint32), near_back=np.tile(np.array([[0.5, 0, 1, 0]], F), (8, 1)),
              near_front=np.tile(np.array([nf], F), (8, 1)), far=np.tile(np.array([fr], F), (8, 1)), max_distance=3.0)
    o8 = np.tile(np.array([o], F), (8, 1))
    g = dict(origin=np.zeros(3, F), spacing=np.array([1.0, 1.0, 1.0], F), counts=np.array([2, 2, 2], np.uint32))
    share = F(F(3) / F(64))
    assert not share > F(0.25) and nf[0] < mf
    dot = F(F(F(nf[1] * fr[1]) + F(nf[2] * fr[2])) + F(nf[3] * fr[3]))
    ln = np.sqrt(F(F(F(nf[1] * nf[1]) + F(nf[2] * nf[2])) + F(nf[3] * nf[3])))
    lf = np.sqrt(F(F(F(fr[1] * fr[1]) + F(fr[2] * fr[2])) + F(fr[3] * fr[3])))
    assert dot <= F(F(F(0.5) * ln) * lf)
    m = fr[0] if fr[0] < mf else mf
    hand = np.array([F(o[a] + F(F(fr[1 + a] * m) / lf)) for a in range(3)], F)
    assert all(abs(h) < F(F(0.45) * F(1.0)) for h in hand)
    want, v = pr.place(sv, o8, g, min_front=float(mf), want_verdict=True)
    assert v[0] == pr.PLACE_AWAY and np.array_equal(bits(want[0]), bits(hand))
    got, gv, gs = c_place(pkg, g, sv, o8, min_front=float(mf))
    assert gv[0] == pr.PLACE_AWAY and gs[0] == pr.ACTIVE and np.array_equal(bits(got[0]), bits(hand))
    # ... and the part of the way BACK, by hand
    sv["near_front"][:] = [0.3, 1, 0, 0]
    lo = np.sqrt(F(F(F(o[0] * o[0]) + F(o[1] * o[1])) + F(o[2] * o[2])))
    room = F(F(0.3) - mf)
    assert room < lo
    hand = np.array([F(o[a] + F(F(F(-o[a]) * room) / lo)) for a in range(3)], F)
    want, v = pr.place(sv, o8, g, min_front=float(mf), want_verdict=True)
    assert v[0] == pr.PLACE_BACK and np.array_equal(bits(want[0]), bits(hand)) and np.array_equal(bits(c_place(pkg, g, sv, o8, min_front=float(mf))[0][0]), bits(hand))
    assert np.linalg.norm(hand) < np.linalg.norm(o)


# ---- the lookup that knows the offsets -------------------------------------------------------------------------------------------------------------------------------
def offsets_for(g, pts, seed):
    """(name, offsets) for a grid: zero, fixed-seed within +-0.45 spacing, and one that puts a probe exactly on the first query"""
    cnt = [int(c) for c in g["counts"]]
    nprobes = cnt[0] * cnt[1] * cnt[2]
    rng = np.random.default_rng(seed)
    rnd = (rng.uniform(-0.45, 0.45, (nprobes, 3)) * g["spacing"].astype(np.float64)).astype(F)
    on = rnd.copy()
    gp = pc.probe_positions(g)
    j = int(np.argmin(np.where(np.isfinite(pts[0]).all(), np.abs(gp - pts[0]).sum(axis=1), 0)))
    on[j] = pts[0] - gp[j]                                          # exact where the subtraction is (Sterbenz); the r == 0 case is asserted by the caller
    return [("zero", np.zeros((nprobes, 3), F)), ("random", np.ascontiguousarray(rnd)), ("on the query", np.ascontiguousarray(on))]


@pytest.mark.parametrize("mode", ["radiance", "irradiance"])
def test_lookup_placed_one_equals_the_statement_and_collapses(pkg, pr, mode):
    used = unused = differs = on_query = 0
    for k, (name, g, res, depth, usable, pts, dirs, nrm) in enumerate(pv.lookup_cases()):
        step = 1 if len(pts) < 200 else 4                              # the queries' kinds repeat with period 8: the residues k % 4 and k % 4 + 4 alternate over the cases
        p, d, nr = (np.ascontiguousarray(a[k % step::step]) for a in (pts, dirs, nrm))
        plain, pok = pr.lookup(g, res, p, d, mode, usable)
        for cheb, facing in pv.FLAGS:
            normals, bias = ((nr, 0.13), (None, 0.0), (nr, 0.0))[(k + cheb + 2 * facing) % 3]
            vis, vok = pr.lookup_vis(g, res, depth, p, d, normals, mode, usable, cheb, facing, bias)
            # NULL offsets: lookup_vis on every bit, for the statement and for the library
            want, wok = pr.lookup_placed(g, res, depth, p, d, normals, mode, usable, cheb, facing, bias, None)
            got, gok = c_lookup_placed(pkg, g, res, depth, usable, None, p, d, normals, mode, cheb, facing, bias)
            assert np.array_equal(bits(want), bits(vis)) and np.array_equal(wok, vok), (name, cheb, facing)
            assert np.array_equal(bits(got), bits(vis)) and np.array_equal(gok, vok), (name, cheb, facing)
            for oname, off in offsets_for(g, p, 70 + k):
                want, wok = pr.lookup_placed(g, res, depth, p, d, normals, mode, usable, cheb, facing, bias, off)
                got, gok = c_lookup_placed(pkg, g, res, depth, usable, off, p, d, normals, mode, cheb, facing, bias)
                assert np.array_equal(gok, wok), (name, oname, cheb, facing)
                assert np.array_equal(bits(got), bits(want)), (name, oname, cheb, facing)
                assert not want[wok == 0].view(np.uint32).any()
                if not cheb and (not facing or normals is None):
                    # with both flags off the offsets cannot matter: lookup on every bit
                    assert np.array_equal(bits(want), bits(plain)) and np.array_equal(wok, pok), (name, oname)
                elif oname == "random":
                    differs += int((bits(want) != bits(vis)).any())
                used += int(wok.sum()); unused += int((wok == 0).sum())
        # a probe exactly on the query (r == 0): visibility 1 and facing skipped, so its weight is its trilinear weight
        off = offsets_for(g, p, 70 + k)[2][1]
        if np.isfinite(p[0]).all() and usable is None:
            w, probe = pr.corner_weights(g, res, depth, p[:1], nr[:1], None, True, True, 0.0, off)
            w0, _ = pr.corner_weights(g, res, depth, p[:1], None, None, False, False, 0.0, None)
            gp = pc.probe_positions(g)
            hit = [(j, c) for c, j in enumerate(probe[0]) if np.array_equal((gp[j] + off[j]).astype(F), p[0])]
            for j, c in hit:
                assert bits(w[0, c]) == bits(w0[0, c])
                on_query += 1
    assert used > 5000 and unused > 1000 and differs > 10 and on_query >= 8
    with pytest.raises(ValueError, match="offsets"):
        pr.lookup_placed(g, res, depth, p, d, None, mode, offsets=np.full((len(res["n"]), 3), np.inf, F))
    with pytest.raises(ValueError, match="mode"):
        pr.lookup_placed(g, res, depth, p, d, None, "sine")


# ---- the outcomes on hand-made scenes, traced by the CPU oracle -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tracer(pkg, oracle, pr):
    ga = importlib.import_module("raytracer_rs_amd.gather")
    ft = importlib.import_module("raytracer_rs_amd.features")
    made = []

    def get(scene):
        made.append(pp.OracleTracer(oracle, ga, pr, ft, scene))
        return made[-1]
    yield get
    for t in made:
        t.close()


def test_a_buried_probe_within_reach_leaves_its_box(pr, tracer):
    rt = tracer(pp.scene_a())
    gp = pr.grid_points(pp.GRID3)
    D = pr.grid_max_distance(pp.GRID3)
    before = rt.probes_survey(gp, None, spp=64, max_distance=D)
    c = pp.CENTRE
    assert np.array_equal(gp[c], np.array([1, 1, 1], F)) and before["back"][c] == before["n"][c] == 64 and pr.classify(before)[c] == pr.BURIED
    assert (pr.classify(before)[np.arange(27) != c] != pr.BURIED).all()
    res = pr.relocate(rt, pp.GRID3, rounds=4, spp=64, min_front=0.2)
    fresh = rt.probes_survey(res["points"], None, spp=64, first_sample=1000, max_distance=D)
    assert fresh["back"][c] == 0 and res["survey"]["back"][c] == 0
    assert (np.abs(res["offsets"]) < F(0.45)).all() and np.abs(res["offsets"][c]).max() > 0.1                      # outside a box of half-size 0.1
    assert res["state"][c] != pr.BURIED and res["usable"][c] == 1 and (res["state"] != pr.BURIED).all()
    assert np.array_equal(res["points"], (gp + res["offsets"]).astype(F))
    # end to end: a query beside the box, in a cell that has the centre probe as a corner.  The depth films at the moved points, the offset-aware weights and
    # usable_states let all eight corners contribute; the unmoved grid has to drop the buried probe and keeps seven
    q = np.array([[1.4, 1.3, 1.35]], F)
    films = lambda pts, first: dict(res=8, max_distance=D, **film_of(rt, pr, pts, first, D))
    moved, unmoved = films(res["points"], 2000), films(gp, 2000)
    n = dict(n=np.full(27, 64, np.uint32))
    w, probe = pr.corner_weights(pp.GRID3, n, moved, q, None, res["usable"], True, False, 0.0, res["offsets"])
    assert c in probe[0] and (w[0] > 0).sum() == 8
    w0, _ = pr.corner_weights(pp.GRID3, n, unmoved, q, None, pr.usable_states(pr.classify(before)), True, False, 0.0, None)
    assert (w0[0] > 0).sum() == 7 and w0[0][list(probe[0]).index(c)] == 0


def film_of(rt, pr, pts, first, D, spp=64, R=8):
    """the depth film of the points from the oracle's hits: dict(count, moments)"""
    rays, _, _, _ = rt.ga.rays(rt.table, pp.SEED, pts, None, None, first, spp)
    tuv, prim = rt.orc.intersect(rays, brute=True)
    return pr.project_depth(tuv[:, 0], prim != pp.MISS, rays[:, 3:], len(pts), R, D)


def test_a_buried_probe_out_of_reach_stays_and_is_marked(pr, tracer):
    rt = tracer(pp.scene_b())
    c = pp.CENTRE
    for rounds in (1, 4):
        res = pr.relocate(rt, pp.GRID3, rounds=rounds, spp=64, min_front=0.2)
        assert res["verdict"][c] == pr.PLACE_THROUGH | pr.PLACE_REFUSED                                           # every candidate is refused: 0.6 + 0.1 >= 0.45
        assert not res["offsets"][c].any() and res["state"][c] == pr.BURIED and res["usable"][c] == 0
        assert res["survey"]["back"][c] == 64 and res["usable"].sum() == 26


def test_a_probe_against_a_wall_steps_away_and_returns_when_the_wall_is_gone(pr, tracer):
    rt = tracer(pp.scene_c())
    gp = pr.grid_points(pp.GRID_WALL)
    D = pr.grid_max_distance(pp.GRID_WALL)
    near = np.nonzero(gp[:, 2] == F(0.02))[0]
    assert len(near) == 4
    before = rt.probes_survey(gp, None, spp=64, max_distance=D)
    assert (before["back"] == 0).all() and (before["near_front"][near, 0] < F(0.2)).all() and (before["near_front"][near, 0] >= F(0.02)).all()
    res = pr.relocate(rt, pp.GRID_WALL, rounds=4, spp=64, min_front=0.2)
    assert (res["points"][near, 2] > gp[near, 2] + F(0.05)).all()                                                 # farther from the wall than they began
    assert (res["state"] == pr.ACTIVE).all() and (np.abs(res["offsets"]) < F(0.45)).all()
    one = pr.relocate(rt, pp.GRID_WALL, rounds=1, spp=64, min_front=0.2)
    assert (one["verdict"][near] == pr.PLACE_AWAY).all() and (one["offsets"][near, 2] > 0).all()
    # the wall taken out: the next placement brings every probe back to its grid point, the whole way
    gone = tracer(pp.scene_d())
    sv = gone.probes_survey(res["points"], None, spp=64, first_sample=500, max_distance=D)
    off, verdict = pr.place(sv, res["offsets"], pp.GRID_WALL, min_front=0.2, want_verdict=True)
    assert (verdict[near] == pr.PLACE_BACK).all() and not off.any()


def test_a_probe_in_empty_space_rests_and_is_idle(pr, tracer):
    rt = tracer(pp.scene_d())
    res = pr.relocate(rt, pp.GRID3, rounds=2, spp=16)
    assert not res["offsets"].any() and (res["state"] == pr.IDLE).all() and (res["usable"] == 1).all() and (res["verdict"] == pr.PLACE_REST).all()
    assert (res["survey"]["n"] == 16).all() and not res["survey"]["front"].any() and rt.rays == 3 * 27 * 16          # rounds + 1 surveys, fresh sample numbers each
