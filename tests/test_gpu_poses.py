"""The pinhole's screen-space shortcuts (cull rectangles, coverage mask, tile bins, cached verdicts) where they switch on and off.

`Renderer::device_camera` derives all of them from the camera, and only while every corner of every padded top BVH box lies in front of the eye
(`front`).  Here the eye is dollied through the geometry and turned away from it, one handle is taken across the switch and back, and every frame
is held to the CPU oracle bit for bit in both shipped semantics: film sums, sums of squares, counts, packed pixels and the ray counters, the same f32
camera arguments going to the handle and to the oracle in the same order.

Every frame is classified from the library's own report (MI355RT_DEBUG_CULL, captured from fd 2): `cull rects N front F`, the rectangles, `cull mask:`
and `tile bins:`.  Each test asserts the regimes it is about, so a pose that stops reaching its regime fails the test instead of silently testing
something else.  `nodes_visited` under FLAG_COUNT_STEPS is the second witness that the bins served the primary round.

MI355RT_TEST_VERBOSE=1 prints every frame's report and figures (past the capture that reads the library's lines)."""
import os
import re

import numpy as np
import pytest

from test_gpu_denoise import assert_guides_equal, oracle_guides
from test_gpu_tiles import assert_matches_snapshots, checkerboard, pixels_of

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 7
# (scene, z of the "past everything" pose, z range in which the dolly poses have the eye inside the geometry)
DOLLY = {"4boxes": (16.0, (10.0, 13.0)), "ico2": (16.0, (10.0, 13.0)), "thai2": (40.0, (10.0, 18.0))}
ENV_SWITCHES = ("MI355RT_NO_CULL", "MI355RT_NO_CULL_MASK", "MI355RT_NO_CULL_CACHE", "MI355RT_NO_RASTER", "MI355RT_NO_SPECULATE", "MI355RT_NO_FUSED")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def say(capfd, text):
    if os.environ.get("MI355RT_TEST_VERBOSE"):
        with capfd.disabled():
            print(text, flush=True)


# ---- the library's own report -------------------------------------------------------------------------------------------------------
RE_RECTS = re.compile(r"\[mi355rt\] cull rects (\d+) front (\d)")
RE_RECT = re.compile(r"^\s+x \[(\S+), (\S+)\] y \[(\S+), (\S+)\]\s*$")
RE_MASK = re.compile(r"\[mi355rt\] cull mask: (\d+) of (\d+) cells set")
RE_BINS = re.compile(r"\[mi355rt\] tile bins: (\d+) x (\d+) tiles")
RE_NOBINS = re.compile(r"\[mi355rt\] tile bins: not built \(exit (\d+)\)")


class Report:
    """one call of device_camera as the library printed it"""

    def __init__(self):
        self.front = None          # 0 / 1
        self.nrects = 0
        self.widest = 0.0          # the widest side of any cull rectangle
        self.mask_cells = None     # cells set, when the mask was rebuilt in this call
        self.bins = None           # (blocks, groups) when the bins were rebuilt in this call
        self.bins_exit = None      # k of "not built (exit k)"

    def __repr__(self):
        return "front %s rects %d widest %.4g mask %s bins %s exit %s" % (self.front, self.nrects, self.widest, self.mask_cells, self.bins, self.bins_exit)


def parse_reports(err):
    """the device_camera calls in a piece of the library's stderr, in order (the mask and bins lines of a call come before its `cull rects` line)"""
    out, cur, last = [], Report(), None
    for line in err.splitlines():
        m = RE_MASK.search(line)
        if m:
            cur.mask_cells = int(m.group(1)); continue
        m = RE_BINS.search(line)
        if m:
            cur.bins = (int(m.group(1)), int(m.group(2))); continue
        m = RE_NOBINS.search(line)
        if m:
            cur.bins_exit = int(m.group(1)); continue
        m = RE_RECTS.search(line)
        if m:
            cur.nrects, cur.front = int(m.group(1)), int(m.group(2))
            out.append(cur); last, cur = cur, Report()
            continue
        m = RE_RECT.match(line)
        if m and last is not None:
            x0, x1, y0, y1 = (float(g) for g in m.groups())
            last.widest = max(last.widest, x1 - x0, y1 - y0)
    return out


def one_report(err):
    reps = parse_reports(err)
    assert len(reps) == 1, err              # frames this small are one pass of one slice
    r = reps[0]
    if r.front == 0:                        # the whole machinery stands down: nothing is built
        assert r.mask_cells is None and r.bins is None and r.bins_exit is None, r
    return r


# ---- a handle and an oracle that are moved together -----------------------------------------------------------------------------------
class Pair:
    def __init__(self, pkg, oracle, scenes, name, w, h, sem, capfd):
        self.pkg, self.oracle, self.capfd = pkg, oracle, capfd
        self.name, self.w, self.h, self.sem = name, w, h, sem
        self.scene = scenes(name)
        self.rt = pkg.create_raytracer_from_arrays(self.scene, pkg.DEFAULT_TRIANGLES_PER_LEAF, w, h, seed=SEED, flags=sem.gpu)
        self.orc = oracle.Oracle(self.scene, w, h, seed=SEED, flags=sem.orc)
        self.z = F(0.0)                     # the dolly coordinate: what the camera's own `pos.z += z` (f32) holds

    def move(self, x, y, z):
        self.rt.camera.move_rel(x, y, z); self.orc.camera_move_rel(x, y, z)

    def yaw(self, a):
        self.rt.camera.add_y_angle(a); self.orc.camera_add_y_angle(a)

    def pitch(self, a):
        self.rt.camera.add_x_angle(a); self.orc.camera_add_x_angle(a)

    def dolly_to(self, z):
        """relative moves along the view axis until the camera's f32 coordinate IS z (the first lands within an ulp, the second is exact)"""
        z = F(z)
        for _ in range(3):
            d = F(z - self.z)
            if d == 0:
                break
            self.move(0.0, 0.0, float(d))
            self.z = F(self.z + d)
        assert self.z == z

    def clear(self):
        self.rt.film.clear(); self.orc.film_clear()

    def same_cameras(self):
        for a, b in zip(self.rt.camera.matrices(), self.orc.camera_matrices()):
            assert np.array_equal(bits(a), bits(b))

    def same_pixels(self, where=""):
        assert np.array_equal(self.rt.get_tonemapped_pixels(), self.orc.get_tonemapped_pixels()), (self.name, self.w, self.h, self.sem, where)

    def same_film(self, where=""):
        tag = (self.name, self.w, self.h, self.sem, where)
        gs, gq, gn = self.rt.film.pixel_datas(); os_, oq, on = self.orc.film()
        assert np.array_equal(gn, on), tag
        assert np.array_equal(bits(gs), bits(os_)), tag
        assert np.array_equal(bits(gq), bits(oq)), tag
        self.same_pixels(where)

    def render(self, spp, where="", compare=True):
        """one whole frame on both sides: (the handle's counters, the library's report); counters and film equal the oracle's"""
        self.capfd.readouterr()
        c = self.rt.render(spp)
        rep = one_report(self.capfd.readouterr().err)
        oc = self.orc.render(spp, nthreads=16)
        tag = (self.name, self.w, self.h, self.sem, where, rep)
        assert (c.primary, c.bounce, c.shadow, c.primary_hits) == (oc["primary"], oc["bounce"], oc["shadow"], oc["primary_hits"]), tag
        assert c.primary == self.w * self.h * spp
        if rep.front == 0:
            assert c.primary_culled == 0, tag           # no rectangles, nothing culled
        if compare:
            self.same_film(where)
        return c, rep

    def frame(self, where=""):
        """one 50-row frame of the drop-in entry on both sides; the call's counters equal the oracle's"""
        before = self.orc.counters()
        assert self.rt.trace_frame_additive() == self.orc.trace_frame_additive() == 50 * self.w
        after = self.orc.counters()
        c = self.rt.last_counts()
        assert (c.primary, c.bounce, c.shadow, c.primary_hits) == tuple(after[k] - before[k] for k in ("primary", "bounce", "shadow", "primary_hits")), (self.name, self.sem, where)
        assert self.rt.current_row == self.orc.current_row
        return c

    def eye_inside_bounds(self):
        v = np.asarray(self.scene["tri_verts"], np.float32).reshape(-1, 3)
        o = self.orc.get_ray(0, 0, 0.5, 0.5)[:3]
        return bool(np.all(o >= v.min(0)) and np.all(o <= v.max(0)))


def scene_diag(scene):
    v = np.asarray(scene["tri_verts"], np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def clean_env(monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MI355RT_DEBUG_CULL", "1")          # read with getenv on every call


# ---- the switch, found on the library's own `front` report -----------------------------------------------------------------------------
_switches = {}


def find_switch(pkg, oracle, scenes, sem, capfd, name):
    """(dolly poses, lo, hi): `front` is 1 at z = lo and 0 at z = hi, hi - lo < 1e-5 of the scene's diagonal.  Bisection with relative moves on a mirrored
    16 x 8 pair, every step a compared frame, at most 24 steps.  The library tests its 16 half-rounded, padded sub-boxes, so the switch is nobody's to
    compute but its own."""
    key = (name, sem.name)
    if key in _switches:
        return _switches[key]
    zmax = DOLLY[name][0]
    pair = Pair(pkg, oracle, scenes, name, 16, 8, sem, capfd)
    dolly = np.linspace(0.0, zmax, 10).astype(F)
    fronts = []
    for z in dolly:
        pair.dolly_to(z); pair.clear()
        fronts.append(pair.render(1, "probe z %r" % float(z))[1].front)
    k = sum(fronts)
    assert 0 < k < len(dolly) and fronts == [1] * k + [0] * (len(dolly) - k), fronts          # in front first, then never again
    lo, hi = dolly[k - 1], dolly[k]
    width = 1e-5 * scene_diag(scenes(name))
    steps = 0
    while float(hi) - float(lo) >= width:
        steps += 1
        assert steps <= 24
        mid = F(0.5 * (float(lo) + float(hi)))
        assert lo < mid < hi
        pair.dolly_to(mid); pair.clear()
        if pair.render(1, "bisect z %r" % float(mid))[1].front:
            lo = mid
        else:
            hi = mid
    _switches[key] = (dolly, lo, hi)
    say(capfd, "\n[switch %s %s] front 1 at z = %.9g, front 0 at z = %.9g (%d bisection steps, diagonal %.4f)" % (name, sem.name, lo, hi, steps, scene_diag(scenes(name))))
    return _switches[key]


def graze_poses(lo, hi):
    """8 poses spread geometrically over the last factor 1e4 of the bracket, 4 on each side: the bracket's ends and 10^(4/3), 10^(8/3) and 10^4 bracket
    widths beyond them, alternating sides so that every step crosses the switch"""
    w = float(hi) - float(lo)
    out = []
    for k in (3, 2, 1, 0):
        s = 0.0 if k == 0 else w * 10.0 ** (4.0 * k / 3.0)
        out += [F(float(lo) - s), F(float(hi) + s)]
    return out


# ---- 1. dolly through the switch -------------------------------------------------------------------------------------------------------
SIZES = [(64, 48, 8), (96, 40, 3), (50, 34, 2)]
THAI2_SPP = 2
WIDEST_EXPECTED = 1e3


@pytest.mark.parametrize("name", ["4boxes", "ico2", "thai2"])
def test_dolly_through_the_switch(pkg, scenes, oracle, sem, monkeypatch, capfd, name):
    """10 dolly poses from the file's pose to behind everything, then 8 poses within 1e-5 ... 1e-1 of the scene's diagonal of the `front` switch, four on
    each side, on one mirrored pair per image size: 64 x 48 (sample groups of 8 — thai2: of 2 —, bins eligible), 96 x 40 (3 spp: groups of one) and
    50 x 34 (bins never eligible: rectangles, mask and verdicts only).  The film is cleared after every move and compared after every frame.
    thai2 runs at 2 spp.  Under the brute-force oracle (every ray against thai2's 20 049 triangles: 0.4 s per frame, not the 0.05 s of the other
    cases) its two further sizes take the 8 poses at the switch and the first and the last dolly pose, 10 frames of the 18; that case still takes 13 s.

    Measured on the MI355X (the same in both semantics): `front` is 1 up to z = 6.93364811 and 0 from 6.93370247 (4boxes), 7.28374577 /
    7.28385448 (ico2), 9.79397202 / 9.79410744 (thai2) — the library's 16 sub-boxes hug the geometry, so it holds on far longer than the root box would.
    The widest cull rectangle of a compared frame: 4.59e4 (4boxes), 6.95e4 (ico2), 7.35e4 (thai2), against a screen 0.72 wide; the coverage mask then has one
    cell set of one coarse domain, and the bins stand down on their own ("not built (exit 8)": lists of more than 24 triangles per tile)."""
    clean_env(monkeypatch)
    dolly, lo, hi = find_switch(pkg, oracle, scenes, sem, capfd, name)
    graze = graze_poses(lo, hi)
    inside_lo, inside_hi = DOLLY[name][1]
    seen = dict(front1_bins=0, front1_wide=0, front0=0, inside=0, witness=0, culled=0)
    widest = 0.0
    sizes = [(w, h, THAI2_SPP) for w, h, _ in SIZES] if name == "thai2" else SIZES
    short = name == "thai2" and bool(sem.orc & oracle.FLAG_BRUTE_FORCE)          # the slow oracle: fewer dolly poses at the second and third size
    for w, h, spp in sizes:
        pair = Pair(pkg, oracle, scenes, name, w, h, sem, capfd)
        graze_fronts = []
        for i, z in enumerate(list(dolly) + graze):
            near = i >= len(dolly)
            if short and (w, h) != SIZES[0][:2] and not near and 0 < i < len(dolly) - 1:
                continue
            pair.dolly_to(z); pair.clear()
            where = "z %.9g" % float(z)
            c, rep = pair.render(spp, where)
            say(capfd, "[%s %s %dx%dx%d] %s: %r hits %.3f culled %.3f" % (name, sem.name, w, h, spp, where, rep, c.primary_hits / c.primary, c.primary_culled / c.primary))
            if (w, h) == (50, 34):
                assert rep.bins is None, rep                                    # tiles would straddle row groups
            elif name == "thai2" and rep.front == 1:
                assert rep.bins is None and rep.bins_exit == 8, rep             # eligible, and declined: more than 24 triangles per tile
            if near:
                graze_fronts.append(rep.front)
                assert rep.front == (1 if z <= lo else 0), (where, rep)           # the side of the switch the probe pair found
            elif i == 0:
                assert rep.front == 1 and 0 < c.primary_hits < c.primary, (where, rep)      # the ordinary view
            elif i == len(dolly) - 1:
                assert rep.front == 0 and c.primary_hits == 0, (where, rep)     # past everything
            if not near and inside_lo <= float(z) <= inside_hi:
                assert pair.eye_inside_bounds() and rep.front == 0, (where, rep)
                assert c.primary_hits > 0.8 * c.primary, (where, c.primary_hits, c.primary)
                seen["inside"] += 1
            seen["front0"] += rep.front == 0
            seen["culled"] += c.primary_culled > 0
            if rep.front == 1:
                widest = max(widest, rep.widest)
                seen["front1_wide"] += rep.widest > WIDEST_EXPECTED
                seen["front1_bins"] += rep.bins is not None
            if rep.front == 1 and rep.bins is not None and (i == 0 or near):
                # second witness: the same pose through the tree walk visits more nodes (the bins take the primary rays' visits away), same film
                pair.rt.set_flags(sem.gpu | pkg.FLAG_COUNT_STEPS)
                pair.clear()
                cb, rb = pair.render(spp, where + " counted, bins")
                monkeypatch.setenv("MI355RT_NO_RASTER", "1")
                pair.clear()
                cw, rw = pair.render(spp, where + " counted, walk")
                monkeypatch.delenv("MI355RT_NO_RASTER")
                pair.rt.set_flags(sem.gpu)
                assert rb.bins_exit is None and rw.bins_exit == 1 and rw.bins is None
                assert cb.primary_hits == cw.primary_hits and cb.primary_culled == cw.primary_culled
                if cb.primary_hits:
                    assert cb.nodes_visited < cw.nodes_visited, (where, cb.nodes_visited, cw.nodes_visited)
                    seen["witness"] += 1
        assert sorted(graze_fronts) == [0] * 4 + [1] * 4, graze_fronts
    say(capfd, "[%s %s] widest cull rectangle of a compared frame: %.6g; %r" % (name, sem.name, widest, seen))
    if name != "thai2":                     # thai2's lists are longer than 24 triangles per tile at these sizes (asserted above): it never takes bins here
        assert seen["front1_bins"] > 0 and seen["witness"] > 0
    assert seen["front1_wide"] > 0, widest
    assert seen["front0"] > 0 and seen["inside"] > 0 and seen["culled"] > 0


# ---- 2. looking away and sideways ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4boxes", "ico2", "thai2"])
def test_looking_away_and_sideways(pkg, scenes, oracle, sem, monkeypatch, capfd, name):
    """Yaws of 0.3, 0.6, 0.9, 1.2, 1.6 and pi and a pitch of 1.2 from the file's pose, on one mirrored pair: the geometry leaves the image while it is
    still wholly in front (everything culled by the structures: the count of culled samples is the one computed without the verdict cache), then
    straddles the eye plane, then lies behind it (the structures stand down and every ray walks the tree to a miss)."""
    clean_env(monkeypatch)
    w, h, spp = 64, 48, 4
    pair = Pair(pkg, oracle, scenes, name, w, h, sem, capfd)
    yaw_now = F(0.0)
    miss_front1 = miss_front0 = 0
    poses = [("yaw", a) for a in (0.3, 0.6, 0.9, 1.2, 1.6, np.pi)] + [("pitch", 1.2)]
    for kind, a in poses:
        if kind == "yaw":
            d = F(F(a) - yaw_now); pair.yaw(float(d)); yaw_now = F(yaw_now + d)
        else:
            pair.yaw(float(-yaw_now)); pair.pitch(float(F(a)))          # back to the file's heading (to an ulp), then up
        pair.same_cameras()
        pair.clear()
        where = "%s %.4g" % (kind, a)
        c, rep = pair.render(spp, where)
        say(capfd, "[%s %s] %s: %r hits %d culled %d of %d" % (name, sem.name, where, rep, c.primary_hits, c.primary_culled, c.primary))
        if c.primary_hits == 0 and rep.front == 1:
            miss_front1 += 1
            assert c.primary_culled > 0, (where, rep)
            monkeypatch.setenv("MI355RT_NO_CULL_CACHE", "1")
            pair.clear()
            c2, rep2 = pair.render(spp, where + " without the verdict cache")
            monkeypatch.delenv("MI355RT_NO_CULL_CACHE")
            assert rep2.front == 1 and c2.primary_culled == c.primary_culled, (where, c.primary_culled, c2.primary_culled)
        if c.primary_hits == 0 and rep.front == 0:
            miss_front0 += 1
        if kind == "yaw" and a > 3.0:
            assert rep.front == 0 and c.primary_hits == 0, (where, rep)      # everything behind the eye
    assert miss_front1 > 0 and miss_front0 > 0, (miss_front1, miss_front0)


@pytest.mark.parametrize("name", ["4boxes", "ico2"])
def test_eye_inside_looking_back(pkg, scenes, oracle, sem, monkeypatch, capfd, name):
    """move_rel(0, 0, 12), add_y_angle(2.5), add_x_angle(0.4): the eye inside the geometry, looking back and down — ico2: every primary ray hits;
    4boxes: 88 % do in the reference's default semantics, all of them with true closest hits."""
    clean_env(monkeypatch)
    w, h, spp = 64, 48, 4
    pair = Pair(pkg, oracle, scenes, name, w, h, sem, capfd)
    pair.move(0.0, 0.0, 12.0); pair.yaw(2.5); pair.pitch(float(F(0.4)))
    pair.same_cameras()
    assert pair.eye_inside_bounds()
    c, rep = pair.render(spp, "inside, looking back")
    assert rep.front == 0 and c.primary == 12288
    if name == "ico2":
        assert c.primary_hits == c.primary
    else:                                   # the reference's octree drops the hits that lie on its root cube's bounds; the true closest hit keeps all
        assert 0.8 * c.primary < c.primary_hits <= c.primary
    for _ in range(2):
        pair.frame(); pair.same_pixels("50-row frame")
    pair.same_film("after the 50-row frames")


# ---- 3. one handle across the switch and back ------------------------------------------------------------------------------------------
def run_crossing(pkg, oracle, scenes, sem, capfd, name, stops, clear):
    """outside -> just before the switch -> inside -> outside again on ONE pair.  At each stop a whole frame of 8 spp, then two 50-row frames (the second
    takes over the frame launched behind the first; the one launched behind the second is given back by the move that follows).  Every read-out of the
    film's planes gives a speculated frame back, so after a 50-row frame only the packed pixels of its own rows and the call's counters are compared;
    the sums and squares those frames wrote are compared bit for bit once the next whole frame has settled the speculation — in the run that keeps the
    film, and at the last stop.  In the run that clears the film after each move, the 50-row frames of the first three stops are held through pixels and
    counters alone.  Returns what a run under another setting of the library's switches must repeat bit for bit: the film after every stop's whole
    frame and at the end, every call's counters, the reports."""
    w, h = 24, 104                                  # two 50-row windows that share no row: the library speculates
    pair = Pair(pkg, oracle, scenes, name, w, h, sem, capfd)
    trail = []
    for i, z in enumerate(stops):
        pair.dolly_to(z)
        if clear:
            pair.clear()
        where = "stop %d z %.9g" % (i, float(z))
        # the whole frame gives back the frame speculated at the stop before (with the film kept, its rows must read as if it had never run);
        # compared on the film's bits, and the read-out leaves no row dirty
        c, rep = pair.render(8, where)
        trail.append(("render", rep.front, c.primary, c.bounce, c.shadow, c.primary_hits, c.primary_culled))
        trail.append(("film",) + tuple(x.copy() for x in pair.rt.film.pixel_datas()))
        trail.append(("report", rep))
        launched0, taken0 = pair.rt.debug_speculation()
        for k in range(2):
            c = pair.frame(where)
            pair.same_pixels(where + " frame %d" % k)                           # reads the frame's own rows only: the speculated frame stays out
            trail.append(("frame", c.primary, c.bounce, c.shadow, c.primary_hits, c.primary_culled))
        launched, taken = pair.rt.debug_speculation()
        assert (launched - launched0, taken - taken0) == (2, 1), (where, launched0, taken0, launched, taken)
    pair.same_film("after the last stop")                                       # (this read-out gives the last speculated frame back)
    trail.append(("film",) + tuple(x.copy() for x in pair.rt.film.pixel_datas()))
    return trail


@pytest.mark.parametrize("clear", [True, False], ids=["clearing", "not_clearing"])
def test_one_handle_across_the_switch_and_back(pkg, scenes, oracle, sem, monkeypatch, capfd, clear):
    """The rectangles, mask, bins and verdicts cached for one regime are not read in the other, nor is the 50-row frame speculated behind the last call:
    ico2 at 24 x 104, the film cleared after each move or (allowed, if not what the reference's loop does) kept.  The whole sequence again without the
    verdict cache and without the bins: bit-equal films and equal counters, `primary_culled` included."""
    name = "ico2"
    clean_env(monkeypatch)
    dolly, lo, hi = find_switch(pkg, oracle, scenes, sem, capfd, name)
    inside = [z for z in dolly if DOLLY[name][1][0] <= float(z) <= DOLLY[name][1][1]][0]
    stops = [F(0.0), lo, inside, F(0.0)]
    plain = run_crossing(pkg, oracle, scenes, sem, capfd, name, stops, clear)
    reps = [t[1] for t in plain if t[0] == "report"]
    say(capfd, "\n[crossing %s] %r" % (sem.name, reps))
    assert [r.front for r in reps] == [1, 1, 0, 1]
    assert reps[0].bins is not None and reps[0].mask_cells is not None          # built for the first pose ...
    assert reps[3].bins is not None and reps[3].mask_cells is not None          # ... and again on the way back: the keys hold the origin
    assert reps[1].widest > WIDEST_EXPECTED and reps[1].mask_cells is not None
    for env in ("MI355RT_NO_CULL_CACHE", "MI355RT_NO_RASTER"):
        monkeypatch.setenv(env, "1")
        other = run_crossing(pkg, oracle, scenes, sem, capfd, name, stops, clear)
        monkeypatch.delenv(env)
        assert len(other) == len(plain)
        for a, b in zip(plain, other):
            assert a[0] == b[0]
            if a[0] == "film":
                assert np.array_equal(a[3], b[3]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2])), env
            elif a[0] == "report":
                assert a[1].front == b[1].front
                if env == "MI355RT_NO_RASTER":
                    assert b[1].bins is None
            else:
                assert a == b, (env, a, b)


# ---- 4. read-outs that rest on the camera ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ico2", "thai2"])
def test_guides_and_tiles_at_the_switch(pkg, scenes, oracle, sem, monkeypatch, capfd, name):
    """At the file's pose, just before the switch and inside the geometry: get_guides equals the oracle's primary hits (the helper of
    test_gpu_denoise.py), and a render_tiles frame with a checkerboard mask equals the oracle per pixel (as test_gpu_tiles.py checks it)."""
    clean_env(monkeypatch)
    w, h = 37, 21
    dolly, lo, hi = find_switch(pkg, oracle, scenes, sem, capfd, name)
    inside = [z for z in dolly if DOLLY[name][1][0] <= float(z) <= DOLLY[name][1][1]][0]
    pair = Pair(pkg, oracle, scenes, name, w, h, sem, capfd)
    brute = bool(sem.orc & oracle.FLAG_BRUTE_FORCE)
    mask = checkerboard(w, h)
    on = pixels_of(mask, w, h)
    fronts, widest = [], 0.0
    for z in (F(0.0), lo, inside):
        pair.dolly_to(z); pair.clear()
        got = pair.rt.guides()
        assert_guides_equal(got, oracle_guides(pair.orc, pair.scene, w, h, False, brute))
        if z == inside:
            assert (got["prim"] != 0xFFFFFFFF).mean() > 0.8
        else:
            assert (got["prim"] != 0xFFFFFFFF).any() and (got["prim"] == 0xFFFFFFFF).any()
        snaps = {}
        c, rep = pair.render(2, "z %.9g" % float(z), compare=False)
        snaps[2] = pair.orc.film() + (pair.orc.get_pixels(), pair.orc.get_tonemapped_pixels())
        pair.rt.get_tonemapped_pixels()                                   # every row clean: the packed pixels below need render_tiles to mark its rows
        capfd.readouterr()
        ct = pair.rt.render_tiles(mask, 3)
        rep_t = one_report(capfd.readouterr().err)
        pair.orc.render(3, nthreads=16)
        snaps[5] = pair.orc.film() + (pair.orc.get_pixels(), pair.orc.get_tonemapped_pixels())
        assert 0 < on.sum() < w * h and ct.primary == 3 * int(on.sum())
        assert_matches_snapshots(pair.rt, snaps, np.where(on, 5, 2).astype(np.uint32))
        assert rep_t.front == rep.front
        fronts.append(rep.front); widest = max(widest, rep.widest if rep.front else 0.0)
    assert fronts == [1, 1, 0] and widest > WIDEST_EXPECTED
