"""Hand-made surveys, placement cases and scenes for probe placement (include/mi355rt.h "PROBE PLACEMENT"), shared by
tests/test_probes_place_abi.py (the host side of csrc/probe_place.hpp against the numpy statement, and the statement's own outcomes on the hand-made scenes
through the CPU oracle) and tests/test_gpu_probes_place.py (the kernels against the same statement).  Not a test module."""
import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
W = H = 16
SEED = 5
INF = F(np.inf)


# ---- the points of the device tests: the recipe of tests/test_gpu_probes_vis.py, written out again ----------------------------------------------------------
_POINTS = {}


def probe_points(pkg, cams, scenes, name):
    """(points, ids): five free-space points around the camera, then points 0.05 off the scene's surfaces (the hit points of the camera's rays moved along the
    face normal turned against the ray), and random ids with repeats; computed once per scene and never written to"""
    if name not in _POINTS:
        sc = scenes(name)
        rt = pkg.create_raytracer_from_arrays(sc, pkg.DEFAULT_TRIANGLES_PER_LEAF, W, H, seed=SEED, flags=pkg.FLAG_TRUE_CLOSEST_HIT)
        origin = rt.camera.matrices()[1][12:15]
        rays = cams.pinhole(rt.camera.matrices(), W, H, 8, SEED)
        tuv, prim = rt.intersect_rays(rays)
        rt.close()
        hit = np.nonzero(prim != MISS)[0]
        hit = hit[np.random.default_rng(2).permutation(hit.size)][:280]
        assert hit.size >= 257
        o, d, t = rays[hit, :3], rays[hit, 3:], tuv[hit, 0]
        on = (o + t[:, None] * d).astype(F)
        v = sc["tri_verts"][prim[hit]].astype(np.float64)
        n = np.cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
        n /= np.linalg.norm(n, axis=1)[:, None]
        n[(n * d).sum(axis=1) > 0] *= -1
        free = origin[None] + np.array([[0, 0, 0], [0.1, 0.2, -0.1], [-0.3, 0.1, 0.2], [0.05, -0.2, 0.3], [0.2, 0.2, 0.2]], F)
        pts = np.ascontiguousarray(np.concatenate([free, on + F(0.05) * n.astype(F)]).astype(F))
        ids = np.random.default_rng(4).integers(0, 2**32, len(pts), dtype=np.uint64).astype(np.uint32)
        ids[1::7] = ids[0]                                   # repeats
        assert np.isfinite(pts).all()
        pts.setflags(write=False); ids.setflags(write=False)
        _POINTS[name] = (pts, ids)
    return _POINTS[name]


# ---- hand-made samples for probes.survey ------------------------------------------------------------------------------------------------------------------------
def hand_samples():
    """8 samples of 2 points over 3 triangles with normals +z, -x and a NaN normal: (t, prim, d, tri_normals, D).  Point 0 meets, in order: a front hit, a back
    hit, a front hit at the SAME t as the first, a NaN t, a zero t, a negative t, an infinite t (all misses), a back hit at the same t as the first back hit.
    Point 1: a hit on the NaN-normal triangle (front), a hit exactly at D, a hit beyond D, a miss, a nearer front hit, a front hit again at that t, a back hit,
    a miss."""
    D = F(2.0)
    N = np.array([[0, 0, 1], [-1, 0, 0], [np.nan, 0, 0]], F)
    dn, up, lf, rt = [0.0, 0.6, -0.8], [0.6, 0.0, 0.8], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]
    p0 = [(1.5, 0, dn), (0.7, 0, up), (1.5, 0, [0.6, 0.0, -0.8]), (np.nan, 0, dn), (0.0, 0, dn), (-1.0, 0, dn), (np.inf, 0, dn), (0.7, 1, lf)]
    p1 = [(0.9, 2, up), (2.0, 0, dn), (3.5, 0, [0.0, 0.0, -1.0]), (0.3, MISS, rt), (0.4, 1, rt), (0.4, 0, dn), (0.25, 0, up), (7.0, MISS, up)]
    t = np.array([[a[0], b[0]] for a, b in zip(p0, p1)], F).reshape(-1)
    prim = np.array([[a[1], b[1]] for a, b in zip(p0, p1)], np.uint32).reshape(-1)
    d = np.array([[a[2], b[2]] for a, b in zip(p0, p1)], F).reshape(-1, 3)
    return t, prim, d, N, D


# ---- hand-made surveys for probes.place / probes.classify -----------------------------------------------------------------------------------------------------------
GRID = dict(origin=np.array([0.0, 0.0, 0.0], F), spacing=np.array([1.0, 0.5, 2.0], F), counts=np.array([4, 3, 4], np.uint32))
FLAT = dict(origin=np.array([0.0, 0.0, 0.0], F), spacing=np.array([1.0, 1.0, 1.0], F), counts=np.array([3, 1, 2], np.uint32))       # y has one probe
MIN_FRONT, D_PLACE = 0.2, 3.0


def _rec(dist, d):
    return [dist] + list(d)


EMPTY_NEAR, EMPTY_FAR = _rec(np.inf, (0, 0, 0)), _rec(-np.inf, (0, 0, 0))


def place_cases(nprobes=48):
    """(names, survey dict, offsets) of nprobes hand-made probes: one row per situation, the list repeated to fill the grid.  Every branch of PLACE occurs, each
    both accepted and refused where it can be refused."""
    u = lambda v: list(np.asarray(v, np.float64) / np.linalg.norm(v))
    rows = [
        # name, (n, back, front), near_back, near_front, far, offset
        ("unsampled", (0, 0, 0), EMPTY_NEAR, EMPTY_NEAR, EMPTY_FAR, (0.1, 0.0, 0.0)),
        ("through", (64, 40, 24), _rec(0.05, u((1, 1, 0))), _rec(0.5, u((0, 0, 1))), _rec(3.0, (0, 1, 0)), (0, 0, 0)),
        ("through refused", (64, 64, 0), _rec(0.4, (0, 1, 0)), EMPTY_NEAR, EMPTY_FAR, (0, 0, 0)),                 # 0.4 + 0.1 along y: 0.5 >= 0.45 * 0.5
        ("through at the share", (64, 16, 48), _rec(0.05, (1, 0, 0)), _rec(1.0, (0, 0, 1)), _rec(3.0, (0, 1, 0)), (0, 0, 0)),      # 0.25 is not > 0.25: rest
        ("through on the bound", (8, 8, 0), _rec(0.35, (1, 0, 0)), EMPTY_NEAR, EMPTY_FAR, (0, 0, 0)),            # 0.35 + 0.1 = 0.45 * 1.0 in f32: refused
        ("away", (64, 0, 30), EMPTY_NEAR, _rec(0.02, (0, 0, -1)), _rec(3.0, u((0.3, 0.1, 1))), (0, 0, 0)),
        ("away short far", (64, 0, 64), EMPTY_NEAR, _rec(0.02, (0, 0, -1)), _rec(0.11, (0, 0, 1)), (0.05, 0, 0)),   # the step is far.dist, not min_front
        ("away refused", (64, 0, 30), EMPTY_NEAR, _rec(0.02, (0, -1, 0)), _rec(3.0, (0, 1, 0)), (0, 0.1, 0)),      # 0.1 + 0.2 >= 0.225
        ("stay", (64, 0, 30), EMPTY_NEAR, _rec(0.02, (0, 0, -1)), _rec(3.0, u((0, 0.5, -1))), (0, 0, 0)),          # the farthest way is within 60 degrees
        ("at 60 degrees", (64, 0, 30), EMPTY_NEAR, _rec(0.02, (1, 0, 0)), _rec(3.0, (0.5, 0, 0.8660254)), (0, 0, 0)),       # dot == 0.5 |nf| |far| in f32: <= holds
        ("inside 60 degrees", (64, 0, 30), EMPTY_NEAR, _rec(0.02, (1, 0, 0)), _rec(3.0, (0.51, 0, 0.86)), (0, 0, 0)),
        ("away zero far", (64, 0, 30), EMPTY_NEAR, _rec(0.02, (0, 0, -1)), _rec(3.0, (0, 0, 0)), (0, 0, 0)),       # 0 / 0: refused
        ("back part", (64, 0, 10), EMPTY_NEAR, _rec(0.3, (1, 0, 0)), _rec(3.0, (0, 1, 0)), (0.3, 0.0, 0.4)),        # room 0.1 of 0.5
        ("back whole", (64, 0, 10), EMPTY_NEAR, _rec(2.0, (1, 0, 0)), _rec(3.0, (0, 1, 0)), (0.3, 0.1, -0.4)),
        ("back empty", (64, 0, 0), EMPTY_NEAR, EMPTY_NEAR, _rec(3.0, (0, 1, 0)), (-0.2, 0.0, 0.0)),
        ("back at min_front", (64, 0, 10), EMPTY_NEAR, _rec(F(MIN_FRONT), (1, 0, 0)), _rec(3.0, (0, 1, 0)), (0.3, 0.0, 0.0)),      # room 0: the candidate is the offset
        ("rest", (64, 3, 10), _rec(1.0, (1, 0, 0)), _rec(0.9, (0, 0, 1)), _rec(3.0, (0, 1, 0)), (0, 0, 0)),
        ("rest idle", (64, 0, 0), EMPTY_NEAR, EMPTY_NEAR, _rec(3.0, (0, 1, 0)), (0, 0, 0)),
        ("rest front at D", (64, 0, 5), EMPTY_NEAR, _rec(3.0, (0, 0, 1)), _rec(3.0, (0, 0, 1)), (0, 0, 0)),        # a front hit AT max_distance: idle
        ("through overflow", (2, 2, 0), _rec(3e38, (2, 0, 0)), EMPTY_NEAR, EMPTY_FAR, (0, 0, 0)),                  # the step overflows: refused
        ("through denormal", (2, 2, 0), _rec(1e-44, (1e-3, 0, 0)), EMPTY_NEAR, EMPTY_FAR, (0, 0, 0)),              # dist denormal, the step 1e-4
        ("away denormal", (9, 0, 9), EMPTY_NEAR, _rec(1e-40, (0, 0, -1)), _rec(1e-42, (0, 0, 1e-30)), (0, 0, 0)),   # far's length underflows: 0 -> refused
        ("nan share record", (5, 5, 0), _rec(np.nan, (1, 0, 0)), _rec(0.1, (0, 0, -1)), _rec(3.0, (0, 0, 1)), (0, 0, 0)),     # a NaN near_back counts as empty
        ("buried no way", (64, 64, 0), _rec(0.6, (0, 0, 1)), EMPTY_NEAR, EMPTY_FAR, (0, 0, 0)),                   # 0.7 of a spacing 2.0: accepted on z
        ("back negative zero", (64, 0, 0), EMPTY_NEAR, EMPTY_NEAR, _rec(3.0, (0, 1, 0)), (-0.0, 0.0, 0.0)),        # -0 is 0: rest
    ]
    rows = (rows * (nprobes // len(rows) + 1))[:nprobes]
    sv = dict(n=np.array([r[1][0] for r in rows], np.uint32), back=np.array([r[1][1] for r in rows], np.uint32), front=np.array([r[1][2] for r in rows], np.uint32),
              near_back=np.array([r[2] for r in rows], F), near_front=np.array([r[3] for r in rows], F), far=np.array([r[4] for r in rows], F), max_distance=D_PLACE)
    return [r[0] for r in rows], sv, np.ascontiguousarray(np.array([r[5] for r in rows], F))


def random_surveys(nprobes, seed, grid):
    """(survey, offsets) of nprobes fixed-seed probes whose numbers cluster around the decisions: shares around back_share, distances around min_front and
    max_distance, offsets around the bound"""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 65, nprobes).astype(np.uint32)
    back = (rng.random(nprobes) * 0.5 * n).astype(np.uint32)
    front = ((n - back) * rng.random(nprobes)).astype(np.uint32)
    unit = lambda: (lambda v: v / np.linalg.norm(v, axis=1)[:, None])(rng.normal(size=(nprobes, 3)))
    nb = np.concatenate([rng.uniform(0.0, 0.6, (nprobes, 1)), unit()], axis=1).astype(F)
    nf = np.concatenate([rng.uniform(0.0, 0.5, (nprobes, 1)), unit()], axis=1).astype(F)
    far = np.concatenate([rng.uniform(0.05, D_PLACE, (nprobes, 1)), unit()], axis=1).astype(F)
    nf[rng.random(nprobes) < 0.15] = EMPTY_NEAR
    nf[rng.random(nprobes) < 0.1, 0] = F(D_PLACE)
    nb[back == 0] = EMPTY_NEAR
    off = (rng.uniform(-0.5, 0.5, (nprobes, 3)) * np.asarray(grid["spacing"], np.float64)).astype(F)
    off[rng.random(nprobes) < 0.4] = 0
    off[:, [a for a in range(3) if int(grid["counts"][a]) == 1]] = 0
    return dict(n=n, back=back, front=front, near_back=nb, near_front=nf, far=far, max_distance=D_PLACE), np.ascontiguousarray(off)


# ---- hand-made scenes -------------------------------------------------------------------------------------------------------------------------------------------
def box(centre, half):
    """12 triangles of a closed axis-aligned box, wound so that every normal cross(v1 - v0, v2 - v0) points outwards: float32 (12, 9)"""
    c = np.asarray(centre, np.float64)
    tris = []
    for a in range(3):
        b, e = (a + 1) % 3, (a + 2) % 3
        for s in (-1.0, 1.0):
            q = []
            for sb, se in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = c.copy(); p[a] += s * half; p[b] += sb * half; p[e] += se * half
                q.append(p)
            for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
                tris.append(np.concatenate(tri if n[a] * s > 0 else (tri[0], tri[2], tri[1])))
    return np.array(tris, F)


def quad(p0, ex, ey):
    """two triangles of the parallelogram p0, p0 + ex, p0 + ex + ey, p0 + ey with the normal cross(ex, ey): float32 (2, 9)"""
    p0, ex, ey = (np.asarray(v, np.float64) for v in (p0, ex, ey))
    return np.array([np.concatenate([p0, p0 + ex, p0 + ex + ey]), np.concatenate([p0, p0 + ex + ey, p0 + ey])], F)


def scene_of(tris):
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    cam = np.eye(4, dtype=F).reshape(-1)
    return dict(tri_verts=tris, tri_geom=np.zeros(len(tris), np.uint32), mat_kind=np.zeros(1, np.uint32), mat_rgb=np.array([[0.8, 0.7, 0.6]], F),
                mat_tex=np.zeros(1, np.uint32), lights=np.array([[1.3, 2.6, 1.4, 30.0, 30.0, 30.0]], F), textures=[], camera_matrix=cam, camera_fov=F(60.0))


GRID3 = dict(origin=np.array([0.0, 0.0, 0.0], F), spacing=np.array([1.0, 1.0, 1.0], F), counts=np.array([3, 3, 3], np.uint32))
CENTRE = 13                                                     # probe (1, 1, 1) of GRID3, at (1, 1, 1)
FLOOR = quad((-4.0, -0.5, 6.0), (10.0, 0.0, 0.0), (0.0, 0.0, -10.0))      # y = -0.5, its normal +y: the probes stand above it
SPECK = quad((50.0, 50.0, 50.0), (0.01, 0.0, 0.0), (0.0, 0.01, 0.0))      # a scene needs a triangle: one that no probe ever sees within reach
GRID_WALL = dict(origin=np.array([0.0, 0.0, 0.02], F), spacing=np.array([1.0, 1.0, 1.0], F), counts=np.array([2, 2, 2], np.uint32))
WALL = quad((-6.0, -6.0, 0.0), (14.0, 0.0, 0.0), (0.0, 14.0, 0.0))         # z = 0, its normal +z: the probes with z = 0.02 stand 0.02 in front of it


def scene_a():
    """(a) a buried probe that can be saved: a closed box of half-size 0.1 around the centre probe of GRID3, above a floor"""
    return scene_of(np.concatenate([box((1, 1, 1), 0.1), FLOOR]))


def scene_b():
    """(b) a buried probe out of reach: the same box with half-size 0.6"""
    return scene_of(np.concatenate([box((1, 1, 1), 0.6), FLOOR]))


def scene_c():
    """(c) probes 0.02 in front of a large wall (GRID_WALL)"""
    return scene_of(np.concatenate([WALL, SPECK]))


def scene_d():
    """(d) empty space, and (c) with the wall taken out"""
    return scene_of(SPECK)


class OracleTracer:
    """probes_survey and probes_place of a RayTracer on the CPU: gather.rays -> the oracle's brute-force closest hits -> the statement.  What probes.relocate
    needs of its `rt`, so that the statement's outcomes on the hand-made scenes can be checked without a GPU."""

    def __init__(self, oracle, ga, pr, features, scene):
        self.ga, self.pr = ga, pr
        self.orc = oracle.Oracle(scene, W, H, seed=SEED, flags=oracle.FLAG_BRUTE_FORCE)
        self.table = self.orc.sample_table()
        self.normals = features.tri_normals(scene)
        self.rays = 0

    def probes_survey(self, points, ids=None, spp=64, first_sample=0, max_distance=None, flip=False, into=None):
        rays, keys, valid, w = self.ga.rays(self.table, SEED, points, None, ids, first_sample, spp)
        tuv, prim = self.orc.intersect(rays, brute=True)
        self.rays += len(rays)
        return self.pr.survey(tuv[:, 0], prim, rays[:, 3:], self.normals, len(points), max_distance, flip, into)

    def probes_place(self, grid, survey, offsets=None, back_share=0.25, max_offset=0.45, min_front=None, want=("offsets", "verdict", "state")):
        min_front = self.pr.grid_min_front(grid) if min_front is None else min_front
        off, verdict = self.pr.place(survey, offsets, grid, back_share, max_offset, min_front, want_verdict=True)
        res = dict(offsets=off, verdict=verdict, state=self.pr.classify(survey, back_share))
        return tuple(res[w] for w in want)

    def close(self):
        self.orc.close()
