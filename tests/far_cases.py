"""Scenes far from the origin and lights far from the scene: the cases of tests/test_far_proofs.py (CPU) and tests/test_gpu_far_scenes.py.

Every padding that lets the library leave work out is a fraction of the scene's diagonal; none knows how large the coordinates
themselves are.  One f32 ulp at 4096 is 4.9e-4: for a model ten units across that is already more than the BVH's 2e-5 of the diagonal.  moved()
translates a whole scene — vertices, lights, the position row of every camera — and far_light() carries light 0 away from the scene.  No case holds a
non-finite coordinate, and the largest offset stays inside the binary16 range, so the boxes the BVH ships are finite."""
import numpy as np

F = np.float32

SCENE_NAMES = ("4boxes", "ico2")                                    # 48 and 608 triangles
OFFSETS = ((0.0, 0.0, 0.0), (64.0, 64.0, 64.0), (4096.0, 4096.0, 4096.0), (5000.0, -3000.0, 17.0), (60000.0, 60000.0, 60000.0))
LIGHT_DIAGONALS = (30.0, 100.0, 1e4)                                # 30: hp + 0.01 l leaves the scene for some points and not for others
LIGHT_DIRECTION = (0.48, 0.64, 0.6)                                 # a unit vector; no axis, no face diagonal of a cube map

# (key, scene, offset, diagonals of the far light or None): the ten cases of the GPU test; the CPU proofs take every scene-offset pair and every distance
GPU_CASES = (
    ("4boxes+0", "4boxes", OFFSETS[0], None),
    ("ico2+0", "ico2", OFFSETS[0], None),
    ("4boxes+64", "4boxes", OFFSETS[1], None),
    ("4boxes+4096", "4boxes", OFFSETS[2], None),
    ("ico2+4096", "ico2", OFFSETS[2], None),
    ("4boxes+5000-3000+17", "4boxes", OFFSETS[3], None),
    ("ico2+5000-3000+17", "ico2", OFFSETS[3], None),
    ("ico2+60000", "ico2", OFFSETS[4], None),
    ("ico2 light 30", "ico2", OFFSETS[0], 30.0),
    ("4boxes light 1e4", "4boxes", OFFSETS[0], 1e4),
)
LBVH_CASE = "ico2+4096"                                             # also built on the device (FLAG_DEVICE_LBVH)


def box_of(scene):
    """(lo, hi, diag) of the scene's vertices, in double"""
    v = np.asarray(scene["tri_verts"], np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    return lo, hi, float(np.sqrt(((hi - lo) ** 2).sum()))


def moved(scene, offset):
    """a copy of the scene with `offset` added in f32 to every vertex, every light position and the position row (camera_matrix[3, :3]) of every
    camera; nothing else changes"""
    off = np.asarray(offset, F).reshape(3)
    sc = dict(scene)
    sc["tri_verts"] = (np.asarray(scene["tri_verts"], F).reshape(-1, 3, 3) + off).astype(F).reshape(-1, 9)
    lights = np.array(scene["lights"], F, copy=True)
    lights[:, :3] = (lights[:, :3] + off).astype(F)
    sc["lights"] = lights

    def cam(m):
        m = np.array(m, F, copy=True).reshape(16)
        m[12:15] = (m[12:15] + off).astype(F)
        return m
    sc["camera_matrix"] = cam(scene["camera_matrix"])
    sc["cameras"] = [(cam(m), fov) for m, fov in scene["cameras"]]
    return sc


def far_light(scene, diagonals, direction=LIGHT_DIRECTION):
    """a copy of the scene with light 0 at centre + direction * diagonals * diag, rounded to f32"""
    lo, hi, diag = box_of(scene)
    sc = dict(scene)
    lights = np.array(scene["lights"], F, copy=True)
    lights[0, :3] = (0.5 * (lo + hi) + np.asarray(direction, np.float64) * float(diagonals) * diag).astype(F)
    sc["lights"] = lights
    return sc


def case_scene(base, offset, diagonals):
    sc = moved(base, offset)
    return sc if diagonals is None else far_light(sc, diagonals)


def is_finite(scene):
    return bool(np.isfinite(scene["tri_verts"]).all() and np.isfinite(scene["lights"]).all() and all(np.isfinite(m).all() for m, _ in scene["cameras"]))


def light_diagonals(scene):
    """how many scene diagonals light 0 stands from the centre of the scene's box"""
    lo, hi, diag = box_of(scene)
    return float(np.linalg.norm(np.asarray(scene["lights"], np.float64)[0, :3] - 0.5 * (lo + hi))) / diag
