#!/usr/bin/env python3
"""Regenerates tests/golden/octree_tie_rays_4boxes_5.npy: 48 rays of 4boxes at 5 triangles per leaf on which the order among
octree children of equal slab distance decides the hit record.

They are the first 48 rays of test_octree_statement.statement_rays(tree, verts, seed=100, budget=400000) whose answer in the
numpy statement of the reference's walk (oracle/octree_statement.py) changes when children of equal t are taken in descending
instead of ascending order.  Needs no GPU and no built library; takes about a minute.

Run from the repo root:  python tests/golden/make_octree_tie_rays.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import test_octree_statement as t  # noqa: E402


def main(want=48, seed=100, budget=400000):
    import importlib
    ge.load_package()
    scene_io = importlib.import_module("raytracer_rs_amd.scene_io")
    sc = scene_io.load_scene_file(os.path.join(HERE, "scenes", "4boxes.scene"))
    S = t.statement()
    tree = S.build(sc["tri_verts"], 5)
    rays = t.statement_rays(tree, sc["tri_verts"], seed=seed, budget=budget)
    a_tuv, a_prim = S.intersect(tree, sc["tri_verts"], rays)
    b_tuv, b_prim = S.intersect(tree, sc["tri_verts"], rays, reverse_ties=True)
    differ = (a_prim != b_prim) | ((t.bits(a_tuv) != t.bits(b_tuv)).any(axis=1) & (a_prim != t.MISS))
    out = rays[differ][:want]
    assert out.shape[0] == want, "only %d rays found" % out.shape[0]
    np.save(t.TIE_RAYS, out)
    print("wrote %s: %d rays" % (t.TIE_RAYS, want))


if __name__ == "__main__":
    main()
