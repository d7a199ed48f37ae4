"""Scenes, masks and ray sets of the ray-mask tests (tests/test_mask_inputs.py on the CPU,
tests/test_gpu_masks.py on the GPU) beyond those of tests/visibility_scenes.py.  Everything here is
input.  A masked query is compared with a fresh oracle build of the scene that holds only the objects
the ray sees; that stands for inputs without equal-t ties between instances (or, for "stacked", with
ties inside one mesh only, whose order no mask changes), which the CPU test shows.

Masks by state: object i gets bit s iff it is visible in states[s], so a ray with mask 1 << s sees the
scene of state s."""
import copy
import os
import sys

import numpy as np

import myraytracer_amd as M
from myraytracer_amd import engine, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_scenes as DS                                                       # noqa: E402
import visibility_scenes as V                                                    # noqa: E402

POSED_STATES = ("all", "third", "one", "none")
GAP = 1e-9


def state_masks(case, states):
    """Per object of the case the mask with bit s set iff the object is visible in states[s]."""
    n = len(case.scene.objects)
    return [sum(1 << s for s, name in enumerate(states) if i not in case.states[name]) for i in range(n)]


def subset(sc, hidden):
    return engine.visible_subset(sc, [i not in hidden for i in range(len(sc.objects))])


# ---------------------------------------------------------------- (a) baked posed
_BAKED = {}


def baked_posed():
    """visibility_scenes.posed() with each of its twelve objects baked to world space as a Mesh of its
    own under the identity transform: a static identity scene (the identity walks).  Its states are
    posed's and its ray set is posed's without the rays that have, in one of the states all / third /
    one, a second triangle within 1e-9 relative of their closest t (baking rounds the vertices, so
    the condition is asked again).  Returns a visibility_scenes.Case with `dropped`, the number of
    rays left out."""
    if "case" in _BAKED:
        return _BAKED["case"]
    c = V.case("posed")
    sc = copy.copy(c.scene)
    objs = []
    for i, o in enumerate(c.scene.objects):
        tris = V.object_triangles(c.scene, i)
        objs.append(M.Mesh(id=o.id, material="1", positions=np.ascontiguousarray(tris.reshape(-1, 3)),
                           indices=np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3), indices_one_based=False,
                           shading_mode="flat"))
    sc.objects = objs
    O, D, tmax = c.rays
    keep = np.ones(len(O), bool)
    for state in ("all", "third", "one"):
        tris = V.all_triangles(subset(sc, c.states[state]))
        keep &= DS.closest_gap(tris, O, D, chunk=32)[1] > GAP
    case = V.Case(sc, dict(c.states), (O[keep], D[keep], tmax[keep]))
    case.dropped = int((~keep).sum())
    _BAKED["case"] = case
    return case


# ---------------------------------------------------------------- (b) stacked
def _stacked_mesh():
    hp, hf = scenes.heightfield(6, 4.0, 0.5, 3)
    return hp.astype(np.float32).astype(np.float64), hf.astype(np.int32)


def stacked_rays():
    """Rays straight down from 10 above A's vertices and edge midpoints (the construction of
    test_gpu_query's "grid" case): they meet A at shared vertices and edges, where two or more of its
    triangles give the same t, and B, two above A, first."""
    hp, hf = _stacked_mesh()
    a, b, c = hp[hf[:, 0]], hp[hf[:, 1]], hp[hf[:, 2]]
    pts = np.concatenate([hp, 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a)])
    O = pts + np.array([0.0, 10.0, 0.0])
    D = np.tile([0.0, -1.0, 0.0], (len(O), 1))
    return O, D, np.full(len(O), 9.0)


def stacked(baked=False):
    """Mesh A (object 0) and B (object 1), A translated by (0, 2, 0): a MeshInstance of A, or with
    `baked` a Mesh of its own with the translated vertices under the identity (a static identity
    scene).  A ray from above that hits A hits B first."""
    hp, hf = _stacked_mesh()
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    A_ = M.Mesh(id=1, material="1", positions=hp, indices=hf, indices_one_based=False, shading_mode="flat")
    if baked:
        B_ = M.Mesh(id=2, material="1", positions=hp + np.array([0.0, 2.0, 0.0]), indices=hf, indices_one_based=False,
                    shading_mode="flat")
    else:
        B_ = M.MeshInstance(id=2, base_mesh_id=1, material="1", transform=M.translation(0.0, 2.0, 0.0))
    sc.objects = [A_, B_]
    return sc


STACKED_SETS = {"A": frozenset({1}), "B": frozenset({0}), "AB": frozenset()}      # name -> hidden objects
STACKED_MASK = {"A": 1, "B": 2, "AB": 3}                                          # ray masks; A has bit 0, B bit 1
