"""Scenes, visibility states and ray sets of the instance-visibility tests (tests/test_visibility_inputs.py
on the CPU, tests/test_gpu_visibility.py on the GPU).  Everything here is input.  The GPU tests compare a
committed visibility state with a fresh oracle build of the scene that holds only the visible objects,
whose TLAS topology differs from the kept one; that comparison holds for inputs without equal-t ties
between instances, and the CPU test shows every (scene, state, ray set) used to be so.

A case is a scene, named states (each the set of HIDDEN object indices; "all" is the empty set) and one
ray set (origins, directions, tmax).  States of a case share the ray set, so the CPU test can also show
that hiding changes a good share of the answers."""
import copy
import os
import sys

import numpy as np

import myraytracer_amd as M
from myraytracer_amd import engine, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_scenes as DS                                                       # noqa: E402

FRAME = (48, 40)


class Case:
    def __init__(self, scene, states, rays, frame=False, tie_rule="triangle"):
        self.scene = scene                  # every object visible
        self.states = states                # name -> frozenset of hidden object indices
        self.rays = rays                    # (O, D, tmax)
        self.frame = frame                  # the GPU tests render frames of this case
        # "triangle": no ray has a second triangle within 1e-9 relative of its closest t.
        # "instance": the rays are aimed at shared vertices and edges (ties inside one BLAS, whose
        # order no commit changes), so the condition is between instances: no two OBJECTS' closest
        # hits lie within 1e-9 relative.
        self.tie_rule = tie_rule

    def visible(self, state):
        """The scene of the state: only the visible objects (engine.visible_subset, which
        RayTracerEngine.visible_scene calls with the committed flags)."""
        hidden = self.states[state]
        return engine.visible_subset(self.scene, [i not in hidden for i in range(len(self.scene.objects))])


def reversed_objects(sc):
    """The same scene with its object order reversed: another TLAS build order."""
    out = copy.copy(sc)
    out.objects = list(sc.objects)[::-1]
    return out


def spread(k, seed=0):
    """Instance k's pose: a lattice cell of its own, rotated, scaled 0.2 .. 0.5."""
    rng = np.random.RandomState(1000 * seed + k)
    cell = np.array([k % 7, (k // 7) % 7, k // 49], np.float64) * 1.7 - 5.0
    return DS.m16(DS.rotation(rng) * rng.uniform(0.2, 0.5), cell + rng.uniform(-0.3, 0.3, size=3))


def _mat(m16):
    return np.asarray(m16, np.float64).reshape(4, 4).T


def _lit(sc, eye, at, light, power):
    sc.cameras[0] = M.Camera(position=eye, gaze_point=at, up=(0.0, 1.0, 0.0), fovy=50.0, near_distance=1.0,
                             image_resolution=FRAME, type="lookAt")
    sc.point_lights = [M.PointLight(light, (power, power, power))]
    return sc


def object_triangles(sc, i):
    """(T, 3, 3) world-space vertices of object i's triangles (none for a sphere or a plane)."""
    o = sc.objects[i]
    if isinstance(o, M.Triangle):
        v = np.asarray(o.vertices, np.float64).reshape(1, 3, 3)
    elif isinstance(o, (M.Mesh, M.MeshInstance)):
        b = o if isinstance(o, M.Mesh) else next(x for x in sc.objects if isinstance(x, M.Mesh) and x.id == o.base_mesh_id)
        idx = np.asarray(b.indices, np.int64).reshape(-1, 3) - (1 if b.indices_one_based else 0)
        v = np.asarray(b.positions, np.float64)[idx]
    else:
        return np.zeros((0, 3, 3))
    m = _mat(o.transform)
    return v @ m[:3, :3].T + m[:3, 3]


def all_triangles(sc):
    return np.concatenate([object_triangles(sc, i) for i in range(len(sc.objects))] or [np.zeros((0, 3, 3))])


def instance_gap(sc, O, D, skip_ids=()):
    """Per ray the relative gap between the closest hits of the two nearest OBJECTS (inf with fewer
    than two objects hit): deform_scenes.closest_gap's smallest t per object.  skip_ids: objects shown
    elsewhere to be hit by none of the rays."""
    ts = [DS.closest_gap(object_triangles(sc, i), O, D)[0] for i, o in enumerate(sc.objects)
          if getattr(o, "id", None) not in skip_ids and len(object_triangles(sc, i)) >= 2]
    if len(ts) < 2:
        return np.full(len(O), np.inf)
    t = np.sort(np.stack(ts, axis=1), axis=1)[:, :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.isfinite(t[:, 1]), (t[:, 1] - t[:, 0]) / t[:, 0], np.inf)


def aimed_at(tris, n, rng, near=0.3, far=3.0, up=None):
    """n rays towards random interior points of `tris` from origins `near` .. `far` away (`up`: the
    origins lie on that side of the target)."""
    t = tris[rng.randint(len(tris), size=n)]
    w = rng.dirichlet((2.0, 2.0, 2.0), size=n)
    target = np.einsum("nk,nkc->nc", w, t)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if up is not None:
        flip = d @ np.asarray(up, np.float64) > 0            # d points from the origin to the target
        d[flip] = -d[flip]
    return target - d * rng.uniform(near, far, size=(n, 1)), d


# ---------------------------------------------------------------- the cases
def posed():
    """Six heightfield meshes (1 .. 257 triangles) and a MeshInstance of each under rotated, scaled and
    partly mirrored poses (deform_scenes.base_scene).  "third": a third of the objects hidden, among
    them the largest mesh while its MeshInstance stays and a MeshInstance while its mesh stays."""
    sc = DS.base_scene("flat", sizes=(1, 2, 3, 63, 65, 257))
    dets = [np.linalg.det(_mat(o.transform)[:3, :3]) for o in sc.objects]
    assert min(dets) < 0 < max(dets)
    O, D, tmax, _ = DS.aimed_ray_set(sc, n=1200, seed=9)
    states = {"all": frozenset(), "third": frozenset({2, 5, 7, 9}), "none": frozenset(range(12)),
              "one": frozenset(range(12)) - {11}}
    return Case(sc, states, (O, D, tmax), frame=True)


def kinds():
    """A Mesh, a MeshInstance of it, a Sphere, a Plane, a Triangle and a second Mesh; one state per
    hidden kind, and "base": the base mesh hidden while its MeshInstance stays."""
    pos, faces = scenes.geometry_c2(48, 26)
    pos = pos.astype(np.float32).astype(np.float64)
    hp, hf = scenes.heightfield(6, 3.0, 0.4, 3)
    sc = scenes.scaled(scenes.scene_c2(inline=True), *FRAME)
    base = M.Mesh(id=1, material="1", positions=pos, indices=faces.astype(np.int32), indices_one_based=False,
                  shading_mode="smooth")
    sc.objects = [base,
                  M.MeshInstance(id=11, base_mesh_id=1, material="1",
                                 transform=DS.m16(DS.rotation(np.random.RandomState(3)) * 1.4, (-3.0, 1.0, 1.5))),
                  M.Sphere(center=(2.5, 0.3, 0.5), radius=0.7, material="1", transform=DS.m16(np.diag([1.5, 0.8, 1.2]), (1.0, 0.9, 2.0))),
                  M.Plane(center=(0.0, -1.5, 0.0), normal=(0.0, 1.0, 0.0), material="1"),
                  M.Triangle(vertices=((-3, -1, -3), (3, -1, -3), (0, 2, -3.5)), material="1"),
                  M.Mesh(id=2, material="1", positions=hp.astype(np.float32).astype(np.float64), indices=hf.astype(np.int32),
                         indices_one_based=False, shading_mode="flat", transform=DS.m16(np.eye(3), (0.5, 2.6, -0.5)))]
    _lit(sc, (0.5, 3.0, 9.0), (0.0, 0.3, 0.0), (3.0, 8.0, 6.0), 4.0e3)
    rng = np.random.RandomState(41)
    Os, Ds = [], []
    for i in (0, 1, 4, 5):
        o, d = aimed_at(object_triangles(sc, i), 220, rng, up=(0.0, 1.0, 0.0))
        Os.append(o); Ds.append(d)
    # the sphere: towards points of its (transformed) surface from outside, along the point's own direction
    m = _mat(sc.objects[2].transform)
    u = rng.normal(size=(220, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    surf = (np.asarray(sc.objects[2].center) + 0.7 * u) @ m[:3, :3].T + m[:3, 3]
    out = u @ m[:3, :3].T
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    Os.append(surf + out * rng.uniform(0.3, 2.0, size=(220, 1))); Ds.append(-out)
    # the plane: downward rays from above it, beside the other objects
    o = np.stack([rng.uniform(-9.0, 9.0, 220), rng.uniform(-1.4, -0.9, 220), rng.uniform(-9.0, 9.0, 220)], axis=1)
    d = rng.normal(size=(220, 3)); d[:, 1] = -np.abs(d[:, 1]) - 0.2
    Os.append(o); Ds.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    O, D = np.concatenate(Os), np.concatenate(Ds)
    tmax = rng.uniform(0.1, 12.0, size=len(O))
    states = {"all": frozenset(), "base": frozenset({0}), "instance": frozenset({1}), "sphere": frozenset({2}),
              "plane": frozenset({3}), "triangle": frozenset({4}), "mesh": frozenset({5})}
    return Case(sc, states, (O, D, tmax), frame=True)


LEAF6 = tuple(range(6))                    # the objects of the unsplittable TLAS leaf
GROUP_B = tuple(range(6, 18))              # the objects apart from it


def leaf6():
    """Six concentric icosphere shells (radii 1 .. 3.5 about one centre): their world bounds share one
    centre exactly, no plane separates the centroids, so the TLAS keeps them in ONE leaf of six
    (test_visibility_inputs shows it with the oracle's TLAS).  Twelve small meshes lie apart (group B)
    under TLAS inner nodes of their own.  Shells of different radii have no equal-t ties."""
    sv, sf = scenes.icosphere(2)
    sv = sv.astype(np.float32).astype(np.float64)
    assert np.array_equal(sv.min(0), -sv.max(0))
    hp, hf = scenes.heightfield(6, 4.0, 0.5, 3)
    hp = hp.astype(np.float32).astype(np.float64)
    centre = (-6.0, 1.0, 0.5)
    sc = scenes.scaled(scenes.scene_c1(8, 8), *FRAME)
    objs = [M.Mesh(id=1, material="1", positions=sv, indices=sf.astype(np.int32), indices_one_based=False,
                   shading_mode="flat", transform=DS.m16(np.eye(3), centre))]
    objs += [M.MeshInstance(id=10 + k, base_mesh_id=1, material="1", transform=DS.m16(np.eye(3) * (1.0 + 0.5 * k), centre))
             for k in range(1, 6)]
    objs.append(M.Mesh(id=2, material="1", positions=hp, indices=hf[:24].astype(np.int32), indices_one_based=False,
                       shading_mode="flat", transform=DS.m16(np.eye(3) * 0.4, (6.0, 0.0, 0.0))))
    for k in range(11):
        m = _mat(spread(k, seed=5)).copy()
        m[:3, 3] = m[:3, 3] * 0.6 + (9.0, 1.0, 0.0)
        objs.append(M.MeshInstance(id=30 + k, base_mesh_id=2, material="1", transform=tuple(m.T.reshape(-1))))
    sc.objects = objs
    _lit(sc, (1.0, 6.0, 22.0), (1.0, 0.5, 0.0), (2.0, 30.0, 25.0), 2.0e4)
    rng = np.random.RandomState(57)
    c = np.asarray(centre)
    # shells: rays from inside, between and outside the shells through random points near the centre
    o1 = c + DS._unit(rng, 500) * rng.uniform(0.0, 5.0, size=(500, 1))
    d1 = DS._unit(rng, 500)
    o2, d2 = [], []
    for i in GROUP_B:
        o, d = aimed_at(object_triangles(sc, i), 40, rng)
        o2.append(o); d2.append(d)
    O, D = np.concatenate([o1] + o2), np.concatenate([d1] + d2)
    tmax = rng.uniform(0.1, 8.0, size=len(O))
    states = {"all": frozenset(), "some_of_leaf": frozenset({5, 4, 2}), "whole_leaf": frozenset(LEAF6),
              "group_b": frozenset(GROUP_B)}
    return Case(sc, states, (O, D, tmax), frame=True)


POOL = 300
POOL_LIVE = (0, 1, 2, 255, 256, 257, 300)


def pool():
    """300 instances of a mesh of one triangle (one leaf run, one pair each).  State "live<L>": objects
    0 .. L - 1 visible.  Half of the rays aim at objects 0 and 1, which stay longest."""
    hp, hf = scenes.heightfield(6, 4.0, 0.5, 3)
    mesh = M.Mesh(id=1, material="1", positions=hp.astype(np.float32).astype(np.float64), indices=hf[:1].astype(np.int32),
                  indices_one_based=False, shading_mode="flat", transform=M.translation(0.0, 6.0, 0.0))
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [mesh] + [M.MeshInstance(id=10 + k, base_mesh_id=1, material="1", transform=spread(k)) for k in range(POOL - 1)]
    rng = np.random.RandomState(77)
    parts = [aimed_at(object_triangles(sc, 0), 300, rng, 0.05, 0.3), aimed_at(object_triangles(sc, 1), 300, rng, 0.05, 0.3)]
    # ... a quarter at the objects hidden in every state but the full one, a quarter at all of them
    parts.append(aimed_at(np.concatenate([object_triangles(sc, i) for i in range(257, POOL)]), 300, rng, 0.05, 0.3))
    parts.append(aimed_at(np.concatenate([object_triangles(sc, i) for i in range(POOL)]), 300, rng, 0.05, 0.3))
    O, D = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    tmax = rng.uniform(0.02, 2.0, size=len(O))
    states = {f"live{L}": frozenset(range(L, POOL)) for L in POOL_LIVE}
    states["all"] = states["live300"]
    return Case(sc, states, (O, D, tmax))


def many_pairs():
    """270 instances of a mesh of 64 leaf runs: 17,280 pairs (k_rb_pair_boxes' 68 partial unions),
    every other instance hidden."""
    hp, hf = scenes.heightfield(8, 4.0, 0.5, 3)
    mesh = M.Mesh(id=1, material="1", positions=hp.astype(np.float32).astype(np.float64), indices=hf.astype(np.int32),
                  indices_one_based=False, shading_mode="flat", transform=M.translation(0.0, 6.0, 0.0))
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [mesh] + [M.MeshInstance(id=10 + k, base_mesh_id=1, material="1", transform=spread(k)) for k in range(269)]
    rng = np.random.RandomState(78)
    allt = np.concatenate([object_triangles(sc, i) for i in range(0, 270, 9)])
    O, D = aimed_at(allt, 500, rng, 0.05, 0.6)
    tmax = rng.uniform(0.02, 2.0, size=len(O))
    return Case(sc, {"all": frozenset(), "every_other": frozenset(range(1, 270, 2))}, (O, D, tmax))


FAR_OBJECT, FAR_ID = 4, 90


def far():
    """Three posed instances of a small mesh near the origin and (object 4) C2's mesh as a translated
    instance at 1e6 (tests/test_gpu_wide_bound.py test_fit_tree_reaches_the_bound: local coordinates =
    the far geometry minus the offset, exactly).  Two near-vertex ray sets: at the near instances
    (the case's ray set) and at the far mesh (far_rays)."""
    from test_gpu_wide_bound import _far_c2, _near_vertex_rays
    from test_wide_build import posed as pose, small_scene
    fsc, scale, off = _far_c2("1e6")
    fm = fsc.objects[0]
    Pw, F = np.asarray(fm.positions), np.asarray(fm.indices)
    sc = small_scene([pose(0), pose(1), pose(2)], base_at=(2.0, 0.0, 0.0))
    local = Pw - off
    assert np.array_equal(local + off, Pw)
    sc.objects.append(M.Mesh(id=FAR_ID, material="1", positions=local, indices=F.astype(np.int32), indices_one_based=False,
                             shading_mode=fm.shading_mode, transform=M.translation(*off)))
    assert len(sc.objects) == FAR_OBJECT + 1
    rng = np.random.RandomState(61)
    Of, Df = _near_vertex_rays(Pw, F, 12000, rng, 3.0 * scale)
    near = sc.objects[0]
    P0, F0 = np.asarray(near.positions), np.asarray(near.indices)
    Os, Ds = [], []
    for i in range(4):
        m = _mat(sc.objects[i].transform)
        o, d = _near_vertex_rays(P0 @ m[:3, :3].T + m[:3, 3], F0, 500, rng, 2.0)
        Os.append(o); Ds.append(d)
    O, D = np.concatenate(Os), np.concatenate(Ds)
    case = Case(sc, {"all": frozenset(), "far_hidden": frozenset({FAR_OBJECT})}, (O, D, rng.uniform(0.1, 8.0, size=len(O))),
                tie_rule="instance")
    case.far_rays = (Of, Df, np.full(len(Of), 10.0 * scale))
    return case


def combined():
    """Visibility with the other commits (deform_scenes.combined_case: meshes of 3, 65 and 257 triangles
    as objects 0 .. 2, a MeshInstance of each as objects 3 .. 5).  Returns the scene as built, the ray
    set and the steps, each one commit: what it stages (vis: object -> flag, moves: object -> matrix,
    positions: object -> array), the scene it leaves (every object, at its pose) and the hidden set.
      1  hides object 1, moves objects 5 and 0 and deforms mesh 2, in one commit
      2  hides object 2 (the deformed mesh's own instance; its MeshInstance, object 5, stays)
      3  while hidden: mesh 2 deformed again and object 2's transform changed
      4  shows object 2: it has the pose it would have had"""
    sc, pose, moves = DS.combined_case()
    steps = []
    cur = DS.applied(sc, pose)
    for i, m in moves.items():
        cur.objects[i].transform = m
    steps.append(dict(vis={1: False}, moves=moves, positions={2: pose[2][0]}, scene=cur, hidden=frozenset({1})))
    steps.append(dict(vis={2: False}, moves={}, positions={}, scene=cur, hidden=frozenset({1, 2})))
    nxt = copy.deepcopy(cur)
    p2 = DS.small_step(np.asarray(cur.objects[2].positions, np.float64), 4) * np.array([1.0, 1.6, 1.0])
    m2 = _mat(cur.objects[2].transform).copy()
    m2[:3, 3] += (-4.0, 3.0, 1.0)
    m2 = tuple(float(x) for x in m2.T.reshape(-1))
    nxt.objects[2].positions = p2
    nxt.objects[2].transform = m2
    steps.append(dict(vis={}, moves={2: m2}, positions={2: p2}, scene=nxt, hidden=frozenset({1, 2})))
    steps.append(dict(vis={2: True}, moves={}, positions={}, scene=nxt, hidden=frozenset({1})))
    # a third of the rays at object 2 where step 2 hides it, a third where step 4 shows it
    rng = np.random.RandomState(14)
    parts = [aimed_at(object_triangles(cur, 2), 300, rng), aimed_at(object_triangles(nxt, 2), 300, rng),
             aimed_at(all_triangles(nxt), 300, rng, 0.3, 25.0)]
    O, D = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return sc, (O, D, rng.uniform(0.1, 30.0, size=len(O))), steps


CASES = {f.__name__: f for f in (posed, kinds, leaf6, pool, many_pairs, far)}
_BUILT = {}


def case(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]
