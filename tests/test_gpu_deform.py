"""Deforming meshes (rtcore.h RT_SCENE_DEFORMABLE; myraytracer_amd/csrc/deform.h): new vertex
positions staged with rt_scene_set_mesh_positions, the BLAS refit on the device by rt_scene_commit
with the reference's refit semantics (BVHBuilder.refit, BVH.swift:254-291).

Every comparison is with the oracle of the engine's mirrored scene (oracle.OracleScene(eng.scene))
or with the numpy restatements of tests/wide_tree_check.py, never with the engine itself except
where two engine states must be equal.  A deformed pose is compared with the oracle only on the
tie-free inputs of tests/deform_scenes.py (tests/test_deform_inputs.py shows them tie-free on the
CPU); ties are covered by the round trip back to the build pose, where the kept topology is the
fresh one."""
import copy
import dataclasses
import os
import sys

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import scenes
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_scenes as DS                                                       # noqa: E402
import wide_tree_check as W                                                      # noqa: E402
from test_gpu_rays import _twin_meshes                                           # noqa: E402
from test_gpu_refit import WALKS, _assert_frame, _assert_rays, _mat              # noqa: E402
from test_gpu_refit_edges import _mismatches, _ref, _tmax                        # noqa: E402
from test_gpu_wide_bound import _near_vertex_rays, _touching_grid, _touching_rays   # noqa: E402

pytestmark = pytest.mark.gpu


def _engine(sc, walk="transformed", devices=None, deformable=True, dynamic=False):
    """An engine that remembers the TLAS leaves of the scene as built (a refit keeps them)."""
    leaf_of = W.tlas_leaves(sc) if deformable else None
    eng = M.RayTracerEngine(sc, devices, dynamic=dynamic, deformable=deformable)
    for k, v in WALKS[walk].items():
        eng.set_option(k, v)
    eng.leaf_of = leaf_of
    return eng


def _stage(eng, pose):
    for i, (p, n) in pose.items():
        eng.set_positions(i, p, n)


_REF = {}


def _reference(key, sc, O, D, tmax, time):
    """The oracle's hits, occlusion and frame of scene sc, computed once per key."""
    if key not in _REF:
        osc = oracle.OracleScene(sc)
        _REF[key] = ((osc.trace_rays(O, D, None, time), osc.occluded_rays(O, D, tmax, time)),
                     osc.render(0, threads=0, rgba=True))
        osc.close()
    return _REF[key]


def _assert_frame_ref(eng, frame):
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)
    ref, ref8, ost = frame
    assert float(np.abs(rgb - ref).max()) <= 1e-5
    assert np.array_equal(rgba, ref8)
    assert (st.primary_rays, st.shadow_rays, st.secondary_rays) == (ost.primary_rays, ost.shadow_rays, ost.secondary_rays)


def _scalars(d):
    return {k: d[k] for k in ("wide_coord", "fit_blocked", "wide_root", "fit_root")}


def _same_state(a, b, a_is_build=False):
    """Two read-backs describe the same trees: per node the same (ref, box) multisets (k_octant_copies
    sorts copy 0 stably from its earlier order, so the order among equal keys depends on history),
    the same leaf boxes, instance data and scalars.  fit_coord: a build holds the largest magnitude
    its pairs have, a commit the host bound of scene.cpp refit_host_scene, which is never below it
    (tests/test_gpu_refit_edges.py); two committed states must agree exactly."""
    n = int(a["wide_copy"])
    assert n == int(b["wide_copy"])
    assert np.array_equal(W.node_multisets(a, 0, n), W.node_multisets(b, 0, n))
    for k in ("lbox", "tbox", "bcoord", "inst_bounds", "l2w", "wroot", "fpairs"):
        assert np.array_equal(a[k], b[k]), k
    assert _scalars(a) == _scalars(b)
    assert (a["fit_coord"] <= b["fit_coord"]) if a_is_build else (a["fit_coord"] == b["fit_coord"])


def _baseline(eng):
    """The read-back every later state is compared with, exactly.  It is taken after a commit that
    changes nothing (an instance's own matrix staged again), so that fit_coord is the commit's host
    bound (scene.cpp refit_host_scene) as in every later state; the build's read-back agrees with
    it in everything but fit_coord, which a build takes from its pairs' largest magnitude."""
    built = eng.wide_read(0)
    i = next(i for i in range(len(eng.scene.objects)) if eng.instance_of(i) >= 0)
    eng.set_transform(i, eng.scene.objects[i].transform)
    assert eng.commit().instances_moved == 1
    base = eng.wide_read(0)
    _same_state(built, base, a_is_build=True)
    return base


# ---------------------------------------------------------------- 1. rays and frames at a deformed pose
@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("variant", DS.VARIANTS)
def test_rays_at_a_deformed_pose(variant, walk):
    sc = DS.base_scene(variant)
    eng = _engine(sc, walk)
    assert eng.get_option("compact_tris") == 1                      # the option stands; the layouts are FP64
    for i in DS.mesh_indices(sc):
        assert eng.vertex_count(i) == len(sc.objects[i].positions)
    _stage(eng, DS.pose_b(sc, with_normals=variant == "supplied_new"))
    st = eng.commit()
    ds = eng.last_deform_stats()
    assert st.instances_moved == 0
    assert (ds.meshes_deformed, ds.triangles, ds.instances_rebounded) == (len(DS.SIZES), sum(DS.SIZES), 2 * len(DS.SIZES))
    O, D, tmax, time = DS.ray_set()
    tm = time if variant == "blur" else None
    rays, frame = _reference(variant, eng.scene, O, D, tmax, tm)
    assert np.isfinite(rays[0][0]).sum() > len(O) // 10
    _assert_rays(eng, rays, O, D, tmax, tm)
    if walk == "transformed":                                       # shading normals: flat, supplied, derived
        _assert_frame_ref(eng, frame)
    eng.close()


# ---------------------------------------------------------------- 2. structure, two replicas
@pytest.mark.parametrize("variant", ["flat", "smooth"])
def test_structure_after_a_deformation_on_two_replicas(variant):
    sc = DS.base_scene(variant)
    eng = _engine(sc, devices=[0, 0])
    built = eng.wide_read(0)
    W.assert_ok(built, eng.scene)
    _stage(eng, DS.pose_b(sc))
    eng.commit()
    d0, d1 = eng.wide_read(0), eng.wide_read(1)
    assert W.same_dump(d0, d1) is None, f"the replicas differ in {W.same_dump(d0, d1)}"
    W.assert_ok(d0, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    assert not np.array_equal(built["lbox"], d0["lbox"]) and not np.array_equal(built["bcoord"], d0["bcoord"])
    O, D, tmax, _ = DS.ray_set(400, seed=5)
    osc = oracle.OracleScene(eng.scene)
    ref = (osc.trace_rays(O, D), osc.occluded_rays(O, D, tmax))
    osc.close()
    for slot in (0, 1):
        t = eng.trace_rays(O, D, slot=slot)[0]
        assert np.array_equal(t, ref[0][0])
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)                  # rows shared by the two replicas
    _assert_frame(eng, rgb, rgba, st)
    eng.close()


# ---------------------------------------------------------------- 3. only the deformed BLAS changes
def test_only_the_deformed_blas_changes():
    sc = DS.base_scene("flat", sizes=(64, 257, 65))
    # apart, so that no TLAS leaf is shared between the deformed mesh and the others
    for k, o in enumerate(sc.objects):
        m = _mat(o.transform).copy()
        m[:3, 3] = (120.0 * (k % 3), 0.0, 40.0 * (k // 3))
        o.transform = tuple(m.T.reshape(-1))
    eng = _engine(sc)
    before = eng.wide_read(0)
    pose = DS.pose_b(sc, stretch=(1.1, 1.2, 0.9))
    eng.set_positions(1, *pose[1])
    eng.commit()
    assert eng.last_deform_stats().instances_rebounded == 2
    after = eng.wide_read(0)
    W.assert_ok(after, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    nt = int(before["tw_tlas_nodes"])
    # instances: the MeshInstances (objects 3..5) come first, then the base meshes; the BLASes' TriRecs
    # lie in mesh order and their nodes follow the TLAS's, each BLAS's in one run from its root
    inst_mesh = {eng.instance_of(j): j % 3 for j in range(6)}
    wr = np.asarray(before["wroot"])
    roots = [int(wr[eng.instance_of(j)]) for j in range(3)]
    assert nt <= roots[0] < roots[1] < roots[2] and all(wr[eng.instance_of(3 + j)] == roots[j] for j in range(3))
    shared = {int(eng.leaf_of[i]) for i, m in inst_mesh.items() if m == 1}
    for inst, mesh in inst_mesh.items():
        assert np.array_equal(before["bcoord"][inst], after["bcoord"][inst]) == (mesh != 1)
        if mesh == 1:
            assert not np.array_equal(before["tbox"][inst], after["tbox"][inst])
            assert not np.array_equal(before["inst_bounds"][inst], after["inst_bounds"][inst])
        elif int(eng.leaf_of[inst]) not in shared:
            assert np.array_equal(before["tbox"][inst], after["tbox"][inst])
            assert np.array_equal(before["inst_bounds"][inst], after["inst_bounds"][inst])
    own = np.zeros(len(before["lbox"]), bool)
    own[64:64 + 257] = True
    assert np.array_equal(before["lbox"][~own], after["lbox"][~own])
    assert not np.array_equal(before["lbox"][own], after["lbox"][own])
    fr = int(before["fit_root"])
    hi = fr if fr >= 0 else int(before["wide_copy"])
    for lo_, hi_, same in ((roots[0], roots[1], True), (roots[1], roots[2], False), (roots[2], hi, True)):
        assert np.array_equal(W.node_multisets(before, lo_, hi_), W.node_multisets(after, lo_, hi_)) == same
    eng.close()


# ---------------------------------------------------------------- 4. round trip; ties
def _tie_scene():
    """test_gpu_rays.test_equal_t_ties_between_transformed_instances' scene (stated inline there):
    two instances of one mesh under the same transform, with different materials - every hit a tie."""
    hp, hf = scenes.heightfield(24, 8.0, 1.0, 3)
    hp32 = hp.astype(np.float32).astype(np.float64)
    a = M.Mesh(id=1, material="1", positions=hp32, indices=hf.astype(np.int32), indices_one_based=False, shading_mode="flat")
    c, sn = np.cos(0.5), np.sin(0.5)
    Mt = np.eye(4)
    Mt[:3, :3] = np.array([[c, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, c]]) * 0.75
    Mt[:3, 3] = (0.25, -0.5, 0.125)
    T = tuple(Mt.T.reshape(-1))
    sc = scenes.scaled(scenes.scene_c1(8, 8), 48, 40)
    sc.materials = [sc.materials[0], dataclasses.replace(sc.materials[0], diffuse=(0.1, 0.9, 0.2))]
    sc.objects = [a, M.MeshInstance(id=5, base_mesh_id=1, material="1", transform=T),
                  M.MeshInstance(id=6, base_mesh_id=1, material="2", transform=T)]
    sc.cameras[0].position = (0.5, 7.0, 7.5)
    sc.cameras[0].gaze_point = (0.0, 0.0, 0.0)
    sc.point_lights[0].position = (1.0, 9.0, 2.0)
    rng = np.random.RandomState(4)
    D = rng.normal(size=(3000, 3)) * np.array([0.4, 1.0, 0.4]) - np.array([0.0, 2.0, 0.0])
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    loc = hp32[rng.randint(len(hp32), size=3000)] + rng.uniform(-0.05, 0.05, size=(3000, 3)) * np.array([1, 0, 1])
    O = loc @ Mt[:3, :3].T + Mt[:3, 3] - 12.0 * D
    return sc, O, D


def _round_trip(eng, pose_b):
    """A -> B -> A on the posed meshes of the engine's scene; returns the read-backs before (the
    baseline: fit_coord compared exactly) and after."""
    pose_a = {i: (np.asarray(eng.scene.objects[i].positions, np.float64).copy(), None) for i in pose_b}
    before = _baseline(eng)
    _stage(eng, pose_b)
    eng.commit()
    mid = eng.wide_read(0)
    assert not np.array_equal(before["lbox"], mid["lbox"])
    _stage(eng, pose_a)
    eng.commit()
    return before, eng.wide_read(0)


@pytest.mark.parametrize("variant", ["flat", "smooth", "supplied_new"])
def test_round_trip_restores_the_build(variant):
    sc = DS.base_scene(variant)
    ref_sc = copy.deepcopy(sc)
    eng = _engine(sc)
    pose = DS.pose_b(sc, with_normals=variant == "supplied_new")
    if variant == "supplied_new":                                   # back to A with A's normals
        back = {i: (np.asarray(sc.objects[i].positions).copy(), np.asarray(sc.objects[i].normals).copy()) for i in pose}
        before = _baseline(eng)
        _stage(eng, pose); eng.commit()
        _stage(eng, back); eng.commit()
        after = eng.wide_read(0)
    else:
        before, after = _round_trip(eng, pose)
    _same_state(before, after)
    W.assert_ok(after, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    O, D, tmax, _ = DS.ray_set()
    rays, frame = _reference(("A", variant), ref_sc, O, D, tmax, None)
    _assert_rays(eng, rays, O, D, tmax)
    _assert_frame_ref(eng, frame)
    eng.close()


@pytest.mark.parametrize("walk", list(WALKS))
def test_round_trip_keeps_equal_t_ties(walk):
    sc, O, D = _tie_scene()
    ref_sc = copy.deepcopy(sc)
    eng = _engine(sc, walk)
    before, after = _round_trip(eng, DS.pose_b(sc))
    _same_state(before, after)
    tmax = np.random.RandomState(8).uniform(5.0, 14.0, size=len(O))
    rays, frame = _reference("ties", ref_sc, O, D, tmax, None)
    assert np.isfinite(rays[0][0]).mean() > 0.3
    _assert_rays(eng, rays, O, D, tmax)
    _assert_frame_ref(eng, frame)
    eng.close()


@pytest.mark.parametrize("walk", list(WALKS))
def test_round_trip_keeps_twin_mesh_and_shared_vertex_ties(walk):
    """test_gpu_rays._twin_meshes: two meshes holding the same triangles (one flat, one with derived
    smooth normals), every hit a tie between two BLASes; plus axis rays exactly through vertices and
    edge midpoints of the grid (ties between the triangles of one BLAS, up to six at a vertex)."""
    sc, hp = _twin_meshes()
    ref_sc = copy.deepcopy(sc)
    rng = np.random.RandomState(4)
    D = rng.normal(size=(3000, 3)) * np.array([0.4, 1.0, 0.4]) - np.array([0.0, 2.0, 0.0])
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    O = rng.uniform(hp.min(0), hp.max(0), size=(3000, 3)) - 12.0 * D
    idx = np.asarray(sc.objects[0].indices).reshape(-1, 3)
    tri = idx[rng.randint(len(idx), size=600)]
    tgt = np.concatenate([hp[tri[:300, 0]], 0.5 * (hp[tri[300:, 0]] + hp[tri[300:, 1]])])
    O = np.concatenate([O, tgt * np.array([1.0, 0.0, 1.0]) + np.array([0.0, 10.0, 0.0])])
    D = np.concatenate([D, np.tile([0.0, -1.0, 0.0], (600, 1))])
    eng = _engine(sc, walk)
    before, after = _round_trip(eng, DS.pose_b(sc))
    _same_state(before, after)
    tmax = np.random.RandomState(8).uniform(5.0, 14.0, size=len(O))
    rays, frame = _reference("twins", ref_sc, O, D, tmax, None)
    assert np.isfinite(rays[0][0][:3000]).mean() > 0.5 and np.isfinite(rays[0][0][3000:]).sum() > 100   # (the reference hits a part of the exact ones)
    _assert_rays(eng, rays, O, D, tmax)
    _assert_frame_ref(eng, frame)
    eng.close()


def test_round_trip_keeps_exactly_touching_rays():
    V, Fc, corners = _touching_grid((1048576.0, -524288.0, 786432.0))
    mesh = M.Mesh(id=1, material="1", positions=V, indices=Fc, indices_one_based=False, shading_mode="flat")
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [mesh]
    sc.cameras[0].position = tuple(corners.mean(0) + np.array([0.0, 0.0, 300.0]))
    sc.cameras[0].gaze_point = tuple(corners.mean(0))
    ref_sc = copy.deepcopy(sc)
    O, D, t0 = _touching_rays(corners, 4.0, np.random.RandomState(5), 3000)
    eng = _engine(sc)
    rng = np.random.RandomState(2)
    before, after = _round_trip(eng, {0: (V * np.array([1.0, 1.5, 1.0]) + rng.normal(scale=0.3, size=V.shape), None)})
    _same_state(before, after)
    tmax = t0 * (1 + 2.0 ** -40)
    rays, _ = _reference("touching", ref_sc, O, D, tmax, None)
    assert (rays[0][0] == t0).mean() > 0.5
    _assert_rays(eng, rays, O, D, tmax)
    eng.close()


# ---------------------------------------------------------------- 5. no accumulation
def test_twenty_small_deformations_equal_one():
    sc = DS.base_scene("smooth", sizes=(3, 65, 257, 1200))
    a, b = _engine(copy.deepcopy(sc)), _engine(copy.deepcopy(sc))
    final = {}
    for i in DS.mesh_indices(sc):
        p = np.asarray(sc.objects[i].positions, np.float64)
        for k in range(20):
            p = DS.small_step(p, k)
        final[i] = p
    for k in range(20):
        for i in DS.mesh_indices(sc):
            a.set_positions(i, DS.small_step(np.asarray(a.scene.objects[i].positions), k))
        a.commit()
    for i, p in final.items():
        assert np.array_equal(a.scene.objects[i].positions, p)
        b.set_positions(i, p)
    b.commit()
    _same_state(a.wide_read(0), b.wide_read(0))
    W.assert_ok(a.wide_read(0), a.scene, after_refit=True, leaf_of=a.leaf_of)
    rgb, rgba, st = a.render_rows(0, 0, 1, True)
    rgb2, rgba2, _ = b.render_rows(0, 0, 1, True)
    assert np.array_equal(rgb, rgb2) and np.array_equal(rgba, rgba2)
    _assert_frame(a, rgb, rgba, st)
    a.close(); b.close()


# ---------------------------------------------------------------- 6. frames through the full passes
_c2_like, _wobble = DS.c2_like, DS.wobble


@pytest.mark.parametrize("dielectric", [False, True])
def test_frames_of_a_deformed_mirror_mesh(dielectric):
    sc = _c2_like(dielectric)
    eng = _engine(sc, devices=[0, 0])
    eng.set_positions(0, _wobble(np.asarray(sc.objects[0].positions)))
    eng.commit()
    ref = oracle.OracleScene(eng.scene).render(0, threads=0, rgba=True)
    assert ref[2].secondary_rays > 0 and ref[2].shadow_rays > 0
    _assert_frame_ref(eng, ref)                                     # render_rows over two replicas
    rgb, rgba = eng.alloc_frame(0)
    st = eng.wait(eng.submit_into(0, 0, 1, rgb, rgba))
    assert float(np.abs(rgb - ref[0]).max()) <= 1e-5 and np.array_equal(rgba, ref[1])
    assert (st.primary_rays, st.shadow_rays, st.secondary_rays) == (ref[2].primary_rays, ref[2].shadow_rays,
                                                                    ref[2].secondary_rays)
    eng.close()


# ---------------------------------------------------------------- 7. deformation and motion in one commit
@pytest.mark.parametrize("walk", ["transformed", "transformed_binary"])
def test_deformation_and_motion_in_one_commit(walk):
    sc, pose, moves = DS.combined_case()
    eng = _engine(sc, walk)
    _stage(eng, pose)                                               # mesh 102 (257 triangles); its MeshInstance
    for obj, m in moves.items():                                    # moves too, and so does an instance of a
        eng.set_transform(obj, m)                                   # mesh that keeps its shape
    st = eng.commit()
    ds = eng.last_deform_stats()
    assert st.instances_moved == 2
    assert (ds.meshes_deformed, ds.triangles, ds.instances_rebounded) == (1, 257, 2)
    O, D, tmax, _ = DS.aimed_ray_set(eng.scene)
    osc = oracle.OracleScene(eng.scene)
    ref = (osc.trace_rays(O, D), osc.occluded_rays(O, D, tmax))
    osc.close()
    assert np.isfinite(ref[0][0]).sum() > 600
    _assert_rays(eng, ref, O, D, tmax)
    if walk == "transformed":
        W.assert_ok(eng.wide_read(0), eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    eng.close()


# ---------------------------------------------------------------- 8. coordinates grow
def test_coordinates_grow_and_bcoord_follows():
    """Two meshes and their instances grown from |coordinate| about 10 to 2.6e6 (vertices times
    2^18).  The verifier passes and fails on a stale bcoord.  The near-vertex rays of
    tests/test_gpu_refit_edges.py (test_gpu_wide_bound._near_vertex_rays: aimed a hair from, and
    exactly at, vertices and edges) are bit-equal to the oracle at the production widening, through
    the fit tree and through tw_walk.  Those rays tie between the triangles of one BLAS; a growth
    by a power of two is exact in every step of the builder (bounds, centroids, bin indices; SAH
    costs scale by 2^36), so the fresh build's BLAS topology is the kept one and so is the tie order.
    The same rays with wide_delta_scale = round(1000 * old bcoord / new bcoord), the widening a
    stale bcoord would apply (2^-18 of the bound: the option's 0), mismatch.  Measured on an MI355X,
    (closest hits, occlusion results) of the 6000 rays: fit (236, 112), tw (235, 110); none at the
    production widening."""
    sc, s = DS.grown_case(grown=False)
    eng = _engine(sc)
    old = eng.wide_read(0)
    for i in DS.mesh_indices(sc):
        eng.set_positions(i, np.asarray(sc.objects[i].positions) * s)
    eng.commit()
    new = eng.wide_read(0)
    assert np.array_equal(new["bcoord"], old["bcoord"] * s) and new["wide_coord"] > 1e6
    W.assert_ok(new, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    stale = dict(new)
    stale["bcoord"] = old["bcoord"]
    assert not W.verify(stale, eng.scene, after_refit=True, leaf_of=eng.leaf_of).ok(), "the verifier must see a stale bcoord"
    O, D, tmax, _ = DS.aimed_ray_set(eng.scene, 1500, seed=4, radius=12.0 * s)   # interior points: tie-free
    ref = _ref(eng.scene, O, D, tmax * s)
    assert np.isfinite(ref[0][0]).sum() > 1000
    _assert_rays(eng, ref, O, D, tmax * s)
    # near-vertex rays, per mesh object in its world place
    rng = np.random.RandomState(61)
    parts = []
    for i in range(len(eng.scene.objects)):
        base = eng.scene.objects[i if i < 2 else i - 2]
        t = _mat(eng.scene.objects[i].transform)[:3, 3]
        parts.append(_near_vertex_rays(np.asarray(base.positions) + t, np.asarray(base.indices).reshape(-1, 3), 1500, rng, 4.0 * s))
    O, D = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    hits = _ref(eng.scene, O, D, np.full(len(O), 1.0e12))[0][0]
    assert np.isfinite(hits).mean() > 0.3
    tmax = _tmax(hits, np.random.RandomState(3), 1.0e9)
    ref = _ref(eng.scene, O, D, tmax)

    def counts():
        out = {}
        for fit in (1, 0):
            eng.set_option("fit", fit)
            out[fit] = _mismatches(eng, ref, O, D, tmax)
        eng.set_option("fit", 1)
        return out
    good = counts()
    assert good == {1: (0, 0), 0: (0, 0)}, f"mismatches at the production widening: {good}"
    permille = int(round(1000.0 * float(old["bcoord"].max()) / float(new["bcoord"].max())))
    assert permille == 0
    eng.set_unsafe_option("wide_delta_scale", permille)
    bare = counts()
    print(f"grown by 2^18, wide_delta_scale {permille}: fit {bare[1]}, tw {bare[0]} (closest, occlusion) of {len(O)}")
    assert bare[1][0] + bare[1][1] >= 1 and bare[0][0] + bare[0][1] >= 1, bare    # the set reaches the bound
    eng.close()


# ---------------------------------------------------------------- 9. degenerate
@pytest.mark.parametrize("kind", ["point", "zero_area"])
def test_degenerate_deformations(kind):
    sc = DS.base_scene("flat", sizes=(3, 65, 257))
    ref_sc = copy.deepcopy(sc)
    eng = _engine(sc)
    before = _baseline(eng)
    p = np.asarray(sc.objects[2].positions, np.float64).copy()
    q = DS.degenerate_pose(sc.objects[2], kind)
    eng.set_positions(2, q)
    eng.commit()
    d = eng.wide_read(0)
    assert np.isfinite(d["lbox"]).all() and np.isfinite(d["tbox"]).all() and np.isfinite(d["bcoord"]).all()
    near, _, far, _ = W.split_nodes(d["nodes"])
    assert not np.isnan(near).any() and not np.isnan(far).any()
    W.assert_ok(d, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    O, D, tmax, _ = DS.aimed_ray_set(ref_sc, 1000, seed=11)
    osc = oracle.OracleScene(eng.scene)
    ref = (osc.trace_rays(O, D), osc.occluded_rays(O, D, tmax))
    frame = osc.render(0, threads=0, rgba=True)
    osc.close()
    _assert_rays(eng, ref, O, D, tmax)
    _assert_frame_ref(eng, frame)
    eng.set_positions(2, p)
    eng.commit()
    _same_state(before, eng.wide_read(0))
    rays, frame = _reference(("A3", "flat"), ref_sc, O, D, tmax, None)
    _assert_rays(eng, rays, O, D, tmax)
    _assert_frame_ref(eng, frame)
    eng.close()


# ---------------------------------------------------------------- 10. device path
def test_positions_from_a_device_tensor():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    sc = DS.base_scene("smooth", sizes=(3, 65, 257, 1200))
    a, b = _engine(copy.deepcopy(sc)), _engine(copy.deepcopy(sc))
    keep = []
    for i in DS.mesh_indices(sc):
        t = torch.from_numpy(np.asarray(sc.objects[i].positions, np.float64)).to("cuda:0")
        t = (t * torch.tensor([1.3, 0.7, 1.9], dtype=torch.float64, device="cuda:0") + 0.05 * torch.sin(3.0 * t)).contiguous()
        keep.append(t)
        a.set_positions(i, t)
        b.set_positions(i, t.cpu().numpy())
    torch.cuda.synchronize()
    a.commit(); b.commit()
    _same_state(a.wide_read(0), b.wide_read(0))
    assert np.array_equal(a.wide_read(0)["nodes"], b.wide_read(0)["nodes"])
    for i in DS.mesh_indices(sc):
        assert np.array_equal(a.scene.objects[i].positions, b.scene.objects[i].positions)
    O, D, tmax, _ = DS.ray_set(1000, seed=12)
    osc = oracle.OracleScene(a.scene)
    ref = (osc.trace_rays(O, D), osc.occluded_rays(O, D, tmax))
    osc.close()
    _assert_rays(a, ref, O, D, tmax)
    rgb, rgba, st = a.render_rows(0, 0, 1, True)
    _assert_frame(a, rgb, rgba, st)
    host = torch.zeros((len(sc.objects[0].positions), 3), dtype=torch.float64)
    lib = M.load_library()
    assert lib.rt_scene_set_mesh_positions(a.handle, 0, host.data_ptr(), host.shape[0], None,
                                           A.RT_POSITIONS_DEVICE) == A.RT_ERR_UNSUPPORTED
    a.close(); b.close()


# ---------------------------------------------------------------- 11. contract
def test_contract_arguments():
    sc = DS.base_scene("flat", sizes=(3, 65))
    sc.objects.append(M.Mesh(id=300, material="1", positions=np.zeros((3, 3)), indices=np.zeros((0, 3), np.int32),
                             indices_one_based=False))
    sc.objects.append(M.Sphere(center=(0.0, 50.0, 0.0), radius=1.0, material="1"))
    p = np.asarray(sc.objects[0].positions)
    for kw in (dict(deformable=False, dynamic=True), dict(deformable=False)):
        eng = _engine(copy.deepcopy(sc), **kw)
        with pytest.raises(M.RenderError) as e:
            eng.set_positions(0, p, mirror=False)
        assert e.value.code == A.RT_ERR_UNSUPPORTED
        eng.close()
    eng = _engine(sc)
    for obj, pos, nrm in ((2, p, None),                             # a MeshInstance
                          (5, np.zeros((1, 3)), None),              # a sphere
                          (4, np.zeros((3, 3)), None),              # a mesh without triangles
                          (0, p[:-1], None),                        # wrong count
                          (0, p, np.ones_like(p)),                  # normals for a mesh that derives them
                          (99, p, None)):
        with pytest.raises(M.RenderError) as e:
            eng.set_positions(obj, pos, nrm, mirror=False)
        assert e.value.code == A.RT_ERR_INVALID_ARG, obj
    with pytest.raises(M.RenderError) as e:
        eng.vertex_count(2)
    assert e.value.code == A.RT_ERR_INVALID_ARG
    assert eng.commit().instances_moved == 0 and eng.last_deform_stats().meshes_deformed == 0
    eng.close()


@pytest.mark.parametrize("bad", ["nan_unreferenced", "nan", "huge"])
def test_commit_refuses_bad_positions_and_changes_nothing(bad):
    sc = DS.base_scene("flat", sizes=(3, 65))
    eng = _engine(sc)
    before = eng.wide_read(0)
    O, D, tmax, _ = DS.ray_set(10)
    _, frame = _reference(("A2", "flat"), copy.deepcopy(sc), O, D, tmax, None)
    p = np.asarray(sc.objects[1].positions, np.float64).copy()
    used = np.unique(np.asarray(sc.objects[1].indices))
    if bad == "nan_unreferenced":
        p[np.setdiff1d(np.arange(len(p)), used)[0], 1] = np.nan
    elif bad == "nan":
        p[used[3], 2] = np.nan
    else:
        p[used[0], 0] = 1e31
    good = DS.pose_b(sc)
    eng.set_positions(0, *good[0], mirror=False)                    # dropped with the bad one
    eng.set_positions(1, p, mirror=False)
    eng.set_transform(2, sc.objects[2].transform)
    with pytest.raises(M.RenderError) as e:
        eng.commit()
    assert e.value.code == A.RT_ERR_INVALID_ARG
    assert W.same_dump(before, eng.wide_read(0)) is None
    _assert_frame_ref(eng, frame)
    st = eng.commit()                                               # nothing is staged any more
    assert st.instances_moved == 0 and eng.last_deform_stats().meshes_deformed == 0
    assert W.same_dump(before, eng.wide_read(0)) is None
    eng.close()


def test_staging_in_flight_and_busy_commit():
    sc = DS.base_scene("flat", sizes=(65, 257))
    eng = _engine(sc)
    old = oracle.OracleScene(copy.deepcopy(eng.scene)).render(0, threads=0, rgba=True)
    rgb, rgba = eng.alloc_frame(0)
    ticket = eng.submit_into(0, 0, 1, rgb, rgba)
    _stage(eng, DS.pose_b(sc))                                      # accepted while the render is in flight
    with pytest.raises(M.RenderError) as e:
        eng.commit()
    assert e.value.code == A.RT_ERR_BUSY
    eng.wait(ticket)
    assert float(np.abs(rgb - old[0]).max()) <= 1e-5 and np.array_equal(rgba, old[1])   # the old pose
    eng.commit()                                                    # the staged positions survived the refusal
    assert eng.last_deform_stats().meshes_deformed == 2
    r2, a2, st = eng.render_rows(0, 0, 1, True)
    _assert_frame(eng, r2, a2, st)
    assert not np.array_equal(r2, old[0])
    eng.close()


def test_a_ply_backed_mesh_becomes_inline_in_the_mirror(tmp_path):
    """set_positions on a PLY-backed mesh (with PLY normals): the mirror takes the PLY's faces and
    normals through ply_load and the new positions, and stays the oracle's scene."""
    sc, pose = DS.ply_case(str(tmp_path))
    eng = M.RayTracerEngine(sc, deformable=True)
    # (the oracle reads inline meshes: the TLAS leaves of the same scene before its mesh went to the PLY)
    eng.leaf_of = W.tlas_leaves(DS.base_scene("flat", sizes=(65, 257)))
    assert eng.vertex_count(1) == len(pose[1][0])
    _stage(eng, pose)
    o = eng.scene.objects[1]
    assert o.ply_path is None and not o.indices_one_based and np.asarray(o.indices).shape == (257, 3)
    assert np.array_equal(o.positions, pose[1][0]) and np.asarray(o.normals).shape == np.asarray(o.positions).shape
    eng.commit()
    assert eng.last_deform_stats().meshes_deformed == 2
    O, D, tmax, _ = DS.aimed_ray_set(eng.scene, 1000, seed=14)
    ref = _ref(eng.scene, O, D, tmax)
    assert np.isfinite(ref[0][0]).sum() > 500
    _assert_rays(eng, ref, O, D, tmax)
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)
    _assert_frame(eng, rgb, rgba, st)
    W.assert_ok(eng.wide_read(0), eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    eng.close()


def _inexact(sc):
    """The same scene with one referenced vertex coordinate that is no float: no CTri, no CRec."""
    out = copy.deepcopy(sc)
    for i in DS.mesh_indices(out):
        p = np.asarray(out.objects[i].positions, np.float64).copy()
        v = int(np.asarray(out.objects[i].indices).reshape(-1)[0])
        p[v, 0] *= 1.0 + 2.0 ** -40
        assert np.float64(np.float32(p[v, 0])) != p[v, 0]
        out.objects[i].positions = p
    return out


def test_compact_layouts_stay_in_use_without_the_flag():
    """device_bytes of a scene with float-exact vertices against the same scene with one inexact
    vertex per mesh: a static scene holds CTri (48 B per triangle) and CRec (64 B per BLAS record)
    more, a dynamic one CRec more (its CTri replace the 48-B triangle boxes), a deformable one
    nothing: it never uses them.  (An empty array is uploaded as one element.)"""
    sc = DS.base_scene("flat", sizes=(65, 257))
    got = {}
    for name, kw in (("static", dict(deformable=False)), ("dynamic", dict(deformable=False, dynamic=True)),
                     ("deformable", dict())):
        a, b = _engine(copy.deepcopy(sc), **kw), _engine(_inexact(sc), **kw)
        ia, ib = a.info(), b.info()
        assert (ia.triangles, ia.blas_nodes) == (ib.triangles, ib.blas_nodes) == (65 + 257, ia.blas_nodes)
        got[name] = (int(ia.device_bytes - ib.device_bytes), int(ia.triangles), int(ia.blas_nodes))
        a.close(); b.close()
    n, r = got["static"][1], got["static"][2]
    assert got["static"][0] == 48 * n + 64 * (r - 1)
    assert got["dynamic"][0] == 64 * (r - 1)
    assert got["deformable"][0] == 0


@pytest.mark.parametrize("dynamic", [False, True])
def test_scenes_without_the_flag_are_unchanged(dynamic):
    """One frame each against the oracle, and the deformable scene at rest renders the same."""
    sc = DS.base_scene("flat", sizes=(65, 257))
    eng = _engine(copy.deepcopy(sc), deformable=False, dynamic=dynamic)
    dfm = _engine(copy.deepcopy(sc))
    with pytest.raises(M.RenderError) as e:
        eng.vertex_count(0)
    assert e.value.code == A.RT_ERR_UNSUPPORTED
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)
    _assert_frame(eng, rgb, rgba, st)
    r2, a2, _ = dfm.render_rows(0, 0, 1, True)                      # at rest the deformable scene renders the same
    assert np.array_equal(rgba, a2) and float(np.abs(rgb - r2).max()) <= 1e-5
    eng.close(); dfm.close()
