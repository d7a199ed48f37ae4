"""rt_scene_commit at its edges, checked on the trees themselves and on hits.

tests/test_gpu_refit.py compares hits after a commit with the oracle, on scenes where the constants
the commit re-derives (scene.cpp refit_host_scene: wide_coord, fit_coord, prune_k, det_scale, the
scene centre and extent, the kFitKappa block) hardly matter.  Here the four-wide nodes the device
refit (refit.h k_refit_level, k_octant_copies) are read back with rt_debug_wide_read and checked
slot by slot by tests/wide_tree_check.py against an FP64 restatement - exactly, no tolerance - and
the hits are taken where those constants decide: poses at 1e6, a camera at 1e6, transforms across
forty binades, instances over kFitKappa, instances stacked at one pose.  Every comparison is exact
(array_equal / bit equality) but the frame criteria of test_gpu_refit._assert_frame."""
import dataclasses
import os
import sys

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import engine, scenes
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_tree_check as W                                                      # noqa: E402
from test_fit_coincident import _stacked                                        # noqa: E402
from test_gpu_rays import _grazing_set                                          # noqa: E402
from test_gpu_refit import (WALKS, _assert_frame, _assert_rays, _engine as _refit_engine, _m16, _mat, _pose_b, _ray_set,   # noqa: E402
                            _rotation, _transformed_instances)
from test_gpu_wide_bound import _near_vertex_rays, _touching_grid, _touching_rays   # noqa: E402
from test_wide_build import kappa_pose, m16, posed, small_scene                            # noqa: E402

pytestmark = pytest.mark.gpu


def _engine(sc, walk="transformed", devices=None):
    """A dynamic engine that remembers the TLAS leaves of the scene as built (the oracle's): a refit
    keeps that topology, so tbox is checked against those leaves after every commit."""
    leaf_of = W.tlas_leaves(sc)
    eng = _refit_engine(sc, walk, True, devices)
    eng.leaf_of = leaf_of
    return eng


def _ref(sc, O, D, tmax):
    """The oracle's closest hits and occlusion for the scene as it stands."""
    osc = oracle.OracleScene(sc)
    r = (osc.trace_rays(O, D), osc.occluded_rays(O, D, tmax))
    osc.close()
    return r


def _mismatches(eng, ref, O, D, tmax):
    """(closest hits, occlusion results) that differ from the oracle's, bit for bit."""
    (to, po, no, mo), oo = ref
    tg, pg, ng, mg = eng.trace_rays(O, D)
    bad = (tg.view(np.uint64) != to.view(np.uint64)) | (mg != mo)
    hit = np.isfinite(to) & np.isfinite(tg)
    bad |= hit & ((pg != po).any(1) | (ng != no).any(1))
    return int(bad.sum()), int((eng.occluded_rays(O, D, tmax) != oo).sum())


def _set_walk(eng, walk):
    for k in ("fit", "wide", "unified_transformed"):
        eng.set_option(k, 1)
    for k, v in WALKS[walk].items():
        eng.set_option(k, v)


def _tmax(ref, rng, miss):
    t = ref[0] if isinstance(ref, tuple) else ref
    return np.where(np.isfinite(t), t * (1 + rng.choice([-1e-9, 1e-9], size=len(t))), miss)


def _kappa_pose():
    return kappa_pose()                                                    # diag(1, 1, 2^-13): over kFitKappa


# ---------------------------------------------------------------- 1. device equals host
@pytest.mark.parametrize("name", ["posed", "stacked9", "kappa"])
def test_device_read_back_equals_the_host_build(name):
    sc = {"posed": lambda: small_scene([posed(0), posed(1), posed(2)]), "stacked9": lambda: _stacked(9),
          "kappa": lambda: small_scene([posed(0), _kappa_pose()])}[name]()
    host = engine.wide_build(sc, dynamic=True)
    eng = _engine(sc)
    dev = eng.wide_read()
    assert host["wide_root"] >= 0 and (host["fit_root"] >= 0) == (name != "kappa")
    assert W.same_dump(host, dev) is None, f"device and host differ in {W.same_dump(host, dev)}"
    W.assert_ok(dev, sc)
    if name == "posed":                                          # refused while a render is in flight
        rgb = M.pinned_array((8, 8, 3), np.float64)
        ticket = eng.submit_into(0, 0, 1, rgb, None)
        with pytest.raises(M.RenderError) as e:
            eng.wide_read()
        assert e.value.code == A.RT_ERR_BUSY
        eng.wait(ticket)
        assert W.same_dump(host, eng.wide_read()) is None
    eng.close()


# ---------------------------------------------------------------- 2. refit structure
def _small_transformed():
    """test_gpu_refit._transformed_instances (its poses, so _pose_b applies) over C2's geometry at
    48 x 26 segments: 2.4k triangles."""
    sc = _transformed_instances()
    pos, faces = scenes.geometry_c2(48, 26)
    sc.objects[0].positions = pos.astype(np.float32).astype(np.float64)
    sc.objects[0].indices = faces.astype(np.int32)
    return sc


def test_refit_structure_two_replicas_and_back():
    sc = _small_transformed()
    pose_a = {i: tuple(sc.objects[i].transform) for i in (2, 4, 5)}
    eng = _engine(sc, devices=[0, 0])
    built = eng.wide_read(0)
    W.assert_ok(built, eng.scene)
    for i, m in _pose_b(sc).items():
        eng.set_transform(i, m)
    assert eng.commit().instances_moved == 3
    d0, d1 = eng.wide_read(0), eng.wide_read(1)
    assert W.same_dump(d0, d1) is None, f"the replicas differ in {W.same_dump(d0, d1)}"
    W.assert_ok(d0, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    assert not np.array_equal(built["nodes"], d0["nodes"])       # the commit did change the trees
    # back to pose A: per node the same (ref, box) multisets as the build's, fit tree and TLAS part
    for i, m in pose_a.items():
        eng.set_transform(i, m)
    eng.commit()
    back = eng.wide_read(0)
    W.assert_ok(back, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    fr, fn, nt = int(built["fit_root"]), int(built["fit_nodes"]), int(built["tw_tlas_nodes"])
    assert fr >= 0 and nt > 1
    for lo, hi in ((fr, fr + fn), (0, nt)):
        assert np.array_equal(W.node_multisets(back, lo, hi), W.node_multisets(built, lo, hi))
    # (slot order among equal keys may differ between the host's sort and the device's: not asserted)
    print("nodes byte-equal after the return to pose A:", np.array_equal(back["nodes"], built["nodes"]))
    for k in ("lbox", "fpairs", "tbox", "inst_bounds", "l2w"):
        assert np.array_equal(back[k], built[k]), k
    assert (back["wide_coord"], back["fit_blocked"]) == (built["wide_coord"], 0) and back["fit_coord"] >= built["fit_coord"]
    # twenty commits of small random moves: nothing accumulates
    rng = np.random.RandomState(4)
    for step in range(20):
        for i in range(1, 6):
            m = _mat(eng.scene.objects[i].transform).copy()
            m[:3, :3] = (np.eye(3) + rng.normal(scale=0.02, size=(3, 3))) @ m[:3, :3]
            m[:3, 3] += rng.normal(scale=0.1, size=3)
            eng.set_transform(i, tuple(m.T.reshape(-1)))
        eng.commit()
    d0, d1 = eng.wide_read(0), eng.wide_read(1)
    assert W.same_dump(d0, d1) is None
    W.assert_ok(d0, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    eng.close()


# ---------------------------------------------------------------- 3. level and block edges
_COUNTS = (2, 3, 4, 5, 64, 65, 257)
_LEVELS = {}


def _spread(k, seed=0):
    """Instance k's pose: distinct lattice cell, rotated, scaled 0.2 .. 0.5."""
    rng = np.random.RandomState(1000 * seed + k)
    cell = np.array([k % 7, (k // 7) % 7, k // 49], np.float64) * 1.7 - 5.0
    return _m16(_rotation(rng) * rng.uniform(0.2, 0.5), cell + rng.uniform(-0.3, 0.3, size=3))


def _aimed_rays(sc, limit, seed):
    """Rays at the world image of the first triangle's centroid of up to `limit` instances."""
    mesh = sc.objects[0]
    c = np.asarray(mesh.positions)[np.asarray(mesh.indices)[0]].mean(axis=0)
    rng = np.random.RandomState(seed)
    objs = sc.objects[:limit]
    tgt = np.repeat(np.array([_mat(o.transform)[:3, :3] @ c + _mat(o.transform)[:3, 3] for o in objs]), 3, axis=0)
    d = rng.normal(size=tgt.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return tgt - d * rng.uniform(0.05, 0.3, size=(len(tgt), 1)), d


def _count_rays(sc, seed):
    """Random and axis-parallel rays through the lattice, then (last) rays aimed at the instances."""
    O, D = _ray_set(np.array([0.0, 0.0, 0.0]), 6.0, 1200, seed)
    Oa, Da = _aimed_rays(sc, 100, seed + 1)
    return np.concatenate([O, Oa]), np.concatenate([D, Da]), len(Oa)


def _count_scene(count, mesh):
    n, faces = (6, 2) if mesh == "two_triangles" else (8, None)
    return small_scene([_spread(k) for k in range(count - 1)], n=n, faces=faces, base_at=(0.0, 6.0, 0.0))


@pytest.mark.parametrize("mesh", ["two_triangles", "sixty_four_runs"])
@pytest.mark.parametrize("count", _COUNTS)
def test_level_and_block_edges(count, mesh):
    """k_refit_level runs 4 * (nodes of a level) threads in blocks of 256 and k_octant_copies one
    thread per node: instance counts 2 .. 257 of a 2-triangle mesh and of a mesh of 64 leaf runs put
    levels below, at and above one block (test_levels_lie_on_both_sides_of_a_block).  The trees
    and a ray set are checked before and after a commit that moves every instance."""
    sc = _count_scene(count, mesh)
    eng = _engine(sc)
    O, D, aimed = _count_rays(eng.scene, 7 + count)
    tmax = np.random.RandomState(count).uniform(0.1, 20.0, size=len(O))
    rep = W.assert_ok(eng.wide_read(), eng.scene)
    _LEVELS[(count, mesh)] = rep.trees["tlas"]["levels"] + rep.trees.get("fit", {}).get("levels", [])
    ref = _ref(eng.scene, O, D, tmax)
    assert np.isfinite(ref[0][0][-aimed:]).mean() > 0.5, "the aimed rays must hit"
    _assert_rays(eng, ref, O, D, tmax)
    for k in range(count - 1):
        eng.set_transform(1 + k, _spread(k, seed=1))
    eng.set_transform(0, M.translation(1.0, -6.0, 0.5))
    assert eng.commit().instances_moved == count
    W.assert_ok(eng.wide_read(), eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    O, D, aimed = _count_rays(eng.scene, 9 + count)
    ref = _ref(eng.scene, O, D, tmax)
    assert np.isfinite(ref[0][0][-aimed:]).mean() > 0.5
    _assert_rays(eng, ref, O, D, tmax)
    eng.close()


def test_levels_lie_on_both_sides_of_a_block():
    """From the level sizes the verifier reconstructs (host builds: the device's equal them,
    test_device_read_back_equals_the_host_build): some level has 4 * nodes below 256 threads, one
    exactly 256, one above 256 that is no multiple of 256, one above two blocks."""
    sizes = set()
    for mesh in ("two_triangles", "sixty_four_runs"):
        for count in _COUNTS:
            if (count, mesh) not in _LEVELS:
                sc = _count_scene(count, mesh)
                rep = W.assert_ok(engine.wide_build(sc, dynamic=True), sc)
                _LEVELS[(count, mesh)] = rep.trees["tlas"]["levels"] + rep.trees.get("fit", {}).get("levels", [])
            sizes |= set(_LEVELS[(count, mesh)])
    print("level sizes:", sorted(sizes))
    assert any(4 * s < 256 for s in sizes) and any(4 * s == 256 for s in sizes)
    assert any(4 * s > 256 and (4 * s) % 256 for s in sizes) and any(4 * s > 512 for s in sizes)
    assert any(s > 256 and s % 256 for s in sizes)               # k_octant_copies: nodes per thread block


# ---------------------------------------------------------------- 4. stacked start
@pytest.mark.parametrize("n", [5, 9])
def test_stacked_start_then_moved_apart(n):
    sc = _stacked(n)
    sc = scenes.scaled(sc, 24, 16)
    sc.cameras[0].position = (0.5, 9.0, 4.0)
    sc.cameras[0].gaze_point = (0.5, -0.25, 1.0)
    eng = _engine(sc)
    O, D = _ray_set(np.array([0.5, -0.25, 1.0]), 4.0, 1500, 40 + n)
    tmax = np.random.RandomState(n).uniform(0.1, 12.0, size=len(O))
    ref = _ref(eng.scene, O, D, tmax)
    assert np.isfinite(ref[0][0]).mean() > 0.1
    for walk in WALKS:
        _set_walk(eng, walk)
        _assert_rays(eng, ref, O, D, tmax)
    _set_walk(eng, "transformed")
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)
    assert st.rewalked > 0, "every hit of the stack is a tie between instances"
    _assert_frame(eng, rgb, rgba, st)
    rng = np.random.RandomState(50 + n)
    for k in range(n):
        eng.set_transform(1 + k, _m16(_rotation(rng) * (1.0 + 0.1 * k), (2.5 * (k % 3) - 2.0, 0.6 * k - 2.0, 2.5 * (k // 3))))
    assert eng.commit().instances_moved == n
    W.assert_ok(eng.wide_read(), eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    ref = _ref(eng.scene, O, D, tmax)
    assert np.isfinite(ref[0][0]).mean() > 0.1
    for walk in WALKS:
        _set_walk(eng, walk)
        _assert_rays(eng, ref, O, D, tmax)
    _set_walk(eng, "transformed")
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)
    _assert_frame(eng, rgb, rgba, st)
    eng.close()


# ---------------------------------------------------------------- 5. teeth after a commit
_FAR = (1.0e6, 1.0e6, 1.0e6)


def _teeth_scene(instance_at, w=8, h=8):
    """A 48 x 26 sphere of radius 1e4 snapped to multiples of 2^-4 - so a translation to 1e6 is
    exact, as in test_gpu_wide_bound.test_fit_tree_reaches_the_bound - as one translated instance
    (object 1) plus its base mesh 3e4 away along -x: built near the origin no coordinate exceeds 5e4."""
    pos, faces = scenes.uv_sphere(48, 26)
    P = np.round(pos * 1.0e4 * 16.0) / 16.0
    assert np.array_equal(P.astype(np.float32).astype(np.float64), P)
    mesh = M.Mesh(id=1, material="1", positions=P, indices=faces.astype(np.int32), indices_one_based=False,
                  shading_mode="flat", transform=M.translation(-3.0e4, 0.0, 0.0))
    sc = scenes.scaled(scenes.scene_c2(inline=True), w, h)
    sc.objects = [mesh, M.MeshInstance(id=2, base_mesh_id=1, material="1", transform=M.translation(*instance_at))]
    sc.shadow_ray_epsilon *= 1.0e4
    sc.cameras[0].position = tuple(np.asarray(instance_at) + np.array([0.0, 6.0e3, 4.2e4]))
    sc.cameras[0].gaze_point = tuple(np.asarray(instance_at))
    for L in sc.point_lights:
        L.position = tuple(np.asarray(L.position) * 1.0e4 + np.asarray(instance_at))
        L.intensity = tuple(np.asarray(L.intensity) * 1.0e8)
    return sc, P, faces


def _teeth_counts(eng, sc_now, O, D):
    """Mismatches (closest, occlusion) against the oracle at fit 1 and 0."""
    ref_t = _ref(sc_now, O, D, np.full(len(O), 1.0e9))
    assert np.isfinite(ref_t[0][0]).mean() > 0.3
    tmax = _tmax(ref_t[0][0], np.random.RandomState(3), 1.0e7)
    ref = _ref(sc_now, O, D, tmax)
    out = {}
    for fit in (1, 0):
        eng.set_option("fit", fit)
        out[fit] = _mismatches(eng, ref, O, D, tmax)
    eng.set_option("fit", 1)
    return out


def test_teeth_after_a_commit_to_1e6():
    """Built near the origin (wide_coord and fit_coord ~ 4e4), the instance committed to (1e6, 1e6,
    1e6): the near-vertex rays at its new place are bit-equal to the oracle at the production
    widening through the fit tree and through tw_walk, and differ with wide_delta_scale = 0 - so the
    set reaches the bound rt_scene_commit had to re-derive (a stale wide_coord / fit_coord of 4e4
    would widen 25 times too little).  The other direction, built at 1e6 and committed back to the
    origin, stays exact.
    Measured on an MI355X, mismatching (closest hits, occlusion results) of the 8000 rays:
      wide_delta_scale    0: fit (742, 350), tw (167, 89)
      wide_delta_scale   40: fit (327, 144), tw (18, 8)    - 40/1000 = 4e4 / 1e6 is the widening a
                             commit that kept the build's wide_coord / fit_coord would apply, so
                             that error would show here; asserted below
      wide_delta_scale  100: fit (52, 27),   tw (0, 0);   200, 500, 1000: none."""
    sc, P, F = _teeth_scene((16.0, 0.0, 0.0))
    eng = _engine(sc)
    before = eng.wide_read()
    assert before["wide_coord"] < 5.0e4 and before["fit_coord"] < 5.0e4
    eng.set_transform(1, M.translation(*_FAR))
    assert eng.commit().instances_moved == 1
    d = eng.wide_read()
    W.assert_ok(d, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    assert d["wide_coord"] >= 1.0e6 and d["fit_coord"] >= 1.0e6
    rng = np.random.RandomState(61)
    O, D = _near_vertex_rays(P + np.asarray(_FAR), F, 8000, rng, 3.0e4)
    good = _teeth_counts(eng, eng.scene, O, D)
    assert good == {1: (0, 0), 0: (0, 0)}, f"mismatches at the production widening: {good}"
    eng.set_unsafe_option("wide_delta_scale", 0)
    bare = _teeth_counts(eng, eng.scene, O, D)
    print(f"commit to 1e6, no widening: fit {bare[1]}, tw {bare[0]} (closest, occlusion) of {len(O)}")
    assert bare[1][0] + bare[1][1] >= 1 and bare[0][0] + bare[0][1] >= 1, bare
    eng.set_unsafe_option("wide_delta_scale", 40)                # the widening of a stale 4e4 bound
    stale = _teeth_counts(eng, eng.scene, O, D)
    print(f"commit to 1e6, 40/1000 of the widening: fit {stale[1]}, tw {stale[0]}")
    assert stale[1][0] + stale[1][1] >= 1 and stale[0][0] + stale[0][1] >= 1, stale
    eng.close()
    # built far away, committed back
    sc, P, F = _teeth_scene(_FAR)
    eng = _engine(sc)
    eng.set_transform(1, M.translation(16.0, 0.0, 0.0))
    eng.commit()
    d = eng.wide_read()
    W.assert_ok(d, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    assert d["wide_coord"] < 5.0e4 and d["fit_coord"] < 5.0e4, "the bounds follow the pose down again"
    O, D = _near_vertex_rays(P + np.array([16.0, 0.0, 0.0]), F, 8000, np.random.RandomState(62), 3.0e4)
    good = _teeth_counts(eng, eng.scene, O, D)
    assert good == {1: (0, 0), 0: (0, 0)}, good
    eng.close()


_DYADIC = (1048576.0, -524288.0, 786432.0)


def _touching_scene(instance_at):
    """test_gpu_wide_bound's grid of flat right triangles in local coordinates 0 .. 136 (integers, so
    any dyadic translation is exact) as one translated instance (object 1); its base mesh sits 1000
    away along -x."""
    V, Fc, corners = _touching_grid((0.0, 0.0, 0.0))
    mesh = M.Mesh(id=1, material="1", positions=V, indices=Fc, indices_one_based=False, shading_mode="flat",
                  transform=M.translation(-1000.0, 0.0, 0.0))
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [mesh, M.MeshInstance(id=2, base_mesh_id=1, material="1", transform=M.translation(*instance_at))]
    return sc, corners


def _touching_counts(eng, corners_world, seed):
    """(closest, occlusion) mismatches of the exactly touching rays at fit 1 and 0."""
    O, D, t0 = _touching_rays(corners_world, 4.0, np.random.RandomState(seed), 6000)
    tmax = t0 * (1 + 2.0 ** -40)
    ref = _ref(eng.scene, O, D, tmax)
    assert (ref[0][0] == t0).mean() > 0.5, "the constructed rays should hit their triangle at t0"
    assert ref[1].mean() > 0.5
    out = {}
    for fit in (1, 0):
        eng.set_option("fit", fit)
        out[fit] = _mismatches(eng, ref, O, D, tmax)
    eng.set_option("fit", 1)
    return out


def test_touching_rays_after_a_commit_to_1e6():
    """The exactly touching rays of test_gpu_wide_bound (FP64 tmax == tmin in hitAABB, the hit on the
    triangle's edge) at an instance built near the origin and committed to the dyadic offset
    (1048576, -524288, 786432): closest hits and occlusion are bit-equal to the oracle at the
    production widening through the fit tree and through tw_walk, and differ with wide_delta_scale
    = 0.  Built at the offset and committed back to the origin they stay exact.
    Measured on an MI355X, mismatching (closest hits, occlusion results) of 6000 rays without the
    widening: fit (85, 93), tw (4, 12)."""
    sc, corners = _touching_scene((16.0, 0.0, 0.0))
    eng = _engine(sc)
    eng.set_transform(1, M.translation(*_DYADIC))
    assert eng.commit().instances_moved == 1
    d = eng.wide_read()
    W.assert_ok(d, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    assert d["wide_coord"] >= 1048576.0 and d["fit_coord"] >= 1048576.0
    world = corners + np.asarray(_DYADIC)
    good = _touching_counts(eng, world, 5)
    print(f"touching rays after a commit to 1e6, production widening: {good}")
    assert good == {1: (0, 0), 0: (0, 0)}, f"mismatches at the production widening: {good}"
    eng.set_unsafe_option("wide_delta_scale", 0)
    bare = _touching_counts(eng, world, 5)
    print(f"touching rays after a commit to 1e6, no widening: fit {bare[1]}, tw {bare[0]} (closest, occlusion) of 6000")
    assert bare[1][0] + bare[1][1] >= 1 and bare[0][0] + bare[0][1] >= 1, bare
    eng.close()
    sc, corners = _touching_scene(_DYADIC)
    eng = _engine(sc)
    eng.set_transform(1, M.translation(16.0, 0.0, 0.0))
    eng.commit()
    W.assert_ok(eng.wide_read(), eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    good = _touching_counts(eng, corners + np.array([16.0, 0.0, 0.0]), 6)
    assert good == {1: (0, 0), 0: (0, 0)}, good
    eng.close()


def test_teeth_after_a_camera_move_to_1e6():
    """The scene stays near the origin; rt_scene_set_camera moves the camera 1e6 out along x, looking
    back.  The frame from there equals the oracle's (set_wide's origin_coord takes the new camera),
    near-vertex rays cast from that distance are bit-equal at the production widening and differ
    without it.  Measured on an MI355X with wide_delta_scale = 0: (54, 20) of 7986 rays mismatch
    (closest hits, occlusion results), through the fit tree and through tw_walk alike."""
    sc, P, F = _teeth_scene((16.0, 0.0, 0.0))
    eng = _engine(sc)
    cam = dataclasses.replace(eng.scene.cameras[0], position=(1.0e6, 3.0e3, 0.0), gaze_point=(16.0, 0.0, 0.0), fovy=2.5)
    eng.set_camera(0, cam)
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)
    _assert_frame(eng, rgb, rgba, st)
    assert float(rgba[..., :3].std()) > 1.0, "the frame must show the mesh"
    rng = np.random.RandomState(63)
    Ov, Dv = _near_vertex_rays(P + np.array([16.0, 0.0, 0.0]), F, 8000, rng, 3.0e4)
    osc = oracle.OracleScene(eng.scene)
    t, tgt, _, _ = osc.trace_rays(Ov, Dv)                        # hit points next to the vertices aimed at
    osc.close()
    tgt = tgt[np.isfinite(t)]
    assert len(tgt) > 2000
    O = np.array([1.0e6, 3.0e3, 0.0]) + rng.uniform(-50.0, 50.0, size=tgt.shape)
    D = tgt - O
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    good = _teeth_counts(eng, eng.scene, O, D)
    assert good == {1: (0, 0), 0: (0, 0)}, good
    eng.set_unsafe_option("wide_delta_scale", 0)
    bare = _teeth_counts(eng, eng.scene, O, D)
    print(f"rays from 1e6, no widening: fit {bare[1]}, tw {bare[0]} (closest, occlusion) of {len(O)}")
    assert bare[1][0] + bare[1][1] >= 1 and bare[0][0] + bare[0][1] >= 1, bare
    eng.close()


# ---------------------------------------------------------------- 6. kappa block and release
@pytest.mark.parametrize("start", ["fit_tree", "blocked_from_creation"])
def test_kappa_block_and_release(start):
    free = posed(1)
    sc = small_scene([posed(0), free if start == "fit_tree" else _kappa_pose()])
    eng = _engine(sc)
    d = eng.wide_read()
    assert (d["fit_root"] >= 0) == (start == "fit_tree") and d["fit_blocked"] == 0
    O, D = _ray_set(np.array([0.0, 0.5, 0.0]), 4.0, 1200, 81)
    rng = np.random.RandomState(82)     # and 800 rays cast down (the free poses) and along -z (the squashed strip)
    for axis, origin, spread in ((1, (0.0, 4.0, 0.0), (1.5, 0.0, 1.5)), (2, (0.0, 1.0, 4.0), (1.9, 0.5, 0.0))):
        aim = -np.eye(3)[axis] + rng.normal(scale=0.02, size=(800, 3))
        O = np.concatenate([O, np.array(origin) + rng.uniform(-1.0, 1.0, size=(800, 3)) * np.array(spread)])
        D = np.concatenate([D, aim / np.linalg.norm(aim, axis=1, keepdims=True)])
    tmax = np.random.RandomState(8).uniform(0.1, 12.0, size=len(O))
    for step, pose in enumerate((_kappa_pose(), free, _m16(np.eye(3) * 0.7, (0.5, 0.2, -0.3)))):
        eng.set_transform(2, pose)
        assert eng.commit().instances_moved == 1
        d = eng.wide_read()
        W.assert_ok(d, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
        assert d["fit_blocked"] == (1 if step == 0 else 0)
        assert (d["fit_root"] >= 0) == (start == "fit_tree"), "a scene built without the tree never gets one"
        ref = _ref(eng.scene, O, D, tmax)
        aimed = ref[0][0][-800:] if step == 0 else ref[0][0][-1600:-800]
        assert np.isfinite(aimed).mean() > (0.15 if step == 0 else 0.5), "the rays cast at instance 2 must hit"
        _assert_rays(eng, ref, O, D, tmax)
    eng.close()


# ---------------------------------------------------------------- 7. scale across binades
@pytest.mark.parametrize("walk", ["transformed", "nested"])
def test_scale_across_binades(walk):
    """One instance of the grazing, near-degenerate mesh of tests/test_gpu_rays.py is committed to
    scales 2^-20 .. 2^20 (prune_k, det_scale and with them fast_rcp move by forty binades) beside
    an instance at unit scale; its rays go through the same similarity."""
    mesh, O0, D0, _ = _grazing_set(1500)
    mesh.transform = M.translation(0.0, 0.0, -2.0e3)
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    rot = _rotation(np.random.RandomState(2))
    sc.objects = [mesh, M.MeshInstance(id=5, base_mesh_id=1, material="1", transform=_m16(rot, (3.0, 1.0, 2.0)))]
    eng = _engine(sc, walk)
    rng = np.random.RandomState(9)
    for e in (-20, -10, 10, 20, 0):
        s = 2.0 ** e
        t = np.array([3.0, 1.0, 2.0]) * (1.0 if e <= 0 else s)
        eng.set_transform(1, _m16(rot * s, t))
        assert eng.commit().instances_moved == 1
        O = (O0 @ rot.T) * s + t
        D = D0 @ rot.T
        O = np.concatenate([O, O0 + np.array([0.0, 0.0, -2.0e3])])      # and the unit-scale instance's own set
        D = np.concatenate([D, D0])
        ref_t = _ref(eng.scene, O, D, np.full(len(O), 1.0e30))
        tmax = _tmax(ref_t[0][0], rng, 1.0e3 * max(s, 1.0))
        ref = _ref(eng.scene, O, D, tmax)
        if e >= 0:
            assert np.isfinite(ref[0][0][: len(O0)]).mean() > 0.2, "the scaled instance must be hit"
        assert np.isfinite(ref[0][0][len(O0):]).mean() > 0.2
        _assert_rays(eng, ref, O, D, tmax)
        d = eng.wide_read()
        assert d["wide_root"] >= 0 and d["fit_root"] >= 0
        W.assert_ok(d, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
        assert d["wide_coord"] >= np.abs(d["inst_bounds"]).max()
        assert d["fit_coord"] >= np.abs(d["inst_bounds"][eng.instance_of(1)]).max() and d["fit_coord"] >= np.abs(t).max()
        lo, hi = eng.instance_bounds(eng.instance_of(1))
        P = (np.asarray(mesh.positions) @ rot.T) * s + t
        assert (lo <= P.min(axis=0)).all() and (hi >= P.max(axis=0)).all(), "the bounds cover the new pose"
    eng.close()
