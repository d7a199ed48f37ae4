"""rt_scene_commit_ex(RT_COMMIT_REBUILD_FIT): the flattened instance tree built again on the device
(rebuild.h) for the committed pose.

The tree is a superset filter (wide.h fit header), so a rebuild may change its topology and nothing
else: the four-wide nodes are read back with rt_debug_wide_read and checked slot by slot by
tests/wide_tree_check.py against an FP64 restatement - exactly, no tolerance - and hits, frames and
ray counts are compared with the oracle at the engine's current pose, bit for bit (the frame criteria
are the suite's: test_gpu_refit._assert_frame).  Scenes are small meshes as instances, in the style of
tests/test_gpu_refit_edges.py, whose helpers are used."""
import dataclasses
import os
import sys

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import engine, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_tree_check as W                                                      # noqa: E402
import deform_scenes as DS                                                       # noqa: E402
from test_fit_coincident import _stacked                                        # noqa: E402
from test_gpu_refit import _assert_frame, _assert_rays, _m16, _mat, _ray_set, _rotation   # noqa: E402
from test_gpu_refit_edges import (_aimed_rays, _count_rays, _engine, _kappa_pose, _ref, _set_walk,   # noqa: E402
                                  _spread, _teeth_counts, _teeth_scene, _touching_counts, _touching_scene)
from test_gpu_wide_bound import _near_vertex_rays                               # noqa: E402
from test_wide_build import posed, small_scene                                  # noqa: E402

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- helpers
def _rebuild(eng, pairs=None):
    """commit(rebuild=True) that must rebuild; returns the stats."""
    cs = eng.commit(rebuild=True)
    rs = eng.last_rebuild_stats()
    assert (rs.rebuilt, rs.reason) == (1, A.RT_REBUILD_NONE), (rs.rebuilt, rs.reason)
    assert rs.nodes_after >= (rs.pairs + 3) // 4 and 3 * rs.depth_after + 2 <= 128
    assert cs.total_ms >= rs.total_ms >= rs.sort_ms >= 0.0 and rs.total_ms >= rs.build_ms > 0.0
    if pairs is not None:
        assert rs.pairs == pairs
    return rs


def _tree(eng, slot=0):
    """The read-back of the replica's trees, verified."""
    d = eng.wide_read(slot)
    W.assert_ok(d, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    return d


def _matches_stats(d, rs):
    assert (d["fit_nodes"], d["pairs"]) == (rs.nodes_after, rs.pairs)
    assert d["wide_copy"] == d["fit_root"] + d["fit_nodes"] and d["wnodes"] == 8 * d["wide_copy"]


def _fit_and_tw_exact(eng, O, D, tmax):
    """Bit equality with the oracle at the current pose through the fit walk and through tw_walk."""
    ref = _ref(eng.scene, O, D, tmax)
    for walk in ("transformed", "transformed_tw"):
        _set_walk(eng, walk)
        _assert_rays(eng, ref, O, D, tmax)
    _set_walk(eng, "transformed")
    return ref


def _hits(eng, O, D, tmax):
    t, p, n, m = eng.trace_rays(O, D)
    return t.view(np.uint64).copy(), p.view(np.uint64).copy(), n.view(np.uint64).copy(), m.copy(), eng.occluded_rays(O, D, tmax).copy()


def _same_hits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _frame(eng):
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)
    _assert_frame(eng, rgb, rgba, st)
    return st


def _one_run_scene(count):
    """`count` instances of a mesh of one triangle (one leaf run): `count` pairs."""
    return small_scene([_spread(k) for k in range(count - 1)], n=6, faces=1, base_at=(0.0, 6.0, 0.0))


# ---------------------------------------------------------------- 1. structure
@pytest.mark.parametrize("count", [2, 3, 4, 5, 64, 65, 256, 257])
def test_structure_by_pair_count(count):
    """2 pairs (the smallest tree), 3, 4 and 5 (the first node that overflows four slots), a wave
    and a block and one past each: every instance moves, the commit rebuilds, the tree is valid, and
    hits and a frame are the oracle's."""
    sc = _one_run_scene(count)
    eng = _engine(sc)
    assert eng.wide_read()["pairs"] == count
    for k in range(count - 1):
        eng.set_transform(1 + k, _spread(k, seed=1))
    eng.set_transform(0, M.translation(1.0, -6.0, 0.5))
    rs = _rebuild(eng, pairs=count)
    d = _tree(eng)
    _matches_stats(d, rs)
    O, D, aimed = _count_rays(eng.scene, 9 + count)
    tmax = np.random.RandomState(count).uniform(0.1, 20.0, size=len(O))
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0][-aimed:]).mean() > 0.5, "the aimed rays must hit"
    _frame(eng)
    eng.close()


def test_structure_of_a_few_thousand_pairs():
    """60 instances of a mesh of 64 leaf runs: a multi-block sort, and levels on both sides of a block."""
    sc = small_scene([_spread(k) for k in range(59)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc)
    pairs = int(eng.wide_read()["pairs"])
    assert pairs >= 2000 and pairs % 60 == 0
    for k in range(59):
        eng.set_transform(1 + k, _spread(k, seed=1))
    rs = _rebuild(eng, pairs=pairs)
    d = _tree(eng)
    _matches_stats(d, rs)
    rep = W.verify(d, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    sizes = rep.trees["fit"]["levels"]
    print("rebuilt fit tree levels:", sizes, "depth", rs.depth_after, "nodes", rs.nodes_before, "->", rs.nodes_after)
    assert len(sizes) == rs.depth_after and sum(sizes) == rs.nodes_after
    assert any(4 * s < 256 for s in sizes) and any(s > 256 for s in sizes)
    O, D, aimed = _count_rays(eng.scene, 77)
    tmax = np.random.RandomState(5).uniform(0.1, 20.0, size=len(O))
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0][-aimed:]).mean() > 0.5
    _frame(eng)
    eng.close()


def test_one_pair_alone_has_nothing_to_rebuild():
    sc = small_scene([], n=6, faces=1, base_at=(0.0, 0.0, 0.0))
    eng = _engine(sc)
    O, D = _ray_set(np.array([0.0, 0.5, 0.0]), 3.0, 400, 3)
    tmax = np.random.RandomState(1).uniform(0.1, 9.0, size=len(O))
    before = eng.wide_read()
    assert before["fit_root"] < 0
    h0 = _hits(eng, O, D, tmax)
    cs = eng.commit(rebuild=True)
    rs = eng.last_rebuild_stats()
    assert (rs.rebuilt, rs.reason, rs.pairs, cs.instances_moved) == (0, A.RT_REBUILD_NO_TREE, 0, 0)
    assert W.same_dump(before, eng.wide_read()) is None
    assert _same_hits(h0, _hits(eng, O, D, tmax))
    _assert_rays(eng, _ref(eng.scene, O, D, tmax), O, D, tmax)
    eng.close()


# ---------------------------------------------------------------- 2. degenerate keys
@pytest.mark.parametrize("n", [5, 8, 33])
def test_stacked_instances_then_moved_apart(n):
    """Every instance at one pose: all Morton codes of a leaf run's pairs are equal, and the sorted
    position tells them apart.  Then a plain commit moves them apart over the rebuilt topology."""
    sc = scenes.scaled(_stacked(n), 24, 16)
    sc.cameras[0].position = (0.5, 9.0, 4.0)
    sc.cameras[0].gaze_point = (0.5, -0.25, 1.0)
    eng = _engine(sc)
    O, D = _ray_set(np.array([0.5, -0.25, 1.0]), 4.0, 1200, 40 + n)
    tmax = np.random.RandomState(n).uniform(0.1, 12.0, size=len(O))
    rs = _rebuild(eng)
    _matches_stats(_tree(eng), rs)
    runs = rs.pairs // (n + 1)
    # balanced, not a chain: n stacked copies of a run need about log4(n) levels more, not n
    assert rs.depth_after <= 4 + int(np.ceil(np.log2(max(runs, 2)))) + int(np.ceil(np.log2(n))), rs.depth_after
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0]).mean() > 0.1
    st = _frame(eng)
    assert st.rewalked > 0, "every hit of the stack is a tie between instances"
    rng = np.random.RandomState(50 + n)
    for k in range(n):
        eng.set_transform(1 + k, _m16(_rotation(rng) * (1.0 + 0.02 * k), (2.5 * (k % 3) - 2.0, 0.6 * (k % 7) - 2.0, 2.5 * ((k // 3) % 4))))
    assert eng.commit().instances_moved == n
    assert eng.last_rebuild_stats().rebuilt == 0 and eng.last_rebuild_stats().pairs == 0
    d = _tree(eng)
    assert d["fit_nodes"] == rs.nodes_after, "the plain commit refits the rebuilt topology"
    _fit_and_tw_exact(eng, O, D, tmax)
    _frame(eng)
    eng.close()


def _flat_scene(offsets):
    """A flat mesh (two triangles in the plane z = 0, float-exact) instanced by pure translations."""
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    mesh = M.Mesh(id=1, material="1", positions=P, indices=F, indices_one_based=False, shading_mode="flat",
                  transform=M.translation(*offsets[0]))
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [mesh] + [M.MeshInstance(id=10 + k, base_mesh_id=1, material="1", transform=M.translation(*o))
                           for k, o in enumerate(offsets[1:])]
    return sc


@pytest.mark.parametrize("shape", ["plane", "line", "point_and_plane"])
def test_centroids_in_a_plane_and_on_a_line(shape):
    """The union of the pair boxes has zero extent along z (flat boxes in one plane): that axis
    contributes code bits 0, without a division.  On a line the centroids also share y; with every
    instance but one at one place the codes take two values only."""
    rng = np.random.RandomState(7)
    if shape == "plane":
        offs = [(1.5 * (k % 5), 1.5 * (k // 5), 0.0) for k in range(23)]
    elif shape == "line":
        offs = [(1.25 * k, 0.0, 0.0) for k in range(19)]
    else:
        offs = [(0.0, 0.0, 0.0)] * 9 + [(4.0, 0.0, 0.0)]
    sc = _flat_scene([(20.0, 0.0, 0.0)] + offs)
    eng = _engine(sc)
    eng.set_transform(0, M.translation(*(offs[0] if shape != "point_and_plane" else (4.0, 2.0, 0.0))))
    rs = _rebuild(eng)
    d = _tree(eng)
    _matches_stats(d, rs)
    fr = int(d["fit_root"])
    near, _, far, _ = W.split_nodes(d["nodes"][fr:fr + 1])
    assert np.all(near[0, 2][near[0, 0] < np.inf] == 0.0) and np.all(far[0, 2][near[0, 0] < np.inf] == 0.0), "flat in z"
    tgt = np.array(offs) + rng.uniform(0.05, 0.95, size=(len(offs), 3)) * np.array([1.0, 1.0, 0.0])
    tgt = np.repeat(tgt, 12, axis=0)
    Dr = rng.normal(size=tgt.shape)
    Dr /= np.linalg.norm(Dr, axis=1, keepdims=True)
    O = np.concatenate([tgt - Dr * rng.uniform(0.2, 3.0, size=(len(tgt), 1)), tgt + np.array([0.0, 0.0, 2.0])])
    D = np.concatenate([Dr, np.tile([0.0, 0.0, -1.0], (len(tgt), 1))])
    tmax = rng.uniform(0.1, 6.0, size=len(O))
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0]).mean() > 0.5
    _frame(eng)
    eng.close()


def test_an_instance_committed_to_1e6():
    """Built near the origin, one instance rebuilt at (1e6, 1e6, 1e6): the union of the pair boxes
    spans 1e6, so every pair of the far instance shares a handful of code values; the near-vertex
    rays there stay bit-equal to the oracle through the fit tree and tw_walk."""
    sc, P, F = _teeth_scene((16.0, 0.0, 0.0))
    eng = _engine(sc)
    far = (1.0e6, 1.0e6, 1.0e6)
    eng.set_transform(1, M.translation(*far))
    rs = _rebuild(eng)
    d = _tree(eng)
    _matches_stats(d, rs)
    assert d["wide_coord"] >= 1.0e6 and d["fit_coord"] >= 1.0e6
    O, D = _near_vertex_rays(P + np.asarray(far), F, 4000, np.random.RandomState(61), 3.0e4)
    good = _teeth_counts(eng, eng.scene, O, D)
    assert good == {1: (0, 0), 0: (0, 0)}, f"mismatches after the rebuild: {good}"
    _frame(eng)
    eng.close()


@pytest.mark.parametrize("e", [-20, 20])
def test_scales_across_binades(e):
    sc = small_scene([posed(0), posed(1), posed(2)], n=8)
    eng = _engine(sc)
    s = 2.0 ** e
    rot = _rotation(np.random.RandomState(2))
    t = np.array([3.0, 1.0, 2.0]) * (1.0 if e <= 0 else s)
    eng.set_transform(1, _m16(rot * s, t))
    rs = _rebuild(eng)
    _matches_stats(_tree(eng), rs)
    Oa, Da = _aimed_rays(eng.scene, 4, 12)
    Oa = np.concatenate([Oa, np.repeat(t[None, :], 40, axis=0) + np.random.RandomState(3).normal(size=(40, 3)) * 3.0 * s])
    Da = np.concatenate([Da, -np.random.RandomState(3).normal(size=(40, 3))])
    Da /= np.linalg.norm(Da, axis=1, keepdims=True)
    O0, D0 = _ray_set(np.array([0.0, 0.0, 0.0]), 4.0, 800, 13)
    O, D = np.concatenate([O0, Oa]), np.concatenate([D0, Da])
    tmax = np.random.RandomState(4).uniform(0.1, 20.0 * max(s, 1.0), size=len(O))
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0]).mean() > 0.1
    _frame(eng)
    eng.close()


# ---------------------------------------------------------------- 3. exactness
def test_touching_rays_before_and_after_a_rebuild():
    """The exactly touching rays of test_gpu_wide_bound's construction (FP64 tmax == tmin in hitAABB)
    at an instance committed to a dyadic offset of 1e6: zero mismatches against the oracle through the
    fit tree and tw_walk after the rebuild, and the same bits as the engine gave before it."""
    from test_gpu_refit_edges import _DYADIC
    from test_gpu_wide_bound import _touching_rays
    sc, corners = _touching_scene((16.0, 0.0, 0.0))
    eng = _engine(sc)
    eng.set_transform(1, M.translation(*_DYADIC))
    eng.commit()
    world = corners + np.asarray(_DYADIC)
    O, D, t0 = _touching_rays(world, 4.0, np.random.RandomState(5), 6000)
    tmax = t0 * (1 + 2.0 ** -40)
    before = {}
    for walk in ("transformed", "transformed_tw"):
        _set_walk(eng, walk)
        before[walk] = _hits(eng, O, D, tmax)
    _set_walk(eng, "transformed")
    rs = _rebuild(eng)                                      # nothing staged: the pose as it stands
    _matches_stats(_tree(eng), rs)
    good = _touching_counts(eng, world, 5)
    assert good == {1: (0, 0), 0: (0, 0)}, f"mismatches after the rebuild: {good}"
    for walk in ("transformed", "transformed_tw"):
        _set_walk(eng, walk)
        assert _same_hits(before[walk], _hits(eng, O, D, tmax)), walk
    eng.close()


def test_near_vertex_rays_before_and_after_a_rebuild():
    sc, P, F = _teeth_scene((16.0, 0.0, 0.0))
    eng = _engine(sc)
    O, D = _near_vertex_rays(P + np.array([16.0, 0.0, 0.0]), F, 4000, np.random.RandomState(62), 3.0e4)
    tmax = np.full(len(O), 1.0e7)
    before = {}
    for walk in ("transformed", "transformed_tw"):
        _set_walk(eng, walk)
        before[walk] = _hits(eng, O, D, tmax)
    _set_walk(eng, "transformed")
    rs = _rebuild(eng)
    _matches_stats(_tree(eng), rs)
    good = _teeth_counts(eng, eng.scene, O, D)
    assert good == {1: (0, 0), 0: (0, 0)}, good
    for walk in ("transformed", "transformed_tw"):
        _set_walk(eng, walk)
        assert _same_hits(before[walk], _hits(eng, O, D, tmax)), walk
    _set_walk(eng, "transformed")
    _frame(eng)
    eng.close()


def test_equal_t_ties_keep_the_references_winner():
    """Two instances of one grid under one transform, with different materials, and rays through
    the grid's shared vertices and edge midpoints: every hit is a tie between the instances and many
    are ties between triangles too.  After a rebuild the winner (material, normal) is the
    reference's, and the frame reports re-walked rays."""
    hp, hf = scenes.heightfield(12, 8.0, 1.0, 3)
    hp32 = hp.astype(np.float32).astype(np.float64)
    a = M.Mesh(id=1, material="1", positions=hp32, indices=hf.astype(np.int32), indices_one_based=False,
               shading_mode="flat", transform=M.translation(0.0, 0.0, -30.0))
    c, sn = np.cos(0.5), np.sin(0.5)
    Mt = np.eye(4)
    Mt[:3, :3] = np.array([[c, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, c]]) * 0.75
    Mt[:3, 3] = (0.25, -0.5, 0.125)
    T = tuple(Mt.T.reshape(-1))
    sc = scenes.scaled(scenes.scene_c1(8, 8), 24, 20)
    sc.materials = [sc.materials[0], dataclasses.replace(sc.materials[0], diffuse=(0.1, 0.9, 0.2))]
    sc.objects = [a, M.MeshInstance(id=5, base_mesh_id=1, material="1", transform=T),
                  M.MeshInstance(id=6, base_mesh_id=1, material="2", transform=T)]
    sc.cameras[0].position = (0.5, 7.0, 7.5)
    sc.cameras[0].gaze_point = (0.0, 0.0, 0.0)
    sc.point_lights[0].position = (1.0, 9.0, 2.0)
    eng = _engine(sc)
    rng = np.random.RandomState(4)
    tri = hf[rng.choice(len(hf), 200)]
    va, vb, vc = hp32[tri[:, 0]], hp32[tri[:, 1]], hp32[tri[:, 2]]
    loc = np.concatenate([hp32[rng.choice(len(hp32), 150)], 0.5 * (va + vb), 0.5 * (vb + vc), (va + vb + vc) / 3.0])
    tgt = loc @ Mt[:3, :3].T + Mt[:3, 3]
    Dd = np.array([0.3, -1.0, 0.2]) / np.linalg.norm([0.3, -1.0, 0.2])
    D = np.concatenate([np.tile(Dd, (len(tgt), 1)), np.tile([0.0, -1.0, 0.0], (len(tgt), 1))])
    O = np.concatenate([tgt - 10.0 * Dd, tgt + np.array([0.0, 10.0, 0.0])])
    tmax = np.full(len(O), 9.999)
    rs = _rebuild(eng)
    _matches_stats(_tree(eng), rs)
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0]).mean() > 0.5
    st = _frame(eng)
    assert st.rewalked > 0, "no tie was handed to the reference-order walk"
    eng.close()


# ---------------------------------------------------------------- 4. life after a rebuild
def test_rebuild_move_commit_and_back():
    sc = small_scene([_spread(k) for k in range(40)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc)
    O, D, _ = _count_rays(eng.scene, 21)
    tmax = np.random.RandomState(2).uniform(0.1, 20.0, size=len(O))
    pose_a = {1 + k: _spread(k, seed=1) for k in range(40)}
    pose_b = {1 + k: _spread(k, seed=2) for k in range(40)}
    for i, m in pose_a.items():
        eng.set_transform(i, m)
    rs = _rebuild(eng)
    at_a = _tree(eng)
    _matches_stats(at_a, rs)
    ref_a = _fit_and_tw_exact(eng, O, D, tmax)
    for i, m in pose_b.items():
        eng.set_transform(i, m)
    assert eng.commit().instances_moved == 40
    zero = eng.last_rebuild_stats()
    assert (zero.rebuilt, zero.reason, zero.pairs, zero.nodes_after, zero.total_ms) == (0, 0, 0, 0, 0.0)
    at_b = _tree(eng)                                         # the new fit_levels are the ones refit
    assert at_b["fit_nodes"] == rs.nodes_after and not np.array_equal(at_a["nodes"], at_b["nodes"])
    _fit_and_tw_exact(eng, O, D, tmax)
    for i, m in pose_a.items():
        eng.set_transform(i, m)
    eng.commit()
    back = _tree(eng)
    fr, fn = int(at_a["fit_root"]), int(at_a["fit_nodes"])
    assert np.array_equal(W.node_multisets(back, fr, fr + fn), W.node_multisets(at_a, fr, fr + fn))
    _assert_rays(eng, ref_a, O, D, tmax)
    _frame(eng)
    eng.close()


def test_twenty_rebuilds_and_two_replicas_are_byte_identical():
    sc = small_scene([_spread(k) for k in range(30)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc, devices=[0, 0])
    for k in range(30):
        eng.set_transform(1 + k, _spread(k, seed=3))
    _rebuild(eng)
    first = _tree(eng, 0)
    assert W.same_dump(first, _tree(eng, 1)) is None, "the replicas differ"
    for _ in range(20):
        _rebuild(eng)
    d0, d1 = eng.wide_read(0), eng.wide_read(1)
    assert W.same_dump(first, d0) is None, f"a rebuild at one pose changed {W.same_dump(first, d0)}"
    assert W.same_dump(d0, d1) is None, f"the replicas differ in {W.same_dump(d0, d1)}"
    O, D, _ = _count_rays(eng.scene, 31)
    tmax = np.random.RandomState(3).uniform(0.1, 20.0, size=len(O))
    _fit_and_tw_exact(eng, O, D, tmax)
    eng.close()


def test_a_deformable_scene_stages_positions_and_a_transform_and_rebuilds():
    sc = DS.base_scene("smooth", sizes=(1, 3, 65))
    leaf_of = W.tlas_leaves(sc)
    eng = M.RayTracerEngine(sc, None, deformable=True)
    eng.leaf_of = leaf_of
    d0 = eng.wide_read()
    assert d0["fit_root"] >= 0
    meshes = [i for i, o in enumerate(eng.scene.objects) if isinstance(o, M.Mesh)]
    big = max(meshes, key=lambda i: len(np.asarray(eng.scene.objects[i].positions).reshape(-1, 3)))
    pos = np.asarray(eng.scene.objects[big].positions, np.float64).reshape(-1, 3)
    new = pos * np.array([1.25, 0.75, 1.5]) + 0.125 * np.sin(3.0 * pos[:, [1, 2, 0]])
    eng.set_positions(big, new)
    m = _mat(eng.scene.objects[big].transform).copy()
    m[:3, 3] += (1.5, -0.5, 0.75)
    eng.set_transform(big, tuple(m.T.reshape(-1)))
    cs = eng.commit(rebuild=True)
    rs = eng.last_rebuild_stats()
    assert rs.rebuilt == 1 and cs.instances_moved == 1 and eng.last_deform_stats().meshes_deformed == 1
    d = _tree(eng)
    _matches_stats(d, rs)
    rng = np.random.RandomState(8)
    obj = eng.scene.objects[big]
    faces = np.asarray(obj.indices, np.int64).reshape(-1, 3) - (1 if obj.indices_one_based else 0)
    cen = new[faces[rng.choice(len(faces), 400)]].mean(axis=1)         # face centroids of the deformed mesh
    tgt = cen @ m[:3, :3].T + m[:3, 3]                                  # ... at its new place
    Da = rng.normal(size=tgt.shape)
    Da /= np.linalg.norm(Da, axis=1, keepdims=True)
    c = np.asarray(eng.instance_bounds(eng.instance_of(big))).mean(axis=0)
    O0, D0 = _ray_set(c, 3.0, 600, 8)
    O, D = np.concatenate([O0, tgt - Da * rng.uniform(0.05, 2.0, size=(len(tgt), 1))]), np.concatenate([D0, Da])
    tmax = rng.uniform(0.1, 12.0, size=len(O))
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0][-400:]).mean() > 0.5, "the rays aimed at the deformed mesh must hit"
    _frame(eng)
    eng.close()


def test_a_refused_commit_leaves_the_tree_and_the_stats():
    sc = small_scene([_spread(k) for k in range(12)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc)
    eng.set_transform(3, _spread(3, seed=4))
    rs = _rebuild(eng)
    kept = eng.wide_read()
    eng.set_transform(2, _m16(np.eye(3), (1.0e31, 0.0, 0.0)))
    with pytest.raises(M.RenderError) as e:
        eng.commit(rebuild=True)
    assert e.value.code == A.RT_ERR_INVALID_ARG
    after = eng.last_rebuild_stats()
    for f, _ in A.rt_rebuild_stats._fields_:
        assert getattr(after, f) == getattr(rs, f), f
    lib = M.load_library()
    io = A.rt_wide_dump()
    assert lib.rt_debug_wide_read(eng._h, 0, io) == 0 and (io.fit_nodes, io.wide_copy) == (kept["fit_nodes"], kept["wide_copy"])
    nodes = np.zeros((int(io.wnodes), 32), np.uint32)
    io.cap_wnodes, io.nodes = io.wnodes, nodes.ctypes.data
    assert lib.rt_debug_wide_read(eng._h, 0, io) == 0
    assert np.array_equal(nodes, kept["nodes"]), "the refused commit touched the node array"
    eng.close()


# ---------------------------------------------------------------- 5. guards
def test_depth_cap_leaves_the_old_tree():
    sc = small_scene([_spread(k) for k in range(20)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc)
    for k in range(20):
        eng.set_transform(1 + k, _spread(k, seed=5))
    eng.commit()
    kept = _tree(eng)
    O, D, _ = _count_rays(eng.scene, 41)
    tmax = np.random.RandomState(4).uniform(0.1, 20.0, size=len(O))
    with pytest.raises(M.RenderError):
        eng.set_option("rebuild_depth_cap", 3)              # a test hook: refused by rt_scene_set_option
    with pytest.raises(M.RenderError):
        eng.set_unsafe_option("rebuild_depth_cap", 43)      # it can only be lowered
    assert eng.get_option("rebuild_depth_cap") == 42
    eng.set_unsafe_option("rebuild_depth_cap", 3)
    cs = eng.commit(rebuild=True)
    rs = eng.last_rebuild_stats()
    assert (rs.rebuilt, rs.reason, cs.instances_moved) == (0, A.RT_REBUILD_TOO_DEEP, 0)
    assert (rs.nodes_after, rs.depth_after) == (rs.nodes_before, rs.depth_before) == (kept["fit_nodes"], rs.depth_before)
    assert W.same_dump(kept, eng.wide_read()) is None, "the old tree must stay byte for byte"
    _fit_and_tw_exact(eng, O, D, tmax)
    eng.set_unsafe_option("rebuild_depth_cap", 42)
    rs = _rebuild(eng)
    assert rs.depth_after > 3
    _matches_stats(_tree(eng), rs)
    _fit_and_tw_exact(eng, O, D, tmax)
    eng.close()


def test_blocked_by_kappa_then_released():
    free = posed(1)
    sc = small_scene([posed(0), free])
    eng = _engine(sc)
    O, D = _ray_set(np.array([0.0, 0.5, 0.0]), 4.0, 1000, 81)
    tmax = np.random.RandomState(8).uniform(0.1, 12.0, size=len(O))
    eng.set_transform(2, _kappa_pose())
    cs = eng.commit(rebuild=True)
    rs = eng.last_rebuild_stats()
    assert (rs.rebuilt, rs.reason, cs.instances_moved) == (0, A.RT_REBUILD_BLOCKED, 1)
    d = _tree(eng)
    assert d["fit_blocked"] == 1
    _assert_rays(eng, _ref(eng.scene, O, D, tmax), O, D, tmax)
    eng.set_transform(2, free)
    rs = _rebuild(eng)
    d = _tree(eng)
    assert d["fit_blocked"] == 0
    _matches_stats(d, rs)
    _fit_and_tw_exact(eng, O, D, tmax)
    eng.close()


def test_static_busy_and_unknown_flags():
    sc = small_scene([posed(0), posed(1)])
    lib = M.load_library()
    static = M.RayTracerEngine(sc, None)
    with pytest.raises(M.RenderError) as e:
        static.commit(rebuild=True)
    assert e.value.code == A.RT_ERR_UNSUPPORTED
    static.close()
    eng = _engine(sc)
    assert lib.rt_scene_commit_ex(eng._h, 2, None) == A.RT_ERR_INVALID_ARG
    assert lib.rt_scene_commit_ex(eng._h, A.RT_COMMIT_REBUILD_FIT | 4, None) == A.RT_ERR_INVALID_ARG
    kept = eng.wide_read()
    rgb = M.pinned_array((8, 8, 3), np.float64)
    ticket = eng.submit_into(0, 0, 1, rgb, None)
    with pytest.raises(M.RenderError) as e:
        eng.commit(rebuild=True)
    assert e.value.code == A.RT_ERR_BUSY
    eng.wait(ticket)
    assert W.same_dump(kept, eng.wide_read()) is None
    assert eng.last_rebuild_stats().rebuilt == 0
    _rebuild(eng)
    _tree(eng)
    eng.close()


# ---------------------------------------------------------------- 6. what the rebuild is for
def _fit_cost(d):
    """Sum over the non-empty slots of the fit nodes of the slot box's surface area, over the area of
    the union of the root's slots (copy 0; FP64 from the float rows)."""
    fr, fn = int(d["fit_root"]), int(d["fit_nodes"])
    near, _, far, _ = W.split_nodes(d["nodes"][fr:fr + fn])
    full = near[:, 0, :] < np.inf
    f3 = np.broadcast_to(full[:, None, :], near.shape)
    e = np.where(f3, far, 0.0).astype(np.float64) - np.where(f3, near, 0.0).astype(np.float64)
    area = e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    lo = np.where(full[0][None, :], near[0].astype(np.float64), np.inf).min(axis=1)
    hi = np.where(full[0][None, :], far[0].astype(np.float64), -np.inf).max(axis=1)
    r = hi - lo
    return float(area.sum() / (r[0] * r[1] + r[1] * r[2] + r[2] * r[0]))


def _grid_pose(cell, k):
    rng = np.random.RandomState(300 + k)                     # the instance keeps its rotation and size
    return _m16(_rotation(rng) * 0.2, (2.0 * (cell % 8) - 7.0, 0.3 * rng.uniform(-1, 1), 2.0 * (cell // 8) - 7.0))


def test_a_rebuild_lowers_the_tree_cost_of_a_shuffled_grid():
    """An 8 x 8 grid of small mesh instances committed to a random permutation of the grid's cells:
    the kept topology groups instances that now lie far apart.  cost_fresh < cost_refit shows that the
    pose degrades the kept topology; the rebuild must then lower the cost too.  cost_rebuilt /
    cost_fresh is printed, not asserted (what Morton order loses to SAH here is a measurement)."""
    sc = small_scene([_grid_pose(k, k) for k in range(1, 64)], n=6, base_at=(-7.0, 0.0, -7.0))
    sc.objects[0].transform = _grid_pose(0, 0)
    eng = _engine(sc)
    perm = np.random.RandomState(11).permutation(64)
    for k in range(64):
        eng.set_transform(k, _grid_pose(int(perm[k]), k))
    assert eng.commit().instances_moved == 64
    cost_refit = _fit_cost(_tree(eng))
    cost_fresh = _fit_cost(engine.wide_build(eng.scene, dynamic=True))
    rs = _rebuild(eng)
    cost_rebuilt = _fit_cost(_tree(eng))
    print(f"fit tree cost of the shuffled 8 x 8 grid ({rs.pairs} pairs): refit {cost_refit:.3f}, rebuilt {cost_rebuilt:.3f}, "
          f"fresh {cost_fresh:.3f}; rebuilt / fresh {cost_rebuilt / cost_fresh:.3f}")
    assert cost_fresh < cost_refit, "the permutation must degrade the kept topology"
    assert cost_rebuilt < cost_refit
    O, D, _ = _count_rays(eng.scene, 51)
    tmax = np.random.RandomState(6).uniform(0.1, 20.0, size=len(O))
    _fit_and_tw_exact(eng, O, D, tmax)
    eng.close()
