"""rt_scene_commit_ex(RT_COMMIT_REBUILD_FIT_CLUSTERED): the flattened instance tree built again on the
device by clustering the Morton-sorted pairs (rebuild.h k_pc_*), the detail
record of a rebuild (rt_scene_last_rebuild_detail) and the tree cost (rt_scene_fit_cost).

The checks are test_gpu_rebuild.py's, whose helpers are used: the four-wide nodes are read back and
verified slot by slot by tests/wide_tree_check.py - exactly, no tolerance - and hits, frames and ray
counts are the oracle's at the engine's current pose, bit for bit.  Every case fails on a library
without the flag, where 8 is an unknown flag bit."""
import ctypes as C
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
from test_gpu_rebuild import (_fit_and_tw_exact, _fit_cost, _frame, _grid_pose, _hits, _matches_stats,   # noqa: E402
                              _one_run_scene, _same_hits, _tree)
from test_gpu_refit import _assert_rays, _m16, _mat, _ray_set, _rotation        # noqa: E402
from test_gpu_refit_edges import (_count_rays, _engine, _ref, _set_walk, _spread, _teeth_counts, _teeth_scene,   # noqa: E402
                                  _touching_counts, _touching_scene)
from test_gpu_wide_bound import _near_vertex_rays                               # noqa: E402
from test_wide_build import posed, small_scene                                  # noqa: E402

pytestmark = pytest.mark.gpu

CLUSTERED = A.RT_COMMIT_REBUILD_FIT_CLUSTERED


# ---------------------------------------------------------------- helpers
def _rebuilt(eng, cs, pairs=None, builder=A.RT_BUILDER_CLUSTERED, fell_back=0):
    """The stats and the detail of a commit that must have rebuilt with `builder`."""
    rs, dt = eng.last_rebuild_stats(), eng.last_rebuild_detail()
    assert (rs.rebuilt, rs.reason) == (1, A.RT_REBUILD_NONE), (rs.rebuilt, rs.reason)
    assert (dt.builder, dt.fell_back) == (builder, fell_back), (dt.builder, dt.fell_back, dt.iterations)
    assert rs.nodes_after >= (rs.pairs + 3) // 4 and 3 * rs.depth_after + 2 <= 128
    assert cs.total_ms >= rs.total_ms >= rs.sort_ms >= 0.0 and rs.total_ms >= rs.build_ms > 0.0
    if builder == A.RT_BUILDER_CLUSTERED:
        cap = 4 * int(np.ceil(np.log2(rs.pairs))) + 32
        assert 1 <= dt.iterations <= min(cap, rs.pairs - 1), dt.iterations
        assert rs.build_ms >= dt.cluster_ms > 0.0, "build_ms includes the clustering"
    assert dt.cost_before > 0.0 and dt.cost_after > 0.0
    if pairs is not None:
        assert rs.pairs == pairs
    return rs, dt


def _rebuild_clustered(eng, pairs=None):
    """commit(rebuild="clustered") that must rebuild with the clustered builder."""
    return _rebuilt(eng, eng.commit(rebuild="clustered"), pairs)


def _rebuild_morton(eng, pairs=None):
    return _rebuilt(eng, eng.commit(rebuild=True), pairs, builder=A.RT_BUILDER_MORTON)


def _zero_detail(dt):
    return all(getattr(dt, f) == 0 for f, _ in A.rt_rebuild_detail._fields_)


def _close(a, b):
    """1e-9 relative: FP64 sums of fewer than 1e4 positive terms differ by at most n 2^-53 < 2e-12
    whatever the order."""
    return abs(a - b) <= 1e-9 * abs(b)


# ---------------------------------------------------------------- 1. structure
@pytest.mark.parametrize("count", [2, 3, 4, 5, 17, 33, 64, 65, 256, 257, 273])
def test_structure_by_pair_count(count):
    """2 pairs (the smallest tree), 3, 4 and 5 (the first node that overflows four slots), one past
    the radius of 16 and past two radii, a wave and a block and one past each, and 256 + 17: a
    cluster whose window crosses the LDS tile's halo.  Every instance moves, the commit rebuilds with
    the clustered builder, the tree is valid, and hits and a frame are the oracle's."""
    sc = _one_run_scene(count)
    eng = _engine(sc)
    assert eng.wide_read()["pairs"] == count
    for k in range(count - 1):
        eng.set_transform(1 + k, _spread(k, seed=1))
    eng.set_transform(0, M.translation(1.0, -6.0, 0.5))
    rs, dt = _rebuild_clustered(eng, pairs=count)
    d = _tree(eng)
    _matches_stats(d, rs)
    assert _close(dt.cost_after, _fit_cost(d)) and _close(eng.fit_cost(), _fit_cost(d))
    O, D, aimed = _count_rays(eng.scene, 9 + count)
    tmax = np.random.RandomState(count).uniform(0.1, 20.0, size=len(O))
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0][-aimed:]).mean() > 0.5, "the aimed rays must hit"
    _frame(eng)
    eng.close()


def test_structure_of_a_few_thousand_pairs():
    """60 instances of a mesh of 64 leaf runs: many blocks of clusters, and levels on both sides of a block."""
    sc = small_scene([_spread(k) for k in range(59)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc)
    pairs = int(eng.wide_read()["pairs"])
    assert pairs >= 2000 and pairs % 60 == 0
    for k in range(59):
        eng.set_transform(1 + k, _spread(k, seed=1))
    rs, dt = _rebuild_clustered(eng, pairs=pairs)
    d = _tree(eng)
    _matches_stats(d, rs)
    rep = W.verify(d, eng.scene, after_refit=True, leaf_of=eng.leaf_of)
    sizes = rep.trees["fit"]["levels"]
    print("clustered fit tree levels:", sizes, "depth", rs.depth_after, "nodes", rs.nodes_before, "->", rs.nodes_after,
          "iterations", dt.iterations, "cost", dt.cost_before, "->", dt.cost_after)
    assert len(sizes) == rs.depth_after and sum(sizes) == rs.nodes_after
    assert any(4 * s < 256 for s in sizes) and any(s > 256 for s in sizes)
    O, D, aimed = _count_rays(eng.scene, 77)
    tmax = np.random.RandomState(5).uniform(0.1, 20.0, size=len(O))
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0][-aimed:]).mean() > 0.5
    _frame(eng)
    eng.close()


# ---------------------------------------------------------------- 3. equal boxes
@pytest.mark.parametrize("n", [5, 8, 33])
def test_stacked_one_run_instances_pair_up(n):
    """n one-run instances committed to one pose: every cluster box is equal, every union area too,
    and the tie rule (the smaller i ^ j) pairs them up as (0, 1), (2, 3), ...: the cluster count
    halves, rounded up, per iteration - ceil(log2 n) of them; a chain would take n - 1.  Then a
    plain commit moves them apart over the rebuilt topology."""
    sc = _one_run_scene(n)
    eng = _engine(sc)
    rng = np.random.RandomState(70 + n)
    pose = _m16(_rotation(rng) * 0.75, (0.5, -0.25, 1.0))
    for k in range(n):
        eng.set_transform(k, pose)
    rs, dt = _rebuild_clustered(eng, pairs=n)
    assert dt.iterations <= int(np.ceil(np.log2(n))) + 1, (dt.iterations, n)
    _matches_stats(_tree(eng), rs)
    O, D = _ray_set(np.array([0.5, -0.25, 1.0]), 3.0, 600, 40 + n)
    tmax = np.random.RandomState(n).uniform(0.1, 12.0, size=len(O))
    _fit_and_tw_exact(eng, O, D, tmax)
    for k in range(n):
        eng.set_transform(k, _spread(k, seed=6))
    assert eng.commit().instances_moved == n
    assert eng.last_rebuild_stats().rebuilt == 0 and _zero_detail(eng.last_rebuild_detail())
    d = _tree(eng)
    assert d["fit_nodes"] == rs.nodes_after, "the plain commit refits the rebuilt topology"
    _fit_and_tw_exact(eng, O, D, tmax)
    eng.close()


# ---------------------------------------------------------------- 4. what the builder is for
def _shuffled_grid_engine():
    sc = small_scene([_grid_pose(k, k) for k in range(1, 64)], n=6, base_at=(-7.0, 0.0, -7.0))
    sc.objects[0].transform = _grid_pose(0, 0)
    eng = _engine(sc)
    perm = np.random.RandomState(11).permutation(64)
    for k in range(64):
        eng.set_transform(k, _grid_pose(int(perm[k]), k))
    assert eng.commit().instances_moved == 64
    return eng


def test_the_clustered_tree_costs_less_than_the_morton_tree_on_the_shuffled_grid():
    """The shuffled 8 x 8 grid of test_gpu_rebuild: cost_clustered < cost_morton < cost_refit.  The
    ratios to the host's SAH tree are printed, not asserted.  The device's cost figures equal
    test_gpu_rebuild._fit_cost of the matching read-back to 1e-9 relative (_close)."""
    a, b = _shuffled_grid_engine(), _shuffled_grid_engine()
    refit = _tree(a)
    cost_refit = _fit_cost(refit)
    assert W.same_dump(refit, b.wide_read()) is None
    assert _close(a.fit_cost(), cost_refit) and _close(b.fit_cost(), cost_refit)
    cost_fresh = _fit_cost(engine.wide_build(a.scene, dynamic=True))
    rs_m, dt_m = _rebuild_morton(a)
    cost_morton = _fit_cost(_tree(a))
    rs_c, dt_c = _rebuild_clustered(b)
    cost_clustered = _fit_cost(_tree(b))
    print(f"fit tree cost of the shuffled 8 x 8 grid ({rs_c.pairs} pairs): refit {cost_refit:.3f}, morton {cost_morton:.3f}, "
          f"clustered {cost_clustered:.3f} ({dt_c.iterations} iterations), fresh {cost_fresh:.3f}; "
          f"morton / fresh {cost_morton / cost_fresh:.3f}, clustered / fresh {cost_clustered / cost_fresh:.3f}")
    assert cost_fresh < cost_refit, "the permutation must degrade the kept topology"
    assert cost_clustered < cost_morton < cost_refit
    for eng, dt, cost in ((a, dt_m, cost_morton), (b, dt_c, cost_clustered)):
        assert _close(dt.cost_before, cost_refit), (dt.cost_before, cost_refit)
        assert _close(dt.cost_after, cost), (dt.cost_after, cost)
        assert _close(eng.fit_cost(), cost), (eng.fit_cost(), cost)
    O, D, _ = _count_rays(b.scene, 51)
    tmax = np.random.RandomState(6).uniform(0.1, 20.0, size=len(O))
    _fit_and_tw_exact(b, O, D, tmax)
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. exactness
def test_touching_rays_before_and_after_a_clustered_rebuild():
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
    rs, _ = _rebuild_clustered(eng)                         # nothing staged: the pose as it stands
    _matches_stats(_tree(eng), rs)
    good = _touching_counts(eng, world, 5)
    assert good == {1: (0, 0), 0: (0, 0)}, f"mismatches after the rebuild: {good}"
    for walk in ("transformed", "transformed_tw"):
        _set_walk(eng, walk)
        assert _same_hits(before[walk], _hits(eng, O, D, tmax)), walk
    eng.close()


def test_near_vertex_rays_at_1e6_before_and_after_a_clustered_rebuild():
    sc, P, F = _teeth_scene((16.0, 0.0, 0.0))
    eng = _engine(sc)
    far = (1.0e6, 1.0e6, 1.0e6)
    eng.set_transform(1, M.translation(*far))
    eng.commit()
    O, D = _near_vertex_rays(P + np.asarray(far), F, 4000, np.random.RandomState(61), 3.0e4)
    tmax = np.full(len(O), 1.0e7)
    before = {}
    for walk in ("transformed", "transformed_tw"):
        _set_walk(eng, walk)
        before[walk] = _hits(eng, O, D, tmax)
    _set_walk(eng, "transformed")
    rs, _ = _rebuild_clustered(eng)
    d = _tree(eng)
    _matches_stats(d, rs)
    assert d["wide_coord"] >= 1.0e6 and d["fit_coord"] >= 1.0e6
    good = _teeth_counts(eng, eng.scene, O, D)
    assert good == {1: (0, 0), 0: (0, 0)}, f"mismatches after the rebuild: {good}"
    for walk in ("transformed", "transformed_tw"):
        _set_walk(eng, walk)
        assert _same_hits(before[walk], _hits(eng, O, D, tmax)), walk
    _set_walk(eng, "transformed")
    _frame(eng)
    eng.close()


def test_equal_t_ties_keep_the_references_winner():
    """test_gpu_rebuild's deliberate ties - two instances of one grid under one transform, with
    different materials, rays through shared vertices and edge midpoints - after a clustered
    rebuild: the winner is the reference's, the same as before the rebuild, and the frame reports
    re-walked rays."""
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
    before = _hits(eng, O, D, tmax)
    rs, _ = _rebuild_clustered(eng)
    _matches_stats(_tree(eng), rs)
    ref = _fit_and_tw_exact(eng, O, D, tmax)
    assert np.isfinite(ref[0][0]).mean() > 0.5
    assert _same_hits(before, _hits(eng, O, D, tmax))
    st = _frame(eng)
    assert st.rewalked > 0, "no tie was handed to the reference-order walk"
    eng.close()


# ---------------------------------------------------------------- 6. determinism
def test_twenty_clustered_rebuilds_and_two_replicas_are_byte_identical():
    sc = small_scene([_spread(k) for k in range(30)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc, devices=[0, 0])
    for k in range(30):
        eng.set_transform(1 + k, _spread(k, seed=3))
    _, dt0 = _rebuild_clustered(eng)
    first = _tree(eng, 0)
    assert W.same_dump(first, _tree(eng, 1)) is None, "the replicas differ"
    for _ in range(20):
        _, dt = _rebuild_clustered(eng)
        assert (dt.iterations, dt.cost_after) == (dt0.iterations, dt0.cost_after)
    d0, d1 = eng.wide_read(0), eng.wide_read(1)
    assert W.same_dump(first, d0) is None, f"a rebuild at one pose changed {W.same_dump(first, d0)}"
    assert W.same_dump(d0, d1) is None, f"the replicas differ in {W.same_dump(d0, d1)}"
    O, D, _ = _count_rays(eng.scene, 31)
    tmax = np.random.RandomState(3).uniform(0.1, 20.0, size=len(O))
    _fit_and_tw_exact(eng, O, D, tmax)
    eng.close()


def test_the_morton_builder_does_not_see_the_previous_tree():
    """Engine A rebuilt with Morton; engine B rebuilt clustered, then with Morton, at the same pose:
    byte-identical."""
    dumps = []
    for first in (None, "clustered"):
        sc = small_scene([_spread(k) for k in range(30)], n=8, base_at=(0.0, 6.0, 0.0))
        eng = _engine(sc)
        for k in range(30):
            eng.set_transform(1 + k, _spread(k, seed=3))
        if first:
            _rebuild_clustered(eng)
            clustered = eng.wide_read()
        _rebuild_morton(eng)
        dumps.append(_tree(eng))
        eng.close()
    assert W.same_dump(dumps[0], dumps[1]) is None, W.same_dump(dumps[0], dumps[1])
    assert W.same_dump(dumps[1], clustered) is not None, "the two builders must differ on this scene"


# ---------------------------------------------------------------- 7. life after a clustered rebuild
def test_clustered_rebuild_move_commit_and_back():
    sc = small_scene([_spread(k) for k in range(40)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc)
    O, D, _ = _count_rays(eng.scene, 21)
    tmax = np.random.RandomState(2).uniform(0.1, 20.0, size=len(O))
    pose_a = {1 + k: _spread(k, seed=1) for k in range(40)}
    pose_b = {1 + k: _spread(k, seed=2) for k in range(40)}
    for i, m in pose_a.items():
        eng.set_transform(i, m)
    rs, _ = _rebuild_clustered(eng)
    at_a = _tree(eng)
    _matches_stats(at_a, rs)
    ref_a = _fit_and_tw_exact(eng, O, D, tmax)
    for i, m in pose_b.items():
        eng.set_transform(i, m)
    assert eng.commit().instances_moved == 40
    zero = eng.last_rebuild_stats()
    assert (zero.rebuilt, zero.reason, zero.pairs, zero.nodes_after, zero.total_ms) == (0, 0, 0, 0, 0.0)
    assert _zero_detail(eng.last_rebuild_detail())
    at_b = _tree(eng)                                         # the new fit_levels are the ones refit
    assert at_b["fit_nodes"] == rs.nodes_after and not np.array_equal(at_a["nodes"], at_b["nodes"])
    assert _close(eng.fit_cost(), _fit_cost(at_b))
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


def test_a_deformable_scene_stages_positions_and_a_transform_and_rebuilds_clustered():
    sc = DS.base_scene("smooth", sizes=(1, 3, 65))
    leaf_of = W.tlas_leaves(sc)
    eng = M.RayTracerEngine(sc, None, deformable=True)
    eng.leaf_of = leaf_of
    assert eng.wide_read()["fit_root"] >= 0
    meshes = [i for i, o in enumerate(eng.scene.objects) if isinstance(o, M.Mesh)]
    big = max(meshes, key=lambda i: len(np.asarray(eng.scene.objects[i].positions).reshape(-1, 3)))
    pos = np.asarray(eng.scene.objects[big].positions, np.float64).reshape(-1, 3)
    new = pos * np.array([1.25, 0.75, 1.5]) + 0.125 * np.sin(3.0 * pos[:, [1, 2, 0]])
    eng.set_positions(big, new)
    m = _mat(eng.scene.objects[big].transform).copy()
    m[:3, 3] += (1.5, -0.5, 0.75)
    eng.set_transform(big, tuple(m.T.reshape(-1)))
    cs = eng.commit(rebuild="clustered")
    rs, _ = _rebuilt(eng, cs)
    assert cs.instances_moved == 1 and eng.last_deform_stats().meshes_deformed == 1
    d = _tree(eng)
    _matches_stats(d, rs)
    rng = np.random.RandomState(8)
    obj = eng.scene.objects[big]
    faces = np.asarray(obj.indices, np.int64).reshape(-1, 3) - (1 if obj.indices_one_based else 0)
    cen = new[faces[rng.choice(len(faces), 400)]].mean(axis=1)
    tgt = cen @ m[:3, :3].T + m[:3, 3]
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


def test_a_refused_commit_leaves_the_tree_the_stats_and_the_detail():
    sc = small_scene([_spread(k) for k in range(12)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc)
    eng.set_transform(3, _spread(3, seed=4))
    rs, dt = _rebuild_clustered(eng)
    kept = eng.wide_read()
    eng.set_transform(2, _m16(np.eye(3), (1.0e31, 0.0, 0.0)))
    with pytest.raises(M.RenderError) as e:
        eng.commit(rebuild="clustered")
    assert e.value.code == A.RT_ERR_INVALID_ARG
    after, after_dt = eng.last_rebuild_stats(), eng.last_rebuild_detail()
    for f, _ in A.rt_rebuild_stats._fields_:
        assert getattr(after, f) == getattr(rs, f), f
    for f, _ in A.rt_rebuild_detail._fields_:
        assert getattr(after_dt, f) == getattr(dt, f), f
    lib = M.load_library()
    io = A.rt_wide_dump()
    assert lib.rt_debug_wide_read(eng._h, 0, io) == 0 and (io.fit_nodes, io.wide_copy) == (kept["fit_nodes"], kept["wide_copy"])
    nodes = np.zeros((int(io.wnodes), 32), np.uint32)
    io.cap_wnodes, io.nodes = io.wnodes, nodes.ctypes.data
    assert lib.rt_debug_wide_read(eng._h, 0, io) == 0
    assert np.array_equal(nodes, kept["nodes"]), "the refused commit touched the node array"
    eng.close()


# ---------------------------------------------------------------- 8. guards and hooks
def test_the_iteration_cap_falls_back_to_the_morton_tree():
    """rebuild_cluster_iter_cap = 1 on a 64-pair scene: one iteration cannot finish, the replica
    builds the Morton tree instead - no error, fell_back = 1, builder = 1, a Morton rebuild's bytes."""
    dumps = []
    for capped in (False, True):
        sc = _one_run_scene(64)
        eng = _engine(sc)
        for k in range(63):
            eng.set_transform(1 + k, _spread(k, seed=1))
        if capped:
            with pytest.raises(M.RenderError):
                eng.set_option("rebuild_cluster_iter_cap", 1)        # a test hook: refused by rt_scene_set_option
            default = eng.get_option("rebuild_cluster_iter_cap")
            with pytest.raises(M.RenderError):
                eng.set_unsafe_option("rebuild_cluster_iter_cap", default + 1)   # it can only be lowered
            eng.set_unsafe_option("rebuild_cluster_iter_cap", 1)
            rs, dt = _rebuilt(eng, eng.commit(rebuild="clustered"), pairs=64, builder=A.RT_BUILDER_MORTON, fell_back=1)
            assert dt.iterations == 1
        else:
            rs, dt = _rebuild_morton(eng, pairs=64)
        d = _tree(eng)
        _matches_stats(d, rs)
        dumps.append(d)
        if capped:
            eng.set_unsafe_option("rebuild_cluster_iter_cap", default)
            _rebuild_clustered(eng, pairs=64)
            _tree(eng)
        eng.close()
    assert W.same_dump(dumps[0], dumps[1]) is None, W.same_dump(dumps[0], dumps[1])


def test_depth_cap_leaves_the_old_tree():
    sc = small_scene([_spread(k) for k in range(20)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = _engine(sc)
    for k in range(20):
        eng.set_transform(1 + k, _spread(k, seed=5))
    eng.commit()
    kept = _tree(eng)
    O, D, _ = _count_rays(eng.scene, 41)
    tmax = np.random.RandomState(4).uniform(0.1, 20.0, size=len(O))
    eng.set_unsafe_option("rebuild_depth_cap", 1)
    cs = eng.commit(rebuild="clustered")
    rs, dt = eng.last_rebuild_stats(), eng.last_rebuild_detail()
    assert (rs.rebuilt, rs.reason, cs.instances_moved) == (0, A.RT_REBUILD_TOO_DEEP, 0)
    assert (rs.nodes_after, rs.depth_after) == (rs.nodes_before, rs.depth_before)
    assert dt.builder == A.RT_BUILDER_NONE and dt.cost_after == dt.cost_before and _close(dt.cost_before, _fit_cost(kept))
    assert W.same_dump(kept, eng.wide_read()) is None, "the old tree must stay byte for byte"
    _fit_and_tw_exact(eng, O, D, tmax)
    eng.set_unsafe_option("rebuild_depth_cap", 42)
    rs, _ = _rebuild_clustered(eng)
    assert rs.depth_after > 1
    _matches_stats(_tree(eng), rs)
    _fit_and_tw_exact(eng, O, D, tmax)
    eng.close()


def test_flags_static_busy_and_one_pair():
    sc = small_scene([posed(0), posed(1)])
    lib = M.load_library()
    static = M.RayTracerEngine(sc, None)
    with pytest.raises(M.RenderError) as e:
        static.commit(rebuild="clustered")
    assert e.value.code == A.RT_ERR_UNSUPPORTED
    with pytest.raises(M.RenderError) as e:
        static.fit_cost()
    assert e.value.code == A.RT_ERR_UNSUPPORTED
    static.close()
    eng = _engine(sc)
    for flags in (2, 4, 16, CLUSTERED | 16):
        assert lib.rt_scene_commit_ex(eng._h, flags, None) == A.RT_ERR_INVALID_ARG, flags
    assert eng.last_rebuild_stats().rebuilt == 0 and _zero_detail(eng.last_rebuild_detail())
    for flags in (CLUSTERED, A.RT_COMMIT_REBUILD_FIT | CLUSTERED):
        assert lib.rt_scene_commit_ex(eng._h, flags, None) == A.RT_OK, flags
        assert eng.last_rebuild_detail().builder == A.RT_BUILDER_CLUSTERED, flags
        _tree(eng)
    kept = eng.wide_read()
    rgb = M.pinned_array((8, 8, 3), np.float64)
    ticket = eng.submit_into(0, 0, 1, rgb, None)
    with pytest.raises(M.RenderError) as e:
        eng.commit(rebuild="clustered")
    assert e.value.code == A.RT_ERR_BUSY
    cost = C.c_double(-1.0)
    assert lib.rt_scene_fit_cost(eng._h, C.byref(cost)) == A.RT_ERR_BUSY
    eng.wait(ticket)
    assert W.same_dump(kept, eng.wide_read()) is None
    assert _close(eng.fit_cost(), _fit_cost(kept))
    eng.close()
    one = _engine(small_scene([], n=6, faces=1, base_at=(0.0, 0.0, 0.0)))
    before = one.wide_read()
    assert before["fit_root"] < 0
    cs = one.commit(rebuild="clustered")
    rs, dt = one.last_rebuild_stats(), one.last_rebuild_detail()
    assert (rs.rebuilt, rs.reason, rs.pairs, cs.instances_moved) == (0, A.RT_REBUILD_NO_TREE, 0, 0)
    assert _zero_detail(dt) and one.fit_cost() == 0.0
    assert W.same_dump(before, one.wide_read()) is None
    one.close()
