"""How a commit ends when it does not succeed (rtcore.h "how a commit ends").

A commit (1) is done, (2) is refused or runs out of memory before anything changed, (3) commits the
pose but keeps the old flattened instance tree for want of memory, or (4) loses the scene.  Two test
hooks, both pure host-side early returns that launch nothing, reach the last three without making a
real allocation or a real kernel fail: debug_fail_commit_alloc = n makes the n-th device allocation
the next commit attempts report failure; debug_fail_commit_step = k makes it return as for a HIP
error before its step k.

The fixture is tests/visibility_scenes.combined(), step 1: six objects (meshes of 3, 65 and 257
triangles and a MeshInstance of each) on two replicas; one commit hides object 1, moves objects 0 and 5
and deforms mesh 2, whose normals are derived smooth ones here (so the face and vertex normal scratch
is really used).  tests/test_visibility_inputs.py shows its 900 rays free of ties on the CPU.

"State" below is, per replica, the digest of the read-back four-wide trees, leaf boxes and bounds
(commit_digest_cases.digest) and the 900 rays bit for bit against the oracle (the digest does not cover
triangles); the 48 x 40 frame at the project's bar (the rays do not cover normals); instance bounds,
visibility flags and the tree cost; and the four last_* statistics.  Every oracle is built from the
test's own copy of the scene: the engine's mirror follows staging, not commits.

Measured on an MI355X (the sweeps print what they met):
  deforming fixture, cold, two replicas, plain: 13 allocations (two replicas x five deformation arrays,
  three instance-bounds arrays), n = 1 .. 13 all outcome 2.  Rebuilding, Morton and clustered alike: 22,
  n = 1 .. 13 outcome 2, n = 14 .. 22 outcome 3 (the cost scratch, then per replica the live-pair
  buffer, the arena, the nodes and the levels).  Warm: 8, all outcome 3.  Forced rebuild on one
  replica: 3 (arena, nodes, levels), all outcome 3.  One replica, transforms only, rebuilding: 7,
  n = 1 .. 3 outcome 2, n = 4 .. 7 outcome 3.
  Every step k = 1 .. 10 of debug_fail_commit_step loses the scene (outcome 4), the checking steps
  1 - 3 included: a HIP error leaves the device in no known state.
  The library before the fixes, with the hooks alone: n = 6 .. 8 and 14 .. 16 (bounds scratch) came back
  as RT_ERR_DEVICE; n = 9 .. 13 (replica 1's staging) as RT_ERR_OOM with replica 0 deformed, its digest
  changed and the two-replica frame off the oracle's; n = 14 .. 16 with both replicas deformed under the
  old TLAS; n = 17 (the tree-cost scratch) as RT_ERR_DEVICE with the new pose committed; and a refused
  commit zeroed last_deform."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visibility_scenes as V                                                    # noqa: E402
from commit_digest_cases import digest                                           # noqa: E402
from test_gpu_visibility import _assert_frame, _assert_rays, _engine, _ref, _set_hidden   # noqa: E402

pytestmark = pytest.mark.gpu

DEVICES = [0, 0]
ALLOC, STEP = "debug_fail_commit_alloc", "debug_fail_commit_step"
# two replicas x (def_stage, def_part, def_out, def_face, def_vnorm) + replica 0's (moves, bounds_out, bounds_part)
BEFORE_FIRST_WRITE = 2 * 5 + 3
# at least: the cost scratch, the live-pair buffer, the arena, nodes + levels
REBUILD_AT_LEAST = 4


class _Pose:
    """A scene and its hidden objects, for test_gpu_visibility._ref (which asks for visible_scene())."""

    def __init__(self, scene, hidden=frozenset()):
        self.scene, self.hidden = scene, hidden

    def visible_scene(self):
        return engine.visible_subset(self.scene, [i not in self.hidden for i in range(len(self.scene.objects))])


_FIXTURE = {}


def _fixture():
    """scene A (as built), the rays, step 1 and scene B (what step 1 leaves), mesh 2 smooth in both."""
    if not _FIXTURE:
        sc, rays, steps = V.combined()
        a, b = copy.deepcopy(sc), copy.deepcopy(steps[0]["scene"])
        a.objects[2].shading_mode = b.objects[2].shading_mode = "smooth"
        O, D, tmax = rays
        _FIXTURE.update(a=a, b=b, rays=rays, step=steps[0],
                        ref_a=_ref(_Pose(a), ("commit_failures", "a"), O, D, tmax, True),
                        ref_b=_ref(_Pose(b, steps[0]["hidden"]), ("commit_failures", "b"), O, D, tmax, True))
    return _FIXTURE


def _make():
    return _engine(_fixture()["a"], "transformed", DEVICES, deformable=True)


def _stage(eng, st=None):
    st = st or _fixture()["step"]
    for i, f in st["vis"].items():
        eng.set_visible(i, f)
    for i, m in st["moves"].items():
        eng.set_transform(i, m)
    for i, p in st["positions"].items():
        eng.set_positions(i, p)


def _last_stats(eng, timing=True):
    """The four last_* statistics as tuples; without `timing` the measured milliseconds are left out
    (they differ between two engines that did the same)."""
    out = []
    for st in (eng.last_deform_stats(), eng.last_rebuild_stats(), eng.last_rebuild_detail(), eng.last_visibility_stats()):
        out.append(tuple((f, getattr(st, f)) for f, _ in st._fields_ if timing or not f.endswith("_ms")))
    return out


def _digests(eng):
    return [digest(eng.wide_read(slot)) for slot in range(len(eng.devices))]


def _state(eng, timing=True, stats=True):
    """Not before a commit whose allocations are counted: rt_scene_fit_cost allocates the cost scratch,
    which is also replica 0's bounds_part."""
    n = len(eng.scene.objects)
    out = dict(digests=_digests(eng),
               bounds=[np.concatenate(eng.instance_bounds(eng.instance_of(i))).tobytes() for i in range(n)],
               visible=[eng.is_visible(i) for i in range(n)], fit_cost=eng.fit_cost())
    if stats:
        out["stats"] = _last_stats(eng, timing)
    return out


def _assert_pose(eng, ref, rays, frame=True):
    """Rays on every replica and the frame over all of them, on the four-wide and the binary walk."""
    O, D, tmax = rays
    for wide in (1, 0):
        eng.set_option("wide", wide)
        for slot in range(len(eng.devices)):
            _assert_rays(eng, ref, O, D, tmax, slot=slot)
        if frame:
            _assert_frame(eng, ref)
    eng.set_option("wide", 1)


def _commit_code(eng, rebuild):
    try:
        eng.commit(rebuild=rebuild)
        return A.RT_OK
    except M.RenderError as e:
        return e.code


def _pristine(make, ref_a, rays):
    """State A, from an engine that does nothing else."""
    eng = make()
    state = _state(eng, timing=False)
    _assert_pose(eng, ref_a, rays)
    eng.close()
    return state


def _sweep(make, stage, rebuild, ref_a, ref_b, rays, twin, frame=True, warm=False):
    """n = 1, 2, ...: a fresh engine whose commit finds its n-th device allocation failing, until a
    commit meets no failure.  Returns the outcome (2 or 3) of every failing n."""
    outcomes = []
    state_a = twin if warm else _pristine(make, ref_a, rays)
    while True:
        n = len(outcomes) + 1
        assert n < 64, "the sweep does not end"
        eng = make()
        if warm:
            stage(eng)
            eng.commit(rebuild=rebuild)
        before = _digests(eng)
        eng.set_unsafe_option(ALLOC, n)
        stage(eng)
        code = _commit_code(eng, rebuild)
        assert eng.get_option(ALLOC) == 0, "the hook did not clear itself"
        rs = eng.last_rebuild_stats()
        if code == A.RT_OK and rs.reason != A.RT_REBUILD_NO_MEMORY:           # no allocation was the n-th
            assert _state(eng, timing=False) == twin
            eng.close()
            return outcomes
        if code != A.RT_OK:                                                  # outcome 2
            assert code == A.RT_ERR_OOM, f"n = {n}: code {code}"
            outcomes.append(2)
            assert _digests(eng) == before, f"n = {n}: a commit that ran out of memory changed the device"
            assert _state(eng, timing=False) == state_a, f"n = {n}: a commit that ran out of memory changed the scene"
            _assert_pose(eng, ref_a, rays, frame)
            stage(eng)                                                       # what was staged was dropped
            eng.commit(rebuild=rebuild)
            assert _state(eng, timing=False) == twin, f"n = {n}: the commit after it differs from the twin's"
            _assert_pose(eng, ref_b, rays, frame)
        else:                                                                # outcome 3
            outcomes.append(3)
            assert rebuild and (rs.rebuilt, rs.reason) == (0, A.RT_REBUILD_NO_MEMORY), f"n = {n}"
            assert eng.last_rebuild_detail().builder == 0
            _assert_pose(eng, ref_b, rays, frame)
            eng.commit(rebuild=rebuild)                                      # nothing staged: rebuilds the pose as it stands
            assert eng.last_rebuild_stats().rebuilt == 1
            assert _state(eng, stats=False) == {k: v for k, v in twin.items() if k != "stats"}, f"n = {n}"
            _assert_rays(eng, ref_b, *rays)
        eng.close()


def _twin(make, stage, rebuild, ref_b, rays, frame=True, warm=False):
    eng = make()
    for _ in range(2 if warm else 1):
        stage(eng)
        eng.commit(rebuild=rebuild)
    _assert_pose(eng, ref_b, rays, frame)
    state = _state(eng, timing=False)
    eng.close()
    return state


# ---------------------------------------------------------------- 1. the allocation sweep
@pytest.mark.parametrize("rebuild", [False, True, "clustered"])
def test_every_allocation_of_a_commit_may_fail(rebuild):
    f = _fixture()
    twin = _twin(_make, _stage, rebuild, f["ref_b"], f["rays"])
    outcomes = _sweep(_make, _stage, rebuild, f["ref_a"], f["ref_b"], f["rays"], twin)
    print(f"rebuild = {rebuild}: {len(outcomes)} allocations met; outcome 2 for n = "
          f"{[k + 1 for k, o in enumerate(outcomes) if o == 2]}, outcome 3 for n = {[k + 1 for k, o in enumerate(outcomes) if o == 3]}")
    # the loop ran once more than it met failures
    assert len(outcomes) + 1 >= BEFORE_FIRST_WRITE + (REBUILD_AT_LEAST if rebuild else 0)
    assert outcomes[:BEFORE_FIRST_WRITE] == [2] * BEFORE_FIRST_WRITE
    assert outcomes[BEFORE_FIRST_WRITE:] == [3] * (len(outcomes) - BEFORE_FIRST_WRITE)
    if rebuild:
        assert len(outcomes) >= BEFORE_FIRST_WRITE + REBUILD_AT_LEAST
    else:
        assert len(outcomes) == BEFORE_FIRST_WRITE


# ---------------------------------------------------------------- 2. the sweep on a warm engine
def test_a_second_like_commit_allocates_in_the_rebuild_only():
    """The scratch of steps 1 - 9 is reserved once and kept: after one successful commit an identical
    second one allocates only what a rebuild builds beside the old tree - per replica the live-pair
    buffer (an instance is hidden), the arena, the nodes and the levels; the cost scratch is warm."""
    f = _fixture()
    twin = _twin(_make, _stage, True, f["ref_b"], f["rays"], warm=True)
    outcomes = _sweep(_make, _stage, True, f["ref_b"], f["ref_b"], f["rays"], twin, frame=False, warm=True)
    print(f"warm: {len(outcomes)} allocations met, outcomes {outcomes}")
    assert outcomes == [3] * (len(DEVICES) * 4)


# ---------------------------------------------------------------- 3. a forced rebuild without memory
def test_a_forced_rebuild_without_memory_leaves_the_walks_on_the_marker_tree():
    """test_gpu_visibility.test_showing_what_the_tree_lacks_rebuilds_on_its_own's sequence with every
    allocation of the showing commit's rebuild failing in turn."""
    c = V.case("pool")
    O, D, tmax = c.rays
    ref = _ref(_Pose(c.scene), ("pool", 300, "frame"), O, D, tmax, True)
    failed = 0
    while True:
        eng = _engine(c.scene)
        _set_hidden(eng, c.states["live255"], rebuild=True)
        eng.set_unsafe_option(ALLOC, failed + 1)
        cs, vs = _set_hidden(eng, frozenset())                   # a plain commit that shows 45 instances
        rs = eng.last_rebuild_stats()
        if rs.reason != A.RT_REBUILD_NO_MEMORY:
            assert (rs.rebuilt, vs.forced_rebuild, vs.fit_complete) == (1, 1, 1)
            eng.close()
            break
        failed += 1
        assert failed < 32
        assert (rs.rebuilt, vs.forced_rebuild, vs.fit_complete, vs.pairs_in_tree, vs.pairs_visible, vs.shown) == \
            (0, 0, 0, 255, V.POOL, 45)
        _assert_rays(eng, ref, O, D, tmax)                       # option fit is on: the walks must not use the tree
        _assert_frame(eng, ref)
        cs, vs = _set_hidden(eng, frozenset())                   # the next plain commit rebuilds on its own
        assert (eng.last_rebuild_stats().rebuilt, vs.forced_rebuild, vs.fit_complete, vs.pairs_in_tree) == (1, 1, 1, V.POOL)
        _assert_rays(eng, ref, O, D, tmax)
        eng.close()
    print(f"forced rebuild: {failed} allocations failed in turn")
    assert failed >= 3                                           # the arena, the nodes, the levels


# ---------------------------------------------------------------- 4. step failures
def _raises_device(call):
    with pytest.raises(M.RenderError) as e:
        call()
    assert e.value.code == A.RT_ERR_DEVICE, e.value
    assert "commit" in str(e.value) and "lost" in str(e.value)


@pytest.mark.parametrize("k", range(1, 11))
def test_a_device_failure_in_a_commit_loses_the_scene(k):
    """Every k delivers outcome 4, the checking steps 1 - 3 included."""
    f = _fixture()
    O, D, tmax = f["rays"]
    lib = M.load_library()
    eng = _make()
    _stage(eng)
    eng.set_unsafe_option(STEP, k)
    with pytest.raises(M.RenderError) as e:
        eng.commit(rebuild=True)
    assert e.value.code == A.RT_ERR_DEVICE and f"step {k}" in str(e.value)
    h, w = V.FRAME[1], V.FRAME[0]
    rgb, rgba = M.pinned_array((h, w, 3), np.float64), M.pinned_array((h, w, 4), np.uint8)
    rgb[:], rgba[:] = -7.0, 77
    _raises_device(lambda: eng.render_into(0, 0, 1, rgb, rgba))
    _raises_device(lambda: eng.submit_into(0, 0, 1, rgb, rgba))
    assert (rgb == -7.0).all() and (rgba == 77).all()
    _raises_device(lambda: eng.query_closest(O, D))
    _raises_device(lambda: eng.query_occluded(O, D, tmax))
    rays, n, _, keep, _ = engine._query_rays(O, D, tmax, None)
    occ, t = np.full(n, 77, np.uint8), np.full(n, -7.0)
    hb = A.rt_hit_batch()
    hb.t = t.ctypes.data
    for slot in range(len(DEVICES)):
        assert lib.rt_query_occluded(eng.handle, slot, n, C.byref(rays), C.c_void_p(occ.ctypes.data), None, 0, None) == A.RT_ERR_DEVICE
        assert lib.rt_query_closest(eng.handle, slot, n, C.byref(rays), C.byref(hb), None, 0, None) == A.RT_ERR_DEVICE
    assert (occ == 77).all() and (t == -7.0).all() and keep is not None
    for rebuild in (False, True):
        _raises_device(lambda: eng.commit(rebuild=rebuild))
    _raises_device(eng.fit_cost)
    for slot in range(len(DEVICES)):
        _raises_device(lambda: eng.wide_read(slot))
    _last_stats(eng)                                             # the getters still answer
    eng.close()
    fresh = _engine(f["a"], "transformed", [0], deformable=True)  # the process is unharmed
    _assert_frame(fresh, f["ref_a"])
    fresh.close()


# ---------------------------------------------------------------- 5. refusals keep the stats
def test_a_refused_commit_keeps_the_last_successful_commits_stats():
    f = _fixture()
    eng = _make()
    _stage(eng)
    eng.commit(rebuild=True)                                     # deforms, rebuilds, hides
    ds, rs, vs = eng.last_deform_stats(), eng.last_rebuild_stats(), eng.last_visibility_stats()
    assert (ds.meshes_deformed, ds.instances_rebounded, rs.rebuilt, vs.hidden) == (1, 2, 1, 1) and ds.triangles == 257
    before = _state(eng)
    bad = np.asarray(f["step"]["positions"][2], np.float64).copy()
    bad[-1, 2] = np.nan
    eng.set_positions(2, bad, mirror=False)
    with pytest.raises(M.RenderError) as e:
        eng.commit(rebuild=True)
    assert e.value.code == A.RT_ERR_INVALID_ARG
    assert _state(eng) == before, "a commit refused for a NaN position changed the scene or the stats"
    pose = tuple(eng.scene.objects[0].transform)
    eng.set_transform(0, V.DS.m16(np.eye(3), (1.0e31, 0.0, 0.0)))
    with pytest.raises(M.RenderError) as e:
        eng.commit(rebuild=True)
    assert e.value.code == A.RT_ERR_INVALID_ARG
    eng.scene.objects[0].transform = pose                        # the mirror follows staging: put it back
    assert _state(eng) == before, "a commit refused for a transform out of range changed the scene or the stats"
    _assert_pose(eng, f["ref_b"], f["rays"])
    eng.close()


# ---------------------------------------------------------------- 6. one replica, transforms only
def test_the_sweep_on_a_plain_dynamic_scene_on_one_replica():
    """The common path: a dynamic, not deformable scene on one replica and a commit of transforms with
    a rebuild.  Only the three instance-bounds arrays come before the first write; the rebuild adds
    the cost scratch, the arena, the nodes and the levels (every instance is visible: no live-pair
    buffer)."""
    f = _fixture()
    O, D, tmax = f["rays"]
    moves = f["step"]["moves"]
    a = f["a"]
    b = copy.deepcopy(a)
    for i, m in moves.items():
        b.objects[i].transform = m
    ref_a = _ref(_Pose(a), ("commit_failures", "a"), O, D, tmax, True)
    ref_b = _ref(_Pose(b), ("commit_failures", "moved"), O, D, tmax, True)
    make = lambda: _engine(a, "transformed")
    stage = lambda eng: [eng.set_transform(i, m) for i, m in moves.items()]
    twin = _twin(make, stage, True, ref_b, f["rays"])
    outcomes = _sweep(make, stage, True, ref_a, ref_b, f["rays"], twin)
    print(f"one replica, transforms only: {len(outcomes)} allocations met, outcomes {outcomes}")
    assert outcomes == [2] * 3 + [3] * 4


# ---------------------------------------------------------------- 7. the hooks are test hooks
def test_the_hooks_are_refused_by_the_production_entry_point():
    eng = _engine(_fixture()["a"], "transformed")
    for name, value in ((ALLOC, 1), (STEP, 4)):
        with pytest.raises(M.RenderError) as e:
            eng.set_option(name, value)
        assert e.value.code == A.RT_ERR_INVALID_ARG and eng.get_option(name) == 0
        eng.set_unsafe_option(name, value)
        assert eng.get_option(name) == value
        eng.set_unsafe_option(name, 0)
    with pytest.raises(M.RenderError):
        eng.set_unsafe_option(STEP, 11)
    eng.close()
