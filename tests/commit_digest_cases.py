"""Fixed commit sequences whose device state is frozen as SHA-256 digests
(tests/golden/commit_digests.json, written by tests/golden/make_commit_golden.py from the library of
the commit named there; asserted by tests/test_gpu_commit_digests.py).

Why digests: a rebuilt tree's topology follows from the union of the pair boxes through the Morton
codes, so a wrong union still gives a valid tree with the oracle's hits, and fmin / fmax of -0.0 and
+0.0 depend on the order of a reduction.  The structural and ray tests cannot see either; a byte
comparison with what the earlier library wrote can.

Every case is `case(devices, snap)`: it creates its engine on `devices`, runs its commits and calls
snap(label, eng) where a digest is taken.  What the earlier library cannot tell (statistics, bounds
against a fresh build, a refused commit) is asserted in the case itself."""
import copy
import hashlib
import os
import sys

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_scenes as DS                                                       # noqa: E402
from test_gpu_rebuild import _rebuild                                            # noqa: E402
from test_gpu_refit_edges import _spread                                         # noqa: E402
from test_wide_build import small_scene                                          # noqa: E402

ARRAYS = ("nodes", "lbox", "tbox", "bcoord", "inst_bounds")
SCALARS = ("fit_nodes", "wide_copy")


def digest(d):
    """SHA-256 over the read-back's node bytes, leaf boxes, TLAS leaf boxes, bcoord and instance
    bounds, and the fit_nodes / wide_copy scalars."""
    h = hashlib.sha256()
    for k in ARRAYS:
        h.update(np.ascontiguousarray(d[k]).tobytes())
    h.update(np.array([int(d[k]) for k in SCALARS], np.int64).tobytes())
    return h.hexdigest()


def _instanced(count, devices):
    """`count` instances of the 64-run mesh of test_gpu_rebuild's few-thousand-pairs scene."""
    sc = small_scene([_spread(k) for k in range(count - 1)], n=8, base_at=(0.0, 6.0, 0.0))
    eng = M.RayTracerEngine(sc, devices, dynamic=True)
    pairs = int(eng.wide_read()["pairs"])
    assert pairs == 64 * count
    return sc, eng, pairs


def few_thousand_pairs(devices, snap):
    """60 instances: every instance moved and committed, moved again and committed with a rebuild,
    moved back to the build pose by a plain commit over the rebuilt topology."""
    sc, eng, pairs = _instanced(60, devices)
    home = [o.transform for o in sc.objects]
    for seed, rebuild in ((1, False), (2, True)):
        eng.set_transform(0, M.translation(1.0 * seed, -6.0, 0.5))
        for k in range(59):
            eng.set_transform(1 + k, _spread(k, seed=seed))
        if rebuild:
            _rebuild(eng, pairs=pairs)
        else:
            assert eng.commit().instances_moved == 60
        snap("rebuilt" if rebuild else "moved", eng)
    for k, m in enumerate(home):
        eng.set_transform(k, m)
    assert eng.commit().instances_moved == 60 and eng.last_rebuild_stats().rebuilt == 0
    snap("back", eng)
    eng.close()


def more_than_64_partial_unions(devices, snap):
    """270 instances, 17280 pairs: k_rb_pair_boxes writes 68 partial unions, so the one-wave fold
    takes a second stride."""
    sc, eng, pairs = _instanced(270, devices)
    assert pairs > 64 * 256
    for k in range(0, 269, 3):
        eng.set_transform(1 + k, _spread(k, seed=1))
    _rebuild(eng, pairs=pairs)
    snap("rebuilt", eng)
    eng.close()


def _grid74():
    """A deformable 74 x 74 grid (5476 vertices: 3 * 5476 doubles are 65 blocks of
    k_deform_validate) and an instance of it; the deformed pose has its largest coordinate on the
    last vertex."""
    hp, hf = scenes.heightfield(73, 10.0, 1.0, 4)
    hp = hp.astype(np.float32).astype(np.float64)
    assert len(hp) == 74 * 74 >= 5462 and hf.max() == len(hp) - 1
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [M.Mesh(id=1, material="1", positions=hp, indices=hf.astype(np.int32), indices_one_based=False,
                         shading_mode="flat", transform=M.translation(0.0, 0.0, -12.0)),
                  M.MeshInstance(id=2, base_mesh_id=1, material="1", transform=DS.m16(DS.rotation(np.random.RandomState(3)) * 0.5,
                                                                                      (1.0, 2.0, 3.0)))]
    new = DS.wobble(hp)
    new[-1] = (37.5, -2.25, 40.0)
    assert np.abs(new[:-1]).max() < 40.0
    return sc, new


def large_deformable_mesh(devices, snap):
    sc, new = _grid74()
    eng = M.RayTracerEngine(sc, devices, deformable=True)
    eng.set_positions(0, new)
    assert eng.commit().instances_moved == 0
    ds = eng.last_deform_stats()
    assert (ds.meshes_deformed, ds.triangles, ds.instances_rebounded) == (1, 2 * 73 * 73, 2)
    snap("deformed", eng)
    fresh = M.RayTracerEngine(copy.deepcopy(eng.scene), None)
    for obj in (0, 1):
        got, want = eng.instance_bounds(eng.instance_of(obj)), fresh.instance_bounds(fresh.instance_of(obj))
        assert np.array_equal(np.concatenate(got), np.concatenate(want)), obj
    fresh.close()
    bad = new.copy()
    bad[-1, 2] = np.nan
    eng.set_positions(0, bad, mirror=False)
    last = [eng.last_deform_stats(), eng.last_rebuild_stats(), eng.last_rebuild_detail(), eng.last_visibility_stats()]
    with pytest.raises(M.RenderError) as e:
        eng.commit()
    assert e.value.code == A.RT_ERR_INVALID_ARG
    snap("deformed", eng)                                            # the refused commit changed nothing
    now = [eng.last_deform_stats(), eng.last_rebuild_stats(), eng.last_rebuild_detail(), eng.last_visibility_stats()]
    for a, b in zip(last, now):                                      # ... nor what the last successful one reports
        assert [getattr(a, f) for f, _ in a._fields_] == [getattr(b, f) for f, _ in b._fields_], type(a).__name__
    assert now[0].meshes_deformed == 1
    eng.close()


def deformation_transform_and_rebuild(devices, snap):
    sc, pose, moves = DS.combined_case()
    eng = M.RayTracerEngine(sc, devices, deformable=True)
    for i, (p, n) in pose.items():
        eng.set_positions(i, p, n)
    for obj, m in moves.items():
        eng.set_transform(obj, m)
    cs = eng.commit(rebuild=True)
    rs, ds = eng.last_rebuild_stats(), eng.last_deform_stats()
    assert (cs.instances_moved, rs.rebuilt, ds.meshes_deformed, ds.instances_rebounded) == (2, 1, 1, 2)
    snap("committed", eng)
    eng.close()


CASES = {f.__name__: f for f in (few_thousand_pairs, more_than_64_partial_unions, large_deformable_mesh,
                                 deformation_transform_and_rebuild)}


def run(name, devices):
    """label -> one digest per replica, in the order taken; a label taken twice must repeat itself."""
    out = {}

    def snap(label, eng):
        got = [digest(eng.wide_read(slot)) for slot in range(len(devices))]
        assert out.setdefault(label, got) == got, f"{name}: the state '{label}' changed"

    CASES[name](devices, snap)
    return out
