"""Host build of the flattened instance tree (scene.cpp build_fit) over coincident instances, CPU
only.  Five or more pairs with one world-box centroid leave the reference's builder with a leaf it
cannot split (BVH.swift:128-188: no plane separates equal centroids); the four-wide collapse must
still give every pair a slot (or refuse the tree, so the scene keeps tw_walk).  Animations start
like this - instances stacked at one pose - and a refit cannot bring back a pair that was never in
the tree."""
import ctypes as C

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import scenes


def _fit(sc):
    lib = M.load_library()
    pk = sc.to_desc()
    out = (C.c_int64 * 5)()
    rc = lib.rt_debug_fit_build(pk.ptr, out)
    assert rc == 0, lib.rt_last_error()
    return [int(v) for v in out]


def _stacked(n):
    """One small mesh and n instances of it at one pose (a rotation and scale, so the scene is not
    an identity scene); the base mesh's own instance sits elsewhere."""
    hp, hf = scenes.heightfield(6, 4.0, 0.5, 3)
    mesh = M.Mesh(id=1, material="1", positions=hp.astype(np.float32).astype(np.float64), indices=hf.astype(np.int32),
                  indices_one_based=False, shading_mode="flat", transform=M.translation(20.0, 0.0, 0.0))
    c, s = np.cos(0.4), np.sin(0.4)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) * 1.5
    T[:3, 3] = (0.5, -0.25, 1.0)
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [mesh] + [M.MeshInstance(id=10 + k, base_mesh_id=1, material="1", transform=tuple(T.T.reshape(-1)))
                           for k in range(n)]
    return sc


@pytest.mark.parametrize("n", [5, 6, 9])
def test_coincident_instances_keep_every_pair_or_get_no_tree(n):
    pairs, nodes, depth, runs, _ = _fit(_stacked(n))
    assert runs > 0 and runs % (n + 1) == 0
    assert pairs == runs or pairs == 0, f"{runs - pairs} of {runs} (instance, leaf run) pairs are missing from the tree"
    if pairs:
        assert nodes >= (pairs + 3) // 4
        assert 3 * depth + 2 <= 128
