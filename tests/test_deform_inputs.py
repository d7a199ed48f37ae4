"""Guards the inputs of tests/test_gpu_deform.py, not the code: every deformed pose those tests
compare with the oracle must be free of equal-t ties.  A refit BLAS re-walks ties in the order of
the kept tree, as the reference's own refit would; a fresh oracle build of the deformed scene need
not share that order.  So for each pose the oracle of the scene and the oracle of the same scene
with each mesh's face list reversed (winding kept) must agree bit for bit, and no ray may have a
second triangle within 1e-9 relative of its smallest t.  No GPU."""
import numpy as np
import pytest

import oracle

import deform_scenes as DS


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("variant", DS.VARIANTS)
def test_pose_b_is_free_of_ties(variant):
    sc = DS.base_scene(variant)
    scb = DS.applied(sc, DS.pose_b(sc, with_normals=variant == "supplied_new"))
    O, D, tmax, time = DS.ray_set()
    tm = time if variant == "blur" else None
    fwd, rev = oracle.OracleScene(scb), oracle.OracleScene(DS.reversed_faces(scb))
    try:
        a, b = fwd.trace_rays(O, D, None, tm), rev.trace_rays(O, D, None, tm)
        assert np.isfinite(a[0]).sum() > len(O) // 10, "the ray set must hit the deformed meshes"
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
        hit = np.isfinite(a[0])
        assert np.array_equal(a[1][hit], b[1][hit]) and np.array_equal(a[2][hit], b[2][hit])
        assert np.array_equal(fwd.occluded_rays(O, D, tmax, tm), rev.occluded_rays(O, D, tmax, tm))
        fa, fb = fwd.render(0, threads=0, rgba=True), rev.render(0, threads=0, rgba=True)
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
        assert (fa[0] != np.asarray(sc.background_color)).any(axis=2).mean() > 0.1, "the frame must see the meshes"
    finally:
        fwd.close()
        rev.close()
    if variant not in ("blur", "special"):           # static triangles only: the numpy restatement
        t1, gap = DS.closest_gap(DS.world_triangles(scb), O, D)
        assert np.isfinite(t1).sum() > len(O) // 10
        assert gap.min() > 1e-9, f"a ray has two triangles within {gap.min():.3e} of its closest t"


def _frames_and_rays_agree(scb, rays=None):
    fwd, rev = oracle.OracleScene(scb), oracle.OracleScene(DS.reversed_faces(scb))
    try:
        fa, fb = fwd.render(0, threads=0, rgba=True), rev.render(0, threads=0, rgba=True)
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
        if rays is not None:
            O, D, tmax = rays
            a, b = fwd.trace_rays(O, D), rev.trace_rays(O, D)
            hit = np.isfinite(a[0])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
            assert np.array_equal(a[1][hit], b[1][hit]) and np.array_equal(a[2][hit], b[2][hit])
            assert np.array_equal(fwd.occluded_rays(O, D, tmax), rev.occluded_rays(O, D, tmax))
    finally:
        fwd.close()
        rev.close()


@pytest.mark.parametrize("kind", ["point", "zero_area"])
def test_degenerate_poses_are_free_of_ties(kind):
    sc = DS.base_scene("flat", sizes=(3, 65, 257))
    scb = DS.applied(sc, {2: (DS.degenerate_pose(sc.objects[2], kind), None)})
    O, D, tmax, _ = DS.aimed_ray_set(sc, 1000, seed=11)
    _frames_and_rays_agree(scb, (O, D, tmax))
    _, gap = DS.closest_gap(DS.world_triangles(scb), O, D)
    assert gap.min() > 1e-9


@pytest.mark.parametrize("dielectric", [False, True])
def test_the_wobbled_mirror_mesh_is_free_of_ties(dielectric):
    sc = DS.c2_like(dielectric)
    _frames_and_rays_agree(DS.applied(sc, {0: (DS.wobble(np.asarray(sc.objects[0].positions)), None)}))


def test_the_ply_backed_pose_is_free_of_ties(tmp_path):
    """The PLY-backed mesh of test_gpu_deform at pose B, as the engine's mirror holds it: the PLY's
    faces and normals through the loader's restatement, the staged positions."""
    import myraytracer_amd as M
    sc, pose = DS.ply_case(str(tmp_path))
    m = M.ply_load(sc.objects[1].ply_path)
    o = sc.objects[1]
    o.indices, o.indices_one_based, o.normals, o.ply_path = np.asarray(m["indices"], np.int32).reshape(-1, 3), False, m["normals"], None
    o.positions = m["positions"]
    scb = DS.applied(sc, pose)
    O, D, tmax, _ = DS.aimed_ray_set(scb, 1000, seed=14)
    _frames_and_rays_agree(scb, (O, D, tmax))
    assert DS.closest_gap(DS.world_triangles(scb), O, D)[1].min() > 1e-9


def test_the_combined_and_the_grown_pose_are_free_of_ties():
    """Deformation and motion in one commit (test 7), and the mesh grown to 1e6 (test 8)."""
    sc, pose, moves = DS.combined_case()
    scb = DS.applied(sc, pose)
    for obj, m in moves.items():
        scb.objects[obj].transform = m
    O, D, tmax, _ = DS.aimed_ray_set(scb)
    _frames_and_rays_agree(scb, (O, D, tmax))
    assert DS.closest_gap(DS.world_triangles(scb), O, D)[1].min() > 1e-9
    sc, s = DS.grown_case()
    O, D, tmax, _ = DS.aimed_ray_set(sc, 1500, seed=4, radius=12.0 * s)
    _frames_and_rays_agree(sc, (O, D, tmax * s))
    assert DS.closest_gap(DS.world_triangles(sc), O, D)[1].min() > 1e-9
