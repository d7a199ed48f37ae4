"""Dynamic scenes (rtcore.h ABI 5): instances and cameras move between renders and
rt_scene_commit refits every acceleration structure on the device (refit.h) with the reference's
refitTLAS semantics (RTContext.swift:883-927).  Everything is compared with the oracle of the
engine's current scene (oracle.OracleScene(eng.scene)), never with the code under test; instance
bounds are compared with a static engine freshly created at the same pose (the builder's own
loop, scene.cpp:1359-1379)."""
import copy
import dataclasses

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import scenes
import oracle

pytestmark = pytest.mark.gpu

# the walks of instanced scenes (tests/test_gpu_rays.py WALKS)
WALKS = {"transformed": {}, "transformed_tw": {"fit": 0}, "transformed_binary": {"wide": 0},
         "nested": {"unified_transformed": 0}}


def _engine(sc, walk="transformed", dynamic=True, devices=None):
    eng = M.RayTracerEngine(sc, devices, dynamic=dynamic)
    for k, v in WALKS[walk].items():
        eng.set_option(k, v)
    return eng


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _m16(lin, t):
    M4 = np.eye(4)
    M4[:3, :3] = lin
    M4[:3, 3] = t
    return tuple(float(x) for x in M4.T.reshape(-1))


def _mat(m16):
    return np.asarray(m16, dtype=np.float64).reshape(4, 4).T


def _axis_dirs():
    d = []
    for a in range(3):
        for s in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]; v[a] = s; d.append(v)
    for a in range(3):
        for z in (0.0, -0.0):
            v = [0.6, -0.8, 0.3]; v[a] = z
            d.append(list(np.asarray(v) / np.linalg.norm(v)))
    return np.array(d)


def _ray_set(center, radius, n_random, seed):
    rng = np.random.RandomState(seed)
    o = center + rng.uniform(-radius, radius, size=(n_random, 3))
    d = rng.normal(size=(n_random, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ax = _axis_dirs()
    oa = np.repeat(center[None, :] + rng.uniform(-0.3 * radius, 0.3 * radius, size=(len(ax), 3)), 1, axis=0)
    O = np.concatenate([o[: n_random // 2], oa, o[n_random // 2:], oa + 0.25 * radius])
    D = np.concatenate([d[: n_random // 2], ax, d[n_random // 2:], -ax])
    return O, D


_ORACLE = {}


def _oracle_rays(key, sc, O, D, tmax, time=None):
    """The oracle's closest hits and occlusion of (O, D) in scene sc, computed once per key."""
    if key not in _ORACLE:
        osc = oracle.OracleScene(sc)
        _ORACLE[key] = (osc.trace_rays(O, D, None, time), osc.occluded_rays(O, D, tmax, time))
        osc.close()
    return _ORACLE[key]


def _assert_rays(eng, ref, O, D, tmax, time=None):
    (to, po, no, mo), oo = ref
    tg, pg, ng, mg = eng.trace_rays(O, D, None, time)
    hit = np.isfinite(to)
    assert np.array_equal(tg, to), f"t differs on {int((tg != to).sum())} of {len(to)} rays"
    assert np.array_equal(mg, mo)
    assert np.array_equal(pg[hit], po[hit]) and np.array_equal(ng[hit], no[hit])
    og = eng.occluded_rays(O, D, tmax, time)
    assert np.array_equal(og, oo), f"occlusion differs on {int((og != oo).sum())} rays"


def _assert_frame(eng, rgb, rgba, st):
    """The project's standing criteria against the oracle of the engine's current scene."""
    ref, ref8, ost = oracle.OracleScene(eng.scene).render(0, threads=0, rgba=True)
    assert float(np.abs(rgb - ref).max()) <= 1e-5
    assert np.array_equal(rgba, ref8)
    assert (st.primary_rays, st.shadow_rays, st.secondary_rays) == (ost.primary_rays, ost.shadow_rays,
                                                                    ost.secondary_rays)


# ---------------------------------------------------------------- 1. instance bounds
_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1152, 5000)


def _bounds_scene(variant, pose_seed):
    hp, hf = scenes.heightfield(50, 20.0, 2.0, 5)
    hp = hp.astype(np.float32).astype(np.float64)
    if variant == "inexact":
        hp = hp * (1.0 + 2.0 ** -30)                 # no vertex is a float: no CTri, the pbox path
        assert np.any(hp.astype(np.float32).astype(np.float64) != hp)
    rng = np.random.RandomState(pose_seed)
    objs = []

    def pose(flip):
        s = rng.uniform(0.5, 2.0, size=3) * np.array([-1.0 if flip else 1.0, 1.0, 1.0])
        return _m16(_rotation(rng) @ np.diag(s), rng.uniform(-10.0, 10.0, size=3))

    for k, n in enumerate(_SIZES):
        blur = (0.1, 0.2, 0.05) if (variant == "blur" and n == 257) else (0.0, 0.0, 0.0)
        objs.append(M.Mesh(id=100 + k, material="1", positions=hp, indices=hf[:n].astype(np.int32),
                           indices_one_based=False, shading_mode="flat", transform=pose(k % 3 == 1), motion_blur=blur))
    for k, n in enumerate(_SIZES):
        objs.append(M.MeshInstance(id=200 + k, base_mesh_id=100 + k, material="1", transform=pose(k % 4 == 0)))
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = objs
    return sc


@pytest.mark.parametrize("variant", ["exact", "inexact", "blur"])
def test_instance_bounds_equal_the_builders(variant):
    """k_inst_bounds over 1 .. 5000 triangles (below, at and above a wave, a block and the
    grid-stride share) equals the host builder's union loop bit for bit."""
    a, b = _bounds_scene(variant, 1), _bounds_scene(variant, 2)
    dets = [np.linalg.det(_mat(o.transform)[:3, :3]) for o in b.objects]
    assert min(dets) < 0 < max(dets)
    eng = _engine(a)
    ref = _engine(copy.deepcopy(b), dynamic=False)
    for i, o in enumerate(b.objects):
        eng.set_transform(i, o.transform)
    st = eng.commit()
    assert st.instances_moved == len(b.objects)
    for i in range(len(b.objects)):
        k = eng.instance_of(i)
        assert k >= 0 and k == ref.instance_of(i)
        lo, hi = eng.instance_bounds(k)
        rlo, rhi = ref.instance_bounds(k)
        assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi), (variant, i, lo - rlo, hi - rhi)
    eng.close()
    ref.close()


# ---------------------------------------------------------------- 2, 3. moved scenes, all walks
def _transformed_instances():
    sc = scenes.scaled(scenes.scene_c2(inline=True), 8, 8)
    base = sc.objects[0]
    rng = np.random.RandomState(31)
    objs = [base]
    for k in range(5):
        objs.append(M.MeshInstance(id=40 + k, base_mesh_id=base.id, material="1",
                                   transform=_m16(_rotation(rng) * (0.4 + 0.5 * k), rng.uniform(-3.0, 3.0, size=3))))
    sc.objects = objs
    return sc


def _pose_b(sc):
    """object -> matrix: the largest instance far outside the old scene, one rotated and rescaled
    in place, one mirrored; objects 0, 1 and 3 stay."""
    far = _mat(sc.objects[5].transform).copy()
    far[:3, 3] += (40.0, 0.0, 0.0)
    turn = _mat(sc.objects[2].transform).copy()
    turn[:3, :3] = _rotation(np.random.RandomState(77)) * 1.7
    mirror = _mat(sc.objects[4].transform).copy()
    mirror[:3, :3] = mirror[:3, :3] @ np.diag([-1.0, 1.0, 1.0])
    return {5: tuple(far.T.reshape(-1)), 2: tuple(turn.T.reshape(-1)), 4: tuple(mirror.T.reshape(-1))}


def _moved_rays():
    O, D = _ray_set(np.array([0.0, 0.0, 0.0]), 4.0, 3000, 23)
    rng = np.random.RandomState(12)
    Of = np.array([40.0, 0.0, 12.0]) + rng.uniform(-3.0, 3.0, size=(1000, 3))
    Df = np.tile([0.0, 0.0, -1.0], (1000, 1))
    O, D = np.concatenate([O, Of]), np.concatenate([D, Df])
    tmax = np.random.RandomState(6).uniform(0.1, 30.0, size=len(O))
    return O, D, tmax


@pytest.mark.parametrize("walk", list(WALKS))
def test_moved_instances_give_the_reference_hits(walk):
    sc = _transformed_instances()
    eng = _engine(sc, walk)
    old_hi_x = max(eng.instance_bounds(k)[1][0] for k in range(6))
    O, D, tmax = _moved_rays()
    assert O[-1000:, 0].min() > old_hi_x, "the far rays must start outside the pre-move scene"
    for i, m in _pose_b(sc).items():
        eng.set_transform(i, m)
    ref = _oracle_rays("moved_b", eng.scene, O, D, tmax)
    far_hits = int(np.isfinite(ref[0][0][-1000:]).sum())
    assert far_hits >= 100, f"only {far_hits} far rays hit in the oracle: the input is wrong"
    # staged transforms do not affect renders before the commit
    t_before = eng.trace_rays(O[-1000:], D[-1000:])[0]
    assert not np.isfinite(t_before).any()
    st = eng.commit()
    assert st.instances_moved == 3
    _assert_rays(eng, ref, O, D, tmax)
    eng.close()


@pytest.mark.parametrize("walk", ["transformed", "nested"])
def test_commit_is_a_function_of_the_pose(walk):
    sc = _transformed_instances()
    pose_a = {i: tuple(sc.objects[i].transform) for i in (2, 4, 5)}
    O, D, tmax = _moved_rays()
    ref_a = _oracle_rays("moved_a", copy.deepcopy(sc), O, D, tmax)
    eng = _engine(sc, walk)
    for i, m in _pose_b(sc).items():
        eng.set_transform(i, m)
    eng.commit()
    for i, m in pose_a.items():
        eng.set_transform(i, m)
    eng.commit()
    _assert_rays(eng, ref_a, O, D, tmax)
    st = eng.commit()                                   # nothing staged: legal, changes nothing
    assert st.instances_moved == 0
    _assert_rays(eng, ref_a, O, D, tmax)
    eng.close()


# ---------------------------------------------------------------- 4. never moved
def test_a_dynamic_scene_that_never_moved():
    eng = _engine(scenes.scaled(scenes.scene_c2(inline=True), 48, 40))
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)
    _assert_frame(eng, rgb, rgba, st)
    eng.close()


# ---------------------------------------------------------------- 5. frame sequence
def _sequence_scene(variant, w, h):
    hp, hf = scenes.heightfield(16, 12.0, 0.6, 9)
    sv, sf = scenes.icosphere(2)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    ground = M.Mesh(id=1, material="1", positions=f32(hp), indices=hf.astype(np.int32), indices_one_based=False,
                    shading_mode="flat")
    ball = M.Mesh(id=2, material="1", positions=f32(sv), indices=sf.astype(np.int32), indices_one_based=False,
                  shading_mode="smooth", transform=_m16(np.eye(3) * 0.8, (-1.6, 1.3, 0.2)))
    second = M.MeshInstance(id=3, base_mesh_id=2, material="2", transform=_m16(np.eye(3) * 1.1, (1.4, 1.6, -0.4)))
    sc = scenes.scaled(scenes.scene_c2(inline=True), w, h)
    base = sc.materials[0]
    if variant == "mirror":
        two = dataclasses.replace(base, mirror=(0.6, 0.6, 0.6), type="mirror")
    else:
        two = M.Material(ambient=(0.0, 0.0, 0.0), diffuse=(0.05, 0.05, 0.05), specular=(0.5, 0.5, 0.5), phong=60.0,
                         ior=1.5, absorption=(0.02, 0.04, 0.08), type="dielectric")
        sc.area_lights = [M.AreaLight(position=(0.0, 7.0, 1.0), normal=(0.0, -1.0, 0.1), radiance=(300.0, 280.0, 260.0),
                                      size=1.5)]
    sc.materials = [base, two]
    sc.objects = [ground, ball, second]
    sc.point_lights = [M.PointLight((3.0, 6.0, 4.0), (2.0e3, 2.0e3, 2.0e3))]
    sc.max_recursion_depth = 3
    sc.cameras[0].position = (0.0, 3.5, 7.5)
    sc.cameras[0].gaze_point = (0.0, 0.8, 0.0)
    return sc


@pytest.mark.parametrize("variant,w,h", [("mirror", 48, 40), ("glass_area", 24, 16)])
def test_frame_sequence_through_submit_and_wait(variant, w, h):
    eng = _engine(_sequence_scene(variant, w, h))
    rgb = M.pinned_array((h, w, 3), np.float64)
    rgba = M.pinned_array((h, w, 4), np.uint8)
    for f in range(3):
        if f:
            eng.set_transform(2, _m16(np.eye(3) * (1.1 + 0.1 * f), (1.4 - 0.9 * f, 1.6 + 0.3 * f, -0.4 + 0.5 * f)))
            eng.set_camera(0, dataclasses.replace(eng.scene.cameras[0], position=(0.8 * f, 3.5 + 0.4 * f, 7.5 - 0.5 * f),
                                                  gaze_point=(0.2 * f, 0.8, -0.1 * f)))
            assert eng.commit().instances_moved == 1
        rgb[:] = -1.0
        st = eng.wait(eng.submit_into(0, 0, 1, rgb, rgba))
        _assert_frame(eng, rgb, rgba, st)
    eng.close()


# ---------------------------------------------------------------- 6. mixed primitive kinds
@pytest.mark.parametrize("walk", ["transformed", "nested"])
def test_mixed_primitive_kinds_move(walk):
    sc = scenes.scaled(scenes.scene_c2(inline=True), 8, 8)
    base = sc.objects[0]
    sc.objects = [base,
                  M.MeshInstance(id=11, base_mesh_id=base.id, material="1", motion_blur=(0.3, 0.0, 0.1),
                                 transform=(2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 3.0, 0.5, -2.0, 1)),
                  M.Sphere(center=(-2.5, 0.3, 0.5), radius=0.7, material="1"),
                  M.Plane(center=(0.0, -1.5, 0.0), normal=(0.0, 1.0, 0.0), material="1"),
                  M.Triangle(vertices=((-3, -1, -3), (3, -1, -3), (0, 2, -3.5)), material="1")]
    eng = _engine(sc, walk)
    eng.set_transform(2, _m16(np.diag([1.5, 0.8, 1.2]), (1.0, 0.9, 2.0)))
    eng.set_transform(1, _m16(_rotation(np.random.RandomState(3)) * 1.4, (-3.0, 1.0, 1.5)))
    assert eng.commit().instances_moved == 2
    O, D = _ray_set(np.array([0.5, 0.0, 0.0]), 4.0, 3000, 21)
    rng = np.random.RandomState(5)
    tmax, time = rng.uniform(0.1, 6.0, size=len(O)), rng.uniform(0.0, 1.0, size=len(O))
    _assert_rays(eng, _oracle_rays("mixed", eng.scene, O, D, tmax, time), O, D, tmax, time)
    eng.close()


# ---------------------------------------------------------------- 7. two replicas
def test_two_replicas_commit_alike():
    sc = scenes.scaled(_transformed_instances(), 48, 40)
    sc.cameras[0].position = (0.0, 2.0, 14.0)
    eng = _engine(sc, devices=[0, 0])
    moves = _pose_b(sc)
    far = _mat(moves[5]).copy()
    far[:3, 3] -= (36.0, 0.0, 0.0)                       # still in view
    moves[5] = tuple(far.T.reshape(-1))
    for i, m in moves.items():
        eng.set_transform(i, m)
    eng.commit()
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)       # chunks spread over both replicas
    _assert_frame(eng, rgb, rgba, st)
    eng.close()


# ---------------------------------------------------------------- 8. contract
def test_contract():
    assert f"(abi {A.RT_ABI_VERSION},".encode() in M.load_library().rt_version() and A.RT_ABI_VERSION == 5
    sc = scenes.scaled(_transformed_instances(), 48, 40)
    static = _engine(copy.deepcopy(sc), dynamic=False)
    for call in (lambda: static.set_transform(1, M.translation(1.0, 0.0, 0.0)), static.commit):
        with pytest.raises(M.RenderError) as e:
            call()
        assert e.value.code == A.RT_ERR_UNSUPPORTED
    static.close()

    eng = _engine(sc)
    h, w = 40, 48
    rgb = M.pinned_array((h, w, 3), np.float64)
    before = tuple(sc.objects[1].transform)
    nan = list(before); nan[5] = float("nan")
    flat = list(before); flat[0:3] = [0.0, 0.0, 0.0]     # a zero column: determinant 0
    for bad in (nan, flat):
        with pytest.raises(M.RenderError) as e:
            eng.set_transform(1, bad)
        assert e.value.code == A.RT_ERR_INVALID_ARG
    assert tuple(eng.scene.objects[1].transform) == before
    assert eng.commit().instances_moved == 0             # nothing was staged
    ref0, _, _ = oracle.OracleScene(eng.scene).render(0, threads=0, rgba=True)
    eng.wait(eng.submit_into(0, 0, 1, rgb, None))
    assert float(np.abs(rgb - ref0).max()) <= 1e-5

    # a render in flight: commit and set_camera are refused and change nothing
    eng.set_transform(1, M.translation(0.5, 0.25, 0.0))
    cam0 = eng.scene.cameras[0]
    rgb[:] = -1.0
    ticket = eng.submit_into(0, 0, 1, rgb, None)
    for call in (eng.commit, lambda: eng.set_camera(0, dataclasses.replace(cam0, position=(1.0, 1.0, 9.0)))):
        with pytest.raises(M.RenderError) as e:
            call()
        assert e.value.code == A.RT_ERR_BUSY
    assert eng.scene.cameras[0] is cam0
    eng.wait(ticket)
    assert float(np.abs(rgb - ref0).max()) <= 1e-5      # the pre-move frame
    assert eng.commit().instances_moved == 1
    rgb2, rgba2, st = eng.render_rows(0, 0, 1, True)
    _assert_frame(eng, rgb2, rgba2, st)
    eng.close()
