"""Ray queries (rt_query_closest / rt_query_occluded): the scene's production walks
on caller-given rays from host arrays and from torch tensors on the device, with full hit records.

The bar is the one the explicit-ray tests hold: t, point, normal and material bit-identical to the
oracle's intersectTLAS, occlusion identical to occludedTLAS, on every walk the options select; the
host path and the device path agree bit for bit, and engine.trace_rays / occluded_rays (the test
hooks, which call the query path) repack the same answer faithfully.  On top of that: the ids and
barycentrics name the triangle that was hit; the device-side reduction of the batch's bounds sizes
the four-wide walk's widening (teeth: wide_delta_scale = 0 mismatches); declared bounds flag
exactly the rays beyond them; shapes, optional outputs, moving and deforming scenes, two replicas,
byte accounting and refusals."""
import itertools

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import scenes
from myraytracer_amd.scene import material_index
import oracle

import deform_scenes as DS
import test_gpu_rays as R
import test_gpu_wide_bound as W

pytestmark = pytest.mark.gpu
ALL = ("t", "uv", "ids", "point", "normal", "flags")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a, n):
    import torch
    if a is None:
        return None
    return torch.as_tensor(np.array(np.broadcast_to(a, (n,) + np.shape(a)[1:]), dtype=np.float64), device="cuda:0")


def _closest_both(eng, O, D, tmin=None, time=None, **kw):
    """The query through host arrays and through device tensors: bit-identical; the host's RayHits."""
    import torch
    n = len(O)
    h = eng.query_closest(O, D, tmin, time, want=ALL, **kw)
    g = eng.query_closest(_dev(O, n), _dev(D, n), _dev(tmin, n), _dev(time, n), want=ALL, **kw)
    torch.cuda.synchronize()
    for f in ALL:
        assert isinstance(getattr(h, f), np.ndarray) and getattr(g, f).is_cuda
        assert _same(getattr(h, f), getattr(g, f).cpu().numpy()), f"host and device paths differ in {f}"
    return h


def _occluded_both(eng, O, D, tmax=None, time=None, **kw):
    import torch
    n = len(O)
    h = eng.query_occluded(O, D, tmax, time, **kw)
    g = eng.query_occluded(_dev(O, n), _dev(D, n), _dev(tmax, n), _dev(time, n), **kw)
    torch.cuda.synchronize()
    assert h.dtype == np.uint8 and _same(h, g.cpu().numpy()), "host and device paths differ"
    return h


def _assert_oracle(h, ref):
    to, po, no, mo = ref
    hit = np.isfinite(to)
    assert _same(h.t, to), f"t differs on {int((_bits(h.t) != _bits(to)).sum())} of {len(to)} rays"
    assert np.array_equal(h.ids[:, 3], mo)
    assert _same(h.point[hit], po[hit]) and _same(h.normal[hit], no[hit])
    assert np.array_equal(h.flags, hit.astype(np.uint8) * A.RT_HIT_VALID)
    miss = ~hit
    assert (h.ids[miss] == -1).all() and (h.ids[hit][:, [0, 2, 3]] >= 0).all()
    assert not h.uv[miss].any() and not h.point[miss].any() and not h.normal[miss].any()
    u, v = h.uv[hit, 0], h.uv[hit, 1]
    assert (u >= 0).all() and (v >= 0).all() and (u <= 1).all() and (v <= 1).all()


def _assert_debug(eng, h, O, D, tmin=None, time=None):
    """rt_debug_trace_rays is a thin caller of the query path: this checks that its repacking (t,
    point, normal, the material column of the ids) is faithful, not two kernels against each
    other.  Parity of the query path itself rests on _assert_oracle."""
    tg, pg, ng, mg = eng.trace_rays(O, D, tmin, time)
    assert _same(h.t, tg) and _same(h.point, pg) and _same(h.normal, ng) and np.array_equal(h.ids[:, 3], mg)


_CACHE = {}


def _case(name):
    """(scene, O, D, tlimit for closest, time, tmax) and the oracle's answers, computed once."""
    if name in _CACHE:
        return _CACHE[name]
    tmin = time = None
    if name == "c2":
        sc = scenes.scaled(scenes.scene_c2(inline=True), 8, 8)
        O, D = R._ray_set(np.array([0.0, 0.0, 0.0]), 2.5, 2000, 7)
        tmax = np.random.RandomState(3).uniform(0.05, 4.0, size=len(O))
    elif name == "grid":
        hp, hf = scenes.heightfield(64, 20.0, 2.0, 5)
        hp32 = hp.astype(np.float32).astype(np.float64)
        sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
        sc.objects = [M.Mesh(id=1, material="1", positions=hp32, indices=hf.astype(np.int32), indices_one_based=False,
                             shading_mode="flat")]
        rng = np.random.RandomState(11)
        verts = hp32[rng.choice(len(hp32), 200, replace=False)]
        tri = hf[rng.choice(len(hf), 200, replace=False)]
        a, b, c = hp32[tri[:, 0]], hp32[tri[:, 1]], hp32[tri[:, 2]]
        pts = np.concatenate([verts, 0.5 * (a + b), 0.5 * (b + c), (a + b + c) / 3.0])
        Dt = np.array([0.3, -1.0, 0.2]) / np.linalg.norm([0.3, -1.0, 0.2])
        O = np.concatenate([pts + np.array([0.0, 10.0, 0.0]), pts - 10.0 * Dt])
        D = np.concatenate([np.tile([0.0, -1.0, 0.0], (len(pts), 1)), np.tile(Dt, (len(pts), 1))])
        tmax = np.full(len(O), 9.999)
    elif name == "instances":
        sc = R._transformed_instances()
        O, D = R._ray_set(np.array([0.0, 0.0, 0.0]), 4.0, 2000, 23)
        tmax = np.random.RandomState(6).uniform(0.1, 8.0, size=len(O))
    else:                                                  # spheres, planes, a triangle, motion blur
        sc = scenes.scaled(scenes.scene_c2(inline=True), 8, 8)
        base = sc.objects[0]
        base.motion_blur = (0.0, 0.2, 0.0)
        sc.objects = [base,
                      M.MeshInstance(id=11, base_mesh_id=base.id, material="1", motion_blur=(0.3, 0.0, 0.0),
                                     transform=(2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 3.0, 0.5, -2.0, 1)),
                      M.Sphere(center=(-2.5, 0.3, 0.5), radius=0.7, material="1"),
                      M.Plane(center=(0.0, -1.5, 0.0), normal=(0.0, 1.0, 0.0), material="1"),
                      M.Triangle(vertices=((-3, -1, -3), (3, -1, -3), (0, 2, -3.5)), material="1")]
        O, D = R._ray_set(np.array([0.5, 0.0, 0.0]), 4.0, 2000, 21)
        rng = np.random.RandomState(2)
        tmin, time = rng.uniform(0.0, 0.5, size=len(O)), rng.uniform(0, 1, size=len(O))
        tmax = np.random.RandomState(5).uniform(0.1, 6.0, size=len(O))
    orc = oracle.OracleScene(sc)
    ref = orc.trace_rays(O, D, tmin, time)
    occ = orc.occluded_rays(O, D, tmax, time)
    _CACHE[name] = (sc, O, D, tmin, time, tmax, ref, occ)
    return _CACHE[name]


PARITY = [("c2", "wide"), ("c2", "unified"), ("c2", "general"), ("grid", "wide"), ("grid", "unified"),
          ("instances", "transformed"), ("instances", "transformed_tw"), ("instances", "transformed_binary"),
          ("instances", "nested"), ("special", "transformed"), ("special", "nested")]
WALK_ID = {"wide": 1, "unified": 1, "general": 0, "transformed": 3, "transformed_tw": 2, "transformed_binary": 2,
           "nested": 0}


@pytest.mark.parametrize("case,walk", PARITY)
def test_parity_with_the_oracle(case, walk):
    sc, O, D, tmin, time, tmax, ref, occ = _case(case)
    eng = R._engine(sc, walk)
    h = _closest_both(eng, O, D, tmin, time)
    st = eng.last_query_stats()
    _assert_oracle(h, ref)
    _assert_debug(eng, h, O, D, tmin, time)
    hit = np.isfinite(ref[0])
    assert 0.05 < hit.mean() < 0.98
    if case == "special":                                  # the general / unified transformed walk (no four-wide tree)
        assert st.walk == (2 if walk == "transformed" else 0)
    else:
        assert st.walk == WALK_ID[walk]
    assert (st.rays, st.hits, st.out_of_bounds, st.non_finite, st.reduced) == (len(O), int(hit.sum()), 0, 0, 1)
    g = _occluded_both(eng, O, D, tmax, time)
    assert np.array_equal(g.astype(bool), occ) and g.max() <= 1
    assert np.array_equal(eng.occluded_rays(O, D, tmax, time), occ)
    assert eng.last_query_stats().hits == int(occ.sum())
    if case == "special":                                  # spheres and planes: no face, no barycentrics
        kinds = np.array([type(o).__name__ for o in sc.objects])[h.ids[hit, 0]]
        sp = np.isin(kinds, ("Sphere", "Plane"))
        assert sp.any() and (h.ids[hit][sp, 1] == -1).all() and not h.uv[hit][sp].any()
        assert (h.ids[hit][kinds == "Triangle", 1] == 0).all() and (kinds == "MeshInstance").any()
    eng.close()


def _mesh_faces(obj):
    pos = np.asarray(obj.positions, np.float64)
    return pos[np.asarray(obj.indices, np.int64).reshape(-1, 3) - (1 if obj.indices_one_based else 0)]


def test_ids_and_barycentrics_on_identity_scenes():
    """oracle.intersect_triangle on the named face's vertices with the world ray gives the same t
    bit for bit; each object has its own material, so ids[3] = the oracle's material pins ids[0]."""
    hp, hf = scenes.heightfield(24, 8.0, 1.0, 3)
    hp32 = hp.astype(np.float32).astype(np.float64)
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.materials = [sc.materials[0]] * 3
    sc.objects = [M.Mesh(id=k + 1, material=str(k + 1), positions=hp32 * (1.0 + 0.5 * k) + np.array([0.0, 1.5 * k, 0.0]),
                         indices=hf[::k + 1].astype(np.int32), indices_one_based=False,
                         shading_mode="smooth" if k == 1 else "flat") for k in range(3)]
    rng = np.random.RandomState(4)
    D = rng.normal(size=(1500, 3)) * np.array([0.4, 1.0, 0.4]) - np.array([0.0, 2.0, 0.0])
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    O = rng.uniform(hp32.min(0), hp32.max(0), size=(1500, 3)) * 1.5 + np.array([0.0, 1.5, 0.0]) - 12.0 * D
    ref = oracle.OracleScene(sc).trace_rays(O, D)
    eng = M.RayTracerEngine(sc)
    h = _closest_both(eng, O, D)
    eng.close()
    _assert_oracle(h, ref)
    hit = np.flatnonzero(np.isfinite(ref[0]))
    assert len(hit) > 300
    obj_mat = np.array([material_index(o.material) for o in sc.objects])
    assert len(set(obj_mat)) == 3 and len(set(h.ids[hit, 0])) == 3
    assert np.array_equal(obj_mat[h.ids[hit, 0]], ref[3][hit])
    faces = [_mesh_faces(o) for o in sc.objects]
    for i in hit[:400]:
        f = faces[h.ids[i, 0]][h.ids[i, 1]]
        t, _, _ = oracle.intersect_triangle(f[0], f[1], f[2], O[i], D[i], 0.0, sc.intersection_test_epsilon)
        assert np.float64(t).view(np.uint64) == h.t[i].view(np.uint64), (i, t, h.t[i])
    assert (h.uv[hit].sum(1) <= 1.0).all()


def test_the_twin_meshes_name_the_object_the_oracle_keeps():
    sc, hp = R._twin_meshes()
    rng = np.random.RandomState(4)
    D = rng.normal(size=(1500, 3)) * np.array([0.4, 1.0, 0.4]) - np.array([0.0, 2.0, 0.0])
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    O = rng.uniform(hp.min(0), hp.max(0), size=(1500, 3)) - 12.0 * D
    ref = oracle.OracleScene(sc).trace_rays(O, D)
    hit = np.isfinite(ref[0])
    obj_mat = np.array([material_index(o.material) for o in sc.objects])
    assert obj_mat[0] != obj_mat[1] and hit.mean() > 0.5
    for walk in ("wide", "unified"):
        eng = R._engine(sc, walk)
        h = _closest_both(eng, O, D)
        eng.close()
        _assert_oracle(h, ref)
        assert np.array_equal(obj_mat[h.ids[hit, 0]], ref[3][hit])
        # the twins hold the same faces in the same order: the face is the same whichever is kept
        f = _mesh_faces(sc.objects[0])[h.ids[hit, 1]]
        w = 1.0 - h.uv[hit, 0] - h.uv[hit, 1]
        p = w[:, None] * f[:, 0] + h.uv[hit, :1] * f[:, 1] + h.uv[hit, 1:] * f[:, 2]
        assert np.abs(p - h.point[hit]).max() <= 1e-9 * np.abs(hp).max()


def test_transformed_instances_name_the_face_that_was_hit():
    """The world point lies on the named face mapped through the named object's localToWorld, to
    1e-9 x the scene's largest coordinate: FP64 rounding (1e-16) times the condition bound 2^12 of
    kFitKappa leaves five orders to spare, far below the mesh's triangle size."""
    sc, O, D, tmin, time, tmax, ref, occ = _case("instances")
    eng = R._engine(sc, "transformed")
    h = eng.query_closest(O, D, want=ALL)
    hit = np.flatnonzero(np.isfinite(ref[0]))
    for oi in set(h.ids[hit, 0]):
        assert eng.instance_of(int(oi)) in set(h.ids[hit][h.ids[hit, 0] == oi, 2])
    eng.close()
    faces = _mesh_faces(sc.objects[0])
    assert len(set(h.ids[hit, 0])) >= 4
    big = 0.0
    worst = 0.0
    for i in hit:
        m = np.asarray(sc.objects[h.ids[i, 0]].transform, np.float64).reshape(4, 4).T
        f = faces[h.ids[i, 1]] @ m[:3, :3].T + m[:3, 3]
        u, v = h.uv[i]
        p = (1.0 - u - v) * f[0] + u * f[1] + v * f[2]
        big = max(big, np.abs(f).max(), np.abs(O[i]).max())
        worst = max(worst, np.abs(p - h.point[i]).max())
    assert worst <= 1e-9 * big, (worst, big)


# ---------------------------------------------------------------- the device-side bounds have teeth
def _mismatch(h, ref):
    to, po, no, mo = ref
    bad = (_bits(h.t) != _bits(to)) | (h.ids[:, 3] != mo)
    hit = np.isfinite(to) & np.isfinite(h.t)
    return bad | (hit & ((h.point != po).any(1) | (h.normal != no).any(1)))


def _bounds_of(sc, O, D, slack=1.0):
    """Correct declared bounds of a batch (a generous scene centre: the box of the mesh vertices)."""
    P = np.concatenate([np.asarray(o.positions) for o in sc.objects if isinstance(o, M.Mesh)])
    c = 0.5 * (P.min(0) + P.max(0))
    return (float(np.linalg.norm(O - c, axis=1).max() * 1.001 + np.abs(P - c).max()) * slack,
            float(np.abs(O).max()) * slack, float(np.linalg.norm(D, axis=1).max() * 1.001) * slack)


def test_the_reduced_bounds_size_the_widening():
    """The near-vertex rays at 1e6 and the exactly touching rays (tests/test_gpu_wide_bound.py) through
    the query path: bit-equal to the oracle with the bounds reduced on the device and with correct
    declared bounds; with the widening switched off (wide_delta_scale = 0) they mismatch, so the
    reduction is what carries the exactness, not slack."""
    import torch
    sc, scale, off = W._far_c2("1e6")
    mesh = sc.objects[0]
    Ov, Dv = W._near_vertex_rays(np.asarray(mesh.positions), np.asarray(mesh.indices), 12000, np.random.RandomState(61),
                                 3.0 * scale)
    V, Fc, corners = W._touching_grid((1048576.0, -524288.0, 786432.0))
    tsc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    tsc.objects = [M.Mesh(id=1, material="1", positions=V, indices=Fc, indices_one_based=False, shading_mode="flat")]
    Ot, Dt, t0 = W._touching_rays(corners, 4.0, np.random.RandomState(5), 6000)
    for s, O, D, tmax in ((sc, Ov, Dv, None), (tsc, Ot, Dt, t0 * (1 + 2.0 ** -40))):
        orc = oracle.OracleScene(s)
        ref = orc.trace_rays(O, D)
        eng = M.RayTracerEngine(s)
        assert eng.get_option("wide") == 1
        h = _closest_both(eng, O, D)
        st = eng.last_query_stats()
        assert st.walk == 1 and st.reduced == 1
        # the reduction returns the batch's own maxima, exactly
        assert st.bounds.origin_coord == np.abs(O).max()
        assert abs(st.bounds.dir_norm - np.linalg.norm(D, axis=1).max()) <= 1e-15 * st.bounds.dir_norm
        assert not _mismatch(h, ref).any()
        b = _bounds_of(s, O, D)
        hd = _closest_both(eng, O, D, bounds=b)
        assert eng.last_query_stats().reduced == 0 and not _mismatch(hd, ref).any() and (hd.flags <= 1).all()
        if tmax is not None:
            occ = orc.occluded_rays(O, D, tmax)
            assert np.array_equal(_occluded_both(eng, O, D, tmax).astype(bool), occ)
            assert np.array_equal(_occluded_both(eng, O, D, tmax, bounds=b).astype(bool), occ)
        eng.set_unsafe_option("wide_delta_scale", 0)
        bad = _mismatch(eng.query_closest(O, D, want=ALL), ref)
        print(f"no widening: {int(bad.sum())} of {len(O)} closest hits differ")
        assert bad.any(), "no mismatch without the widening: the set does not reach the bound"
        eng.close()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- declared bounds and non-finite rays
def test_declared_bounds_flag_exactly_the_rays_beyond_them():
    sc, O, D, tmin, time, tmax, ref, occ = _case("c2")
    O, D = O.copy(), D.copy()
    n = len(O)
    rng = np.random.RandomState(12)
    pick = rng.choice(n, 90, replace=False)
    far, coord, long_ = pick[:30], pick[30:60], pick[60:]
    O[far] = np.array([3.9, 3.9, -3.9]) * rng.choice([-1.0, 1.0], size=(30, 1))   # coord 3.9 <= 4, reach 6.7 > 5.5
    O[coord] = 0.0
    O[coord, rng.randint(3, size=30)] = 4.5 * rng.choice([-1.0, 1.0], size=30)     # coord 4.5 > 4, reach ~4.5 <= 5.5
    D[long_] *= 2.0                                                                # |d| = 2 > 1.5
    out = np.zeros(n, bool)
    out[pick] = True
    declared = (5.5, 4.0, 1.5)
    want = oracle.OracleScene(sc).trace_rays(O, D)
    eng = M.RayTracerEngine(sc)
    h = _closest_both(eng, O, D, bounds=declared)
    st = eng.last_query_stats()
    assert np.array_equal(h.flags & A.RT_HIT_OUT_OF_BOUNDS != 0, out), "the flagged rays are not the rays beyond the bounds"
    assert not (h.flags & A.RT_HIT_NON_FINITE).any()
    assert (st.rays, st.out_of_bounds, st.non_finite, st.reduced) == (n, 90, 0, 0)
    assert tuple(getattr(st.bounds, k) for k in ("origin_reach", "origin_coord", "dir_norm")) == declared
    assert np.isinf(h.t[out]).all() and (h.ids[out] == -1).all() and (h.flags[out] == A.RT_HIT_OUT_OF_BOUNDS).all()
    ok = ~out
    assert _same(h.t[ok], want[0][ok]) and np.array_equal(h.ids[ok, 3], want[3][ok])
    hit = ok & np.isfinite(want[0])
    assert _same(h.point[hit], want[1][hit]) and _same(h.normal[hit], want[2][hit]) and st.hits == int(hit.sum())
    g = _occluded_both(eng, O, D, tmax, bounds=declared)
    assert (g[out] == 2).all() and np.array_equal(g[ok] == 1, oracle.OracleScene(sc).occluded_rays(O, D, tmax)[ok])
    assert eng.last_query_stats().out_of_bounds == 90
    eng.close()


def test_non_finite_rays_are_flagged_and_do_not_touch_the_others():
    sc, scale, off = W._far_c2("1e5")
    rng = np.random.RandomState(9)
    n = 3000
    O = off + rng.uniform(-3.0, 3.0, size=(n, 3)) * scale
    D = rng.normal(size=(n, 3))
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    bad = rng.choice(n, 40, replace=False)
    O[bad[:10], 1] = np.nan
    O[bad[10:20], 0] = np.inf
    D[bad[20:30], 2] = -np.inf
    D[bad[30:], 0] = np.nan
    ok = np.ones(n, bool)
    ok[bad] = False
    eng = M.RayTracerEngine(sc)
    h = _closest_both(eng, O, D)
    st = eng.last_query_stats()
    clean = eng.query_closest(O[ok], D[ok], want=ALL)
    st_clean = eng.last_query_stats()
    assert (st.non_finite, st.out_of_bounds, st.hits) == (40, 0, st_clean.hits)
    # one bad ray does not blow up the widening of the others: the same bounds, the same answers
    assert tuple(getattr(st.bounds, k) for k in ("origin_reach", "origin_coord", "dir_norm")) == \
        tuple(getattr(st_clean.bounds, k) for k in ("origin_reach", "origin_coord", "dir_norm"))
    assert np.isfinite(st.bounds.origin_coord) and st.walk == 1
    assert (h.flags[bad] == A.RT_HIT_NON_FINITE).all() and np.isinf(h.t[bad]).all() and (h.ids[bad] == -1).all()
    for f in ALL:
        assert _same(getattr(h, f)[ok], getattr(clean, f)), f
    assert not _mismatch(clean, oracle.OracleScene(sc).trace_rays(O[ok], D[ok])).any()
    g = _occluded_both(eng, O, D)
    assert (g[bad] == 2).all() and (g[ok] <= 1).all()
    eng.close()


# ---------------------------------------------------------------- shapes and seams
def test_batch_seams_and_optional_outputs():
    sc, O, D, tmin, time, tmax, ref, occ = _case("special")
    O, D, tmin, time, tmax = O[:1000], D[:1000], tmin[:1000], time[:1000], tmax[:1000]
    eng = R._engine(sc, "transformed")
    full = eng.query_closest(O, D, tmin, time, want=ALL)
    assert eng.last_query_stats().launches == 1
    _assert_oracle(full, tuple(a[:1000] for a in ref))
    occ_full = eng.query_occluded(O, D, tmax, time)
    eng.set_option("query_batch", 192)
    for n in (0, 1, 63, 64, 65, 1000):
        h = _closest_both(eng, O[:n], D[:n], tmin[:n], time[:n])
        assert eng.last_query_stats().launches == (n + 191) // 192
        for f in ALL:
            assert _same(getattr(h, f), getattr(full, f)[:n]), (n, f)
        assert _same(_occluded_both(eng, O[:n], D[:n], tmax[:n], time[:n]), occ_full[:n]), n
    assert eng.last_query_stats().rays == 1000
    import torch
    n = 200                                                # two launches of 192 and 8: the device path offsets its pointers
    dev_in = [_dev(a[:n], n) for a in (O, D, tmin, time)]
    for drop in itertools.combinations(ALL, 2):
        want = tuple(f for f in ALL if f not in drop)
        h = eng.query_closest(O[:n], D[:n], tmin[:n], time[:n], want=want)
        g = eng.query_closest(*dev_in, want=want)
        torch.cuda.synchronize()
        for f in ALL:
            if f in drop:
                assert getattr(h, f) is None and getattr(g, f) is None
            else:
                assert _same(getattr(h, f), getattr(full, f)[:n]), (drop, f)
                assert _same(getattr(g, f).cpu().numpy(), getattr(full, f)[:n]), (drop, f, "device")
    eng.close()


def test_identity_scene_seams():
    """Launch seams on the four-wide identity walk: 2,024 rays in launches of 640."""
    sc, O, D, tmin, time, tmax, ref, occ = _case("c2")
    eng = M.RayTracerEngine(sc)
    eng.set_option("query_batch", 640)
    h = _closest_both(eng, O, D)
    assert eng.last_query_stats().launches == (len(O) + 639) // 640 > 1
    _assert_oracle(h, ref)
    assert np.array_equal(_occluded_both(eng, O, D, tmax).astype(bool), occ)
    eng.close()


# ---------------------------------------------------------------- moving and deforming scenes
def _answers(eng, O, D, tmax, time):
    h = _closest_both(eng, O, D, None, time)
    return h, _occluded_both(eng, O, D, tmax, time)


def _tie_free(sc, O, D):
    """What tests/test_deform_inputs.py shows of a pose: no ray has two triangles within 1e-9 of its
    closest t (a refit keeps the leaf order of the build, the oracle rebuilds: ties could differ)."""
    return DS.closest_gap(DS.world_triangles(sc), O, D)[1].min() > 1e-9


def test_queries_follow_commits_and_return():
    sc, pose, moves = DS.combined_case()
    target = DS.applied(sc, pose)
    for obj, m in moves.items():
        target.objects[obj].transform = m
    O, D, tmax, time = DS.aimed_ray_set(target)            # the rays test_deform_inputs shows tie-free there
    eng = M.RayTracerEngine(sc, deformable=True)
    first, first_occ = _answers(eng, O, D, tmax, time)
    _assert_oracle(first, oracle.OracleScene(sc).trace_rays(O, D, None, time))
    start_pos = {i: np.asarray(sc.objects[i].positions, np.float64).copy() for i in pose}
    start_m = {obj: tuple(sc.objects[obj].transform) for obj in moves}
    for obj, m in moves.items():                           # set_transform + commit
        eng.set_transform(obj, m)
    eng.commit()
    assert _tie_free(eng.scene, O, D)
    orc = oracle.OracleScene(eng.scene)
    moved, moved_occ = _answers(eng, O, D, tmax, time)
    _assert_oracle(moved, orc.trace_rays(O, D, None, time))
    assert np.array_equal(moved_occ.astype(bool), orc.occluded_rays(O, D, tmax, time))
    assert not _same(moved.t, first.t)
    for i, (p, nrm) in pose.items():                       # set_positions + commit: the combined pose
        eng.set_positions(i, p, nrm)
    eng.commit()
    assert _tie_free(eng.scene, O, D)
    orc = oracle.OracleScene(eng.scene)
    bent, bent_occ = _answers(eng, O, D, tmax, time)
    _assert_oracle(bent, orc.trace_rays(O, D, None, time))
    assert np.array_equal(bent_occ.astype(bool), orc.occluded_rays(O, D, tmax, time))
    assert np.isfinite(bent.t).mean() > 0.3 and not _same(bent.t, moved.t)
    for i, p in start_pos.items():                         # back at the build pose: the first answer
        eng.set_positions(i, p)
    for obj, m in start_m.items():
        eng.set_transform(obj, m)
    eng.commit()
    back, back_occ = _answers(eng, O, D, tmax, time)
    for f in ALL:
        assert _same(getattr(back, f), getattr(first, f)), f
    assert _same(back_occ, first_occ)
    eng.close()


def test_two_replicas_answer_alike():
    sc, O, D, tmin, time, tmax, ref, occ = _case("instances")
    eng = M.RayTracerEngine(sc, devices=[0, 0])
    a = eng.query_closest(O, D, want=ALL, slot=0)
    b = eng.query_closest(O, D, want=ALL, slot=1)
    for f in ALL:
        assert _same(getattr(a, f), getattr(b, f)), f
    _assert_oracle(b, ref)
    assert _same(eng.query_occluded(O, D, tmax, slot=0), eng.query_occluded(O, D, tmax, slot=1))
    assert eng.last_query_stats(1).rays == len(O)
    eng.close()


# ---------------------------------------------------------------- byte accounting and refusals
def test_byte_accounting():
    sc, O, D, tmin, time, tmax, ref, occ = _case("instances")
    tab = M.engine.query_tables(sc)
    eng = M.RayTracerEngine(sc)
    i0 = eng.info()
    eng.query_closest(O[:100], D[:100], want=("t", "uv", "point", "normal", "flags"))
    eng.query_occluded(O[:100], D[:100])
    i1 = eng.info()
    assert i1.device_bytes == i0.device_bytes, "a scene that never asked for ids reports the same device_bytes"
    assert i1.scratch_bytes > i0.scratch_bytes
    eng.query_closest(O[:100], D[:100], want=ALL)
    eng.query_closest(O[:50], D[:50], want=("t",))
    i2 = eng.info()
    assert i2.scratch_bytes == i1.scratch_bytes, "scratch grows with n only"
    assert i2.device_bytes - i1.device_bytes == 4 * len(tab["face"]) + 4 * len(tab["inst_object"])
    eng.query_closest(O, D, want=ALL)
    i3 = eng.info()
    assert i3.scratch_bytes > i2.scratch_bytes and i3.device_bytes == i2.device_bytes
    eng.query_closest(O, D, want=ALL)
    eng.query_occluded(O, D, tmax)
    i4 = eng.info()
    assert (i4.scratch_bytes, i4.device_bytes) == (i3.scratch_bytes, i3.device_bytes)
    eng.close()


def test_refusals_leave_the_outputs_untouched():
    import ctypes as C
    import torch
    sc, O, D, tmin, time, tmax, ref, occ = _case("c2")
    n = 64
    O, D = np.ascontiguousarray(O[:n]), np.ascontiguousarray(D[:n])
    eng = M.RayTracerEngine(sc)
    lib = M.load_library()
    t = np.full(n, 7.0)
    ids = np.full((n, 4), 7, np.int32)
    out = np.full(n, 7, np.uint8)
    p = lambda a: a.ctypes.data
    rays = A.rt_ray_batch(p(O), p(D), None, None)
    hits = A.rt_hit_batch(p(t), None, p(ids), None, None, None)
    no_o, no_d = A.rt_ray_batch(None, p(D), None, None), A.rt_ray_batch(p(O), None, None, None)
    B = A.rt_query_bounds

    def closest(slot=0, count=n, r=rays, b=None, flags=0):
        return lib.rt_query_closest(eng.handle, slot, count, C.byref(r), C.byref(hits), b, flags, None)

    def occluded(slot=0, count=n, r=rays, b=None, flags=0):
        return lib.rt_query_occluded(eng.handle, slot, count, C.byref(r), p(out), b, flags, None)

    for call in (closest, occluded):
        assert call(slot=1) == A.RT_ERR_INVALID_ARG and call(slot=-1) == A.RT_ERR_INVALID_ARG
        assert call(count=-1) == A.RT_ERR_INVALID_ARG
        assert call(r=no_o) == A.RT_ERR_INVALID_ARG and call(r=no_d) == A.RT_ERR_INVALID_ARG
        for b in (B(-1.0, 1.0, 1.0), B(1.0, np.nan, 1.0), B(1.0, 1.0, np.inf)):
            assert call(b=C.byref(b)) == A.RT_ERR_INVALID_ARG
        assert call(flags=64) == A.RT_ERR_INVALID_ARG
        assert call(flags=A.RT_QUERY_DEVICE) == A.RT_ERR_UNSUPPORTED     # host pointers are not device pointers
    assert lib.rt_query_occluded(eng.handle, 0, n, C.byref(rays), None, None, 0, None) == A.RT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (t == 7.0).all() and (ids == 7).all() and (out == 7).all()
    assert closest() == A.RT_OK and occluded() == A.RT_OK and np.isfinite(t).any() and (out <= 1).all()
    with pytest.raises(ValueError):
        eng.query_closest(O, D, want=("t", "colour"))
    eng.close()
