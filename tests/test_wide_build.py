"""The four-wide trees of host builds (scene.cpp build_wide, build_wide_tw, build_fit,
wide_octant_copies), read back with rt_debug_wide_build and checked structurally by
tests/wide_tree_check.py: every slot box against an FP64 restatement, exactly.  CPU only.

Inner slots after a build: the fit tree, the TLAS part and the BLAS parts of a transformed scene
are asserted to EQUAL the float union of their child node's slots - the builders round the FP64
union of the children outward, and rounding is monotone, so the rounded union is the union of the
rounded children.  The same holds for the groups WideBuilder::regroup makes of a TLAS leaf with
more than four instances (the group's box is the fmin / fmax over its members, rounded), so the
regroup scene below asserts "equal" too.  Only an identity scene whose TLAS has inner nodes is held
to "contains": there a slot may carry a TLAS leaf's own box, which is AABB.transformed of the
instance's triangles and not the BLAS root box its child node holds."""
import copy
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import engine, scenes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_tree_check as W                                      # noqa: E402
from test_fit_build import _instanced, _rot                     # noqa: E402
from test_fit_coincident import _stacked                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def m16(lin, t):
    M4 = np.eye(4)
    M4[:3, :3] = lin
    M4[:3, 3] = t
    return tuple(float(x) for x in M4.T.reshape(-1))


def small_scene(transforms, n=6, base_at=(20.0, 0.0, 0.0), faces=None):
    """A heightfield mesh of 2 n^2 float-exact triangles (its own instance translated to base_at)
    and one mesh instance per transform."""
    hp, hf = scenes.heightfield(n, 4.0, 0.5, 3)
    hf = hf if faces is None else hf[:faces]
    mesh = M.Mesh(id=1, material="1", positions=hp.astype(np.float32).astype(np.float64), indices=hf.astype(np.int32),
                  indices_one_based=False, shading_mode="flat", transform=M.translation(*base_at))
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [mesh] + [M.MeshInstance(id=10 + k, base_mesh_id=1, material="1", transform=tuple(t))
                           for k, t in enumerate(transforms)]
    return sc


def posed(k):
    return m16(_rot(0.3 * k + 0.2, 0.7 * k) * (0.6 + 0.4 * k), (1.5 * k - 2.0, -0.5 * k, 0.25 * k))


def kappa_pose():
    """|l2w| |w2l| = 2^13, over kFitKappa = 2^12: the mesh squashed along z into a strip in the xy plane."""
    return m16(np.diag([1.0, 1.0, 2.0 ** -13]), (0.0, 1.0, 0.0))


def _c2():
    return scenes.scaled(scenes.scene_c2(inline=True), 8, 8)


def regroup_scene():
    """Six identity meshes of two shapes with one bounding box: no plane separates their equal
    centroids, so the TLAS is one leaf of six instances and WideBuilder::regroup splits it."""
    hp, hf = scenes.heightfield(6, 4.0, 0.5, 3)
    hp = hp.astype(np.float32).astype(np.float64)
    shapes = [hf.astype(np.int32), hf[::-1, ::-1].astype(np.int32).copy()]
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [M.Mesh(id=1 + k, material="1", positions=hp, indices=shapes[k % 2], indices_one_based=False,
                         shading_mode="flat") for k in range(6)]
    return sc


def _meshes_below(d, node, slot, tris_per_mesh):
    """The meshes whose triangles lie below one slot of copy 0."""
    near, ref, far, _ = W.split_nodes(d["nodes"][: int(d["wide_copy"])])
    out, st = set(), [int(ref[node, slot])]
    while st:
        r = st.pop()
        if r < 0:
            out.add(int(d["tri_prim"][~r]) // tris_per_mesh)
            continue
        st += [int(ref[r, s]) for s in range(4) if near[r, 0, s] < np.inf]
    return out


# ---------------------------------------------------------------- the scenes
def test_c2_identity():
    sc = _c2()
    d = engine.wide_build(sc)
    assert d["identity"] == 1 and d["fit_root"] == -1 and d["wide_root"] >= 0 and d["instances"] == 1
    W.assert_ok(d, sc, inner={"identity": "equal"})            # one TLAS leaf: no slot carries a TLAS box


def test_regrouped_tlas_leaf():
    """Groups of WideBuilder::regroup EQUAL the union of their members (module docstring)."""
    sc = regroup_scene()
    d = engine.wide_build(sc)
    assert d["identity"] == 1 and d["instances"] == 6
    root = int(d["wide_root"])
    sizes = sorted(len(_meshes_below(d, root, s, 72)) for s in range(4))
    assert sizes == [1, 1, 2, 2], f"the root's slots hold {sizes} meshes: regroup was not taken"
    W.assert_ok(d, sc, inner={"identity": "equal"})


def test_identity_scene_with_tlas_inner_nodes_contains():
    """Four identity meshes apart, their vertices no floats: the TLAS has inner nodes, and a slot
    that stands for a TLAS leaf carries that leaf's own box (AABB.transformed by the identity of the
    triangles' boxes), not the union of the BLAS root boxes below it - the verifier's "contain"
    mode, its default for identity trees."""
    hp, hf = scenes.heightfield(6, 4.0, 0.5, 3)
    sc = scenes.scaled(scenes.scene_c1(8, 8), 8, 8)
    sc.objects = [M.Mesh(id=1 + k, material="1", positions=(hp + np.array([7.0 * k, 0.3 * k, -5.0 * (k % 2)])) * (1.0 + 2.0 ** -30),
                         indices=hf.astype(np.int32), indices_one_based=False, shading_mode="flat") for k in range(4)]
    d = engine.wide_build(sc)
    assert d["identity"] == 1 and d["instances"] == 4 and len(set(W.tlas_leaves(sc).tolist())) >= 2
    rep = W.assert_ok(d, sc)
    assert d["wide_coord"] >= 21.0 and rep.trees["identity"]["depth"] >= 2


def test_triangle_object_beside_instances():
    sc = small_scene([posed(0), posed(1)])
    sc.objects.insert(1, M.Triangle(vertices=((-3.0, -1.0, -3.0), (3.0, -1.0, -3.0), (0.0, 2.0, -3.5)), material="1",
                                    transform=m16(_rot(0.2, 0.1) * 1.3, (0.0, -2.0, 1.0))))
    d = engine.wide_build(sc)
    assert d["instances"] == 4 and (d["wroot"] < 0).sum() == 1 and d["fit_root"] >= 0
    W.assert_ok(d, sc)


def test_instanced():
    sc = _instanced()
    d = engine.wide_build(sc)
    assert d["identity"] == 0 and d["fit_root"] >= 0 and d["pairs"] > 0 and d["tw_tlas_nodes"] > 0
    rep = W.assert_ok(d, sc)
    assert set(rep.trees) >= {"tlas", "fit"} and any(k.startswith("blas@") for k in rep.trees)


@pytest.mark.parametrize("n", [5, 6, 9])
def test_stacked_instances_have_group_nodes(n):
    sc = _stacked(n)
    d = engine.wide_build(sc)
    assert d["fit_root"] >= 0
    W.assert_ok(d, sc)
    # a group node: two or more pairs of ONE leaf run (one box, several instances) side by side
    near, ref, far, _ = W.split_nodes(d["nodes"][: int(d["wide_copy"])])
    fr, fn = int(d["fit_root"]), int(d["fit_nodes"])
    groups = 0
    for k in range(fr, fr + fn):
        t0 = [int(d["fpairs"][~r, 0]) for s, r in enumerate(ref[k]) if near[k, 0, s] < np.inf and r < 0]
        groups += len(t0) >= 2 and len(set(t0)) == 1 and len(t0) == int((near[k, 0] < np.inf).sum())
    assert groups > 0


def test_mirrored_instance():
    sc = small_scene([posed(0), m16(_rot(0.4, 0.1) @ np.diag([-1.0, 1.2, 0.9]), (1.0, 0.5, -1.0))])
    d = engine.wide_build(sc)
    dets = [np.linalg.det(m.reshape(4, 4).T[:3, :3]) for m in d["l2w"]]
    assert min(dets) < 0 < max(dets) and d["fit_root"] >= 0
    W.assert_ok(d, sc)


def test_instance_at_1e6():
    sc = small_scene([posed(0), m16(_rot(0.1, 0.2), (1e6, 1e6, 1e6))])
    d = engine.wide_build(sc)
    assert d["wide_coord"] >= 1e6 and d["fit_coord"] >= 1e6 and d["fit_root"] >= 0
    W.assert_ok(d, sc)


def test_blas_of_one_leaf_run():
    sc = small_scene([posed(0), posed(1)], faces=1)
    d = engine.wide_build(sc)
    assert (d["wroot"] < 0).all() and d["tris"] == 1 and d["pairs"] == 3
    W.assert_ok(d, sc)


def test_instance_over_kappa_has_no_fit_tree():
    sc = small_scene([posed(0), kappa_pose()])
    d = engine.wide_build(sc)
    assert d["fit_root"] == -1 and d["pairs"] == 0 and d["wide_root"] >= 0 and d["tw_tlas_nodes"] > 0
    rep = W.assert_ok(d, sc)
    assert "fit" not in rep.trees and "tlas" in rep.trees


def test_dynamic_identity_scene_takes_the_transformed_layout():
    sc = _c2()
    d = engine.wide_build(sc, dynamic=True)
    assert d["identity"] == 0 and d["instances"] == 1 and d["fit_root"] >= 0 and d["tw_tlas_nodes"] == 1
    W.assert_ok(d, sc)


def _digest(d):
    h = hashlib.sha256()
    for k in sorted(d):
        h.update(k.encode())
        h.update(d[k].tobytes() if isinstance(d[k], np.ndarray) else repr(d[k]).encode())
    return h.hexdigest()


def test_the_read_back_does_not_depend_on_the_thread_count():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import json; "
            "from myraytracer_amd import engine; import test_wide_build as T; "
            "print(json.dumps([T._digest(engine.wide_build(s, dyn)) for s in (T._c2(), T._instanced(), T._stacked(9)) "
            "for dyn in (False, True)]))" % (ROOT, os.path.join(ROOT, "tests")))
    res = []
    for t in ("1", "8"):
        env = dict(os.environ, MYRT_BUILD_THREADS=t)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        res.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert res[0] == res[1] and len(set(res[0])) == 4          # only C2 builds differently as a dynamic scene


# ---------------------------------------------------------------- the verifier's own test
def _good():
    sc = small_scene([posed(0), posed(1), posed(2)])
    d = engine.wide_build(sc, dynamic=True)
    assert W.verify(d, sc, after_refit=True).ok()
    return sc, d


def _views(d):
    """Writable float / int views of the raw node records: near (N, 3, 4), ref (N, 4), far."""
    n = d["nodes"]
    f, i = n.view(np.float32).reshape(-1, 8, 4), n.view(np.int32).reshape(-1, 8, 4)   # rows: 3 near, ref, 3 far, pad
    assert np.shares_memory(f, n) and np.shares_memory(i, n)
    return f[:, 0:3, :], i[:, 3, :], f[:, 4:7, :]


def _fit_slot(d, terminal, copy_=0):
    """(node, slot) of the fit tree's first terminal / inner slot in an octant copy."""
    near, ref, far = _views(d)
    N, fr, fn = int(d["wide_copy"]), int(d["fit_root"]), int(d["fit_nodes"])
    for k in range(copy_ * N + fr, copy_ * N + fr + fn):
        for s in range(4):
            if near[k, 0, s] < np.inf and (ref[k, s] < 0) == terminal:
                return k, s
    raise AssertionError("no such slot")


def test_the_verifier_reports_each_corruption():
    sc, good = _good()
    assert good["nodes"].flags.c_contiguous

    def corrupt(fn):
        d = copy.deepcopy(good)
        fn(d)
        return W.verify(d, sc, after_refit=True).kinds()

    def near_up(d):                                            # one slot's near plane raised by one ulp
        near, ref, far = _views(d)
        k, s = _fit_slot(d, True)
        near[k, 1, s] = np.nextafter(near[k, 1, s], np.float32(np.inf))

    def rows_swapped(d):                                       # one copy's near / far rows swapped for one slot
        near, ref, far = _views(d)
        k, s = _fit_slot(d, True, copy_=3)
        a, b = near[k, 2, s].copy(), far[k, 2, s].copy()
        assert a != b
        near[k, 2, s], far[k, 2, s] = b, a

    def pair_dropped(d):
        d["fpairs"] = d["fpairs"][:-1].copy()
        d["pairs"] -= 1

    def stale_inner(d):                                        # one inner box left at a larger, older value
        near, ref, far = _views(d)
        k, s = _fit_slot(d, False)
        far[k, 0, s] = np.nextafter(far[k, 0, s], np.float32(np.inf))
        for o in range(1, 8):                                  # consistently in every copy: only `inner` can see it
            ko = o * int(d["wide_copy"]) + k
            so = int(np.flatnonzero(ref[ko] == ref[k, s])[0])
            row = near if o & 1 else far
            row[ko, 0, so] = far[k, 0, s]

    def out_of_order(d):                                       # two slots of one copy exchanged against their keys
        near, ref, far = _views(d)
        N, fr = int(d["wide_copy"]), int(d["fit_root"])
        for k in range(5 * N + fr, 5 * N + fr + int(d["fit_nodes"])):
            key = -0.5 * (near[k, 0].astype(np.float64) + far[k, 0]) + 0.5 * (near[k, 1].astype(np.float64) + far[k, 1]) \
                  - 0.5 * (near[k, 2].astype(np.float64) + far[k, 2])
            if np.isfinite(key[:2]).all() and key[0] < key[1]:
                for a in (near, far):
                    a[k, :, [0, 1]] = a[k, :, [1, 0]]
                ref[k, [0, 1]] = ref[k, [1, 0]]
                return
        raise AssertionError("no node with two distinct keys")

    def tbox_of_one_instance(d):                               # a two-instance TLAS leaf, each given its own bounds
        lf = W.tlas_leaves(sc)
        ks = [k for k in range(len(lf)) if (lf == lf[k]).sum() >= 2][:2]
        assert len(ks) == 2 and not np.array_equal(d["inst_bounds"][ks[0]], d["inst_bounds"][ks[1]])
        near, ref, far = _views(d)
        for k in ks:
            d["tbox"][k] = d["inst_bounds"][k]
            for o in range(8):                                 # the markers follow, so only the membership is wrong
                N = int(d["wide_copy"])
                tl = slice(o * N, o * N + int(d["tw_tlas_nodes"]))
                node, slot = np.nonzero(ref[tl] == ~(int(d["marker_base"]) + k))
                lo, hi = W.f32_down(d["tbox"][k][:3]), W.f32_up(d["tbox"][k][3:])
                for a in range(3):
                    neg = (o >> a) & 1
                    near[tl][node, a, slot] = hi[a] if neg else lo[a]
                    far[tl][node, a, slot] = lo[a] if neg else hi[a]

    def fit_coord_halved(d):
        d["fit_coord"] *= 0.5

    assert "terminal" in corrupt(near_up)
    assert "octant" in corrupt(rows_swapped)
    assert "pairs" in corrupt(pair_dropped)
    assert corrupt(stale_inner) == ["inner"]
    assert corrupt(out_of_order) == ["order"]
    assert corrupt(fit_coord_halved) == ["scalar"]
    d = copy.deepcopy(good)
    tbox_of_one_instance(d)
    assert any("TLAS leaf" in m for k, m in W.verify(d, sc, after_refit=True).problems if k == "terminal")
