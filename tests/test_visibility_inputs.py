"""The inputs of tests/test_gpu_visibility.py, checked with the oracle and numpy alone (no GPU, none of
the code under test but engine.visible_subset, which only selects objects).

The GPU tests compare a visibility state committed on a kept TLAS topology with a fresh oracle build of
the scene that holds only the visible objects.  The two may order equal-t candidates differently, so
the comparison stands for inputs free of such ties between instances.  For every case, state and ray set:
  * the oracle of the visible scene agrees bit for bit, rays and frame, with the oracle of the same
    scene with its object order reversed: nothing depends on the TLAS order;
  * no ray has a second triangle within 1e-9 relative of its closest t (deform_scenes.closest_gap);
    the near-vertex sets of the "far" case aim at shared vertices and edges, ties inside one BLAS
    whose order no commit changes, so theirs is the condition between objects (instance_gap);
  * at least a tenth of the rays hit (states with no visible object are exempt: nothing can hit);
  * at least a twentieth of the answers differ from the all-visible state, so an implementation
    that hides nothing cannot pass.
These are conditions on the inputs, not measurements of the code."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_scenes as DS                                                       # noqa: E402
import visibility_scenes as V                                                    # noqa: E402
import wide_tree_check as W                                                      # noqa: E402

_ANSWERS = {}


def _oracle(sc, O, D, tmax, frame):
    osc = oracle.OracleScene(sc)
    out = [osc.trace_rays(O, D), osc.occluded_rays(O, D, tmax)]
    if frame:
        rgb, rgba, st = osc.render(0, threads=0, rgba=True)
        out.append((rgb, rgba, (st.primary_rays, st.shadow_rays, st.secondary_rays)))
    osc.close()
    return out


def _answers(name, state):
    """The oracle's answers of one state, computed once (the all-visible state serves every other)."""
    if (name, state) not in _ANSWERS:
        c = V.case(name)
        O, D, tmax = c.rays
        _ANSWERS[name, state] = _oracle(c.visible(state), O, D, tmax, c.frame)
    return _ANSWERS[name, state]


def _same(a, b):
    (ta, pa, na, ma), oa = a[0], a[1]
    (tb, pb, nb, mb), ob = b[0], b[1]
    hit = np.isfinite(ta)
    ok = np.array_equal(ta.view(np.uint64), tb.view(np.uint64)) and np.array_equal(ma, mb) and np.array_equal(oa, ob)
    ok = ok and np.array_equal(pa[hit], pb[hit]) and np.array_equal(na[hit], nb[hit])
    if len(a) > 2:
        ok = ok and np.array_equal(a[2][0].view(np.uint64), b[2][0].view(np.uint64)) and np.array_equal(a[2][1], b[2][1])
        ok = ok and a[2][2] == b[2][2]
    return ok


def _changed(a, b):
    """The share of rays whose closest hit or occlusion answer differs."""
    (ta, _, _, ma), oa = a[0], a[1]
    (tb, _, _, mb), ob = b[0], b[1]
    return float(((ta.view(np.uint64) != tb.view(np.uint64)) | (ma != mb) | (oa != ob)).mean())


PAIRS = [(n, s) for n in V.CASES for s in V.case(n).states if not (n == "pool" and s == "all")]


@pytest.mark.parametrize("name,state", PAIRS)
def test_state_is_tie_free_hits_and_differs(name, state):
    c = V.case(name)
    O, D, tmax = c.rays
    vs = c.visible(state)
    got = _answers(name, state)
    rev = _oracle(V.reversed_objects(vs), O, D, tmax, c.frame)
    assert _same(got, rev), "the oracle's answers depend on the object order"
    if c.tie_rule == "triangle":
        tris = V.all_triangles(vs)
        if len(tris) >= 2:                                 # a single triangle has no second one
            gap = DS.closest_gap(tris, O, D, chunk=32)[1]
            assert gap.min() > 1e-9, f"a ray has two triangles within {gap.min()} of its closest t"
    else:
        # the far mesh is hit by none of these rays (test_the_far_sets_see_only_their_own_side)
        gap = V.instance_gap(vs, O, D, skip_ids=(V.FAR_ID,))
        assert gap.min() > 1e-9, f"two objects' closest hits lie within {gap.min()}"
    share = float(np.isfinite(got[0][0]).mean())
    print(f"{name}/{state}: {len(vs.objects)} objects, hit share {share:.3f}")
    if len(vs.objects):
        assert share >= 0.1
    else:
        assert share == 0.0 and not got[1].any()
    if c.states[state] and name != "far":
        full = "live300" if name == "pool" else "all"
        ch = _changed(got, _answers(name, full))
        print(f"{name}/{state}: {ch:.3f} of the answers differ from the all-visible state")
        assert ch >= 0.05


def test_the_far_sets_see_only_their_own_side():
    """The far case's two near-vertex sets: the rays at the near instances never hit the far mesh and
    the rays at the far mesh never hit a near instance, so between objects only the near instances can
    tie (instance_gap above), and hiding the far mesh changes every far ray that hit."""
    c = V.case("far")
    only_far = V.engine.visible_subset(c.scene, [i == V.FAR_OBJECT for i in range(len(c.scene.objects))])
    O, D, tmax = c.rays
    osc = oracle.OracleScene(only_far)
    assert not np.isfinite(osc.trace_rays(O, D)[0]).any()
    Of, Df, tf = c.far_rays
    t_far = osc.trace_rays(Of, Df)[0]
    osc.close()
    assert np.isfinite(t_far).mean() > 0.3
    osc = oracle.OracleScene(c.visible("far_hidden"))
    assert not np.isfinite(osc.trace_rays(Of, Df)[0]).any()
    osc.close()
    for sc in (c.visible("all"), V.reversed_objects(c.visible("all"))):
        osc = oracle.OracleScene(sc)
        assert np.array_equal(osc.trace_rays(Of, Df)[0].view(np.uint64), t_far.view(np.uint64))
        osc.close()


def test_the_six_shells_share_one_tlas_leaf():
    """leaf6: the oracle's TLAS of the scene as built keeps the six shells in one leaf and spreads
    group B over several others."""
    c = V.case("leaf6")
    leaf = np.asarray(W.tlas_leaves(c.scene))
    inst = {}                                 # object -> instance: MeshInstances first, then meshes (scene.cpp)
    order = [i for i, o in enumerate(c.scene.objects) if isinstance(o, V.M.MeshInstance)]
    order += [i for i, o in enumerate(c.scene.objects) if isinstance(o, V.M.Mesh)]
    for k, i in enumerate(order):
        inst[i] = k
    a = {int(leaf[inst[i]]) for i in V.LEAF6}
    b = {int(leaf[inst[i]]) for i in V.GROUP_B}
    assert len(a) == 1 and len(b) >= 4 and not (a & b), (a, b)


def test_the_combined_steps_are_tie_free_and_differ():
    """Every committed state of visibility_scenes.combined(): order-independent, tie-free, at least a
    tenth of the rays hit, and each step that changes what is seen changes a twentieth of the answers."""
    sc, (O, D, tmax), steps = V.combined()
    prev = None
    for k, st in enumerate(steps):
        vs = V.engine.visible_subset(st["scene"], [i not in st["hidden"] for i in range(len(st["scene"].objects))])
        got = _oracle(vs, O, D, tmax, True)
        assert _same(got, _oracle(V.reversed_objects(vs), O, D, tmax, True)), k
        gap = DS.closest_gap(V.all_triangles(vs), O, D)[1]
        assert gap.min() > 1e-9, (k, gap.min())
        assert np.isfinite(got[0][0]).mean() >= 0.1
        if prev is not None and k != 2:                   # step 3 changes only what is hidden: the mesh's
            ch = _changed(got, prev)                      # MeshInstance deforms with it, which may show less
            print(f"combined step {k + 1}: {ch:.3f} of the answers differ from the step before")
            assert ch >= 0.05
        prev = got
