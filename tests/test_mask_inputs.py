"""The inputs of tests/test_gpu_masks.py that tests/visibility_scenes.py does not already hold, checked
with the oracle and numpy alone (no GPU, none of the code under test but engine.visible_subset, which
only selects objects).  tests/test_visibility_inputs.py does the same for the visibility cases the mask
tests reuse (posed, kinds, leaf6).

A masked query is compared with a fresh oracle build of the scene that holds only the objects the ray
sees, whose TLAS differs from the one the engine walks; the comparison stands for inputs free of equal-t
ties between instances:
  (a) "baked posed" (mask_scenes.baked_posed: a static identity scene), states all / third / one: the
      oracle agrees bit for bit with the object-reversed scene, no ray has a second triangle within
      1e-9 relative of its closest t (rays that had one were dropped, at most 1 % of the set), at least
      a tenth of the rays hit and at least a twentieth of the answers differ from the state "all";
  (b) "stacked" (mask_scenes.stacked): at least 100 rays have two triangles of A at an equal closest t,
      so they take the walks' tie re-walk; every ray that hits A hits B first; the answers for {A}, {B}
      and {A, B} do not depend on the object order;
  (c) the centre rays of posed's camera (gbuffer_rays.first_rays): the oracle of each masked sub-scene
      agrees with its object-reversed scene on them.
These are conditions on the inputs, not measurements of the code."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_scenes as DS                                                       # noqa: E402
import gbuffer_rays as GR                                                        # noqa: E402
import mask_scenes as MS                                                         # noqa: E402
import visibility_scenes as V                                                    # noqa: E402

_ANSWERS = {}


def _oracle(sc, O, D, tmax, tmin=None):
    osc = oracle.OracleScene(sc)
    out = (osc.trace_rays(O, D, tmin), osc.occluded_rays(O, D, tmax))
    osc.close()
    return out


def _same(a, b):
    (ta, pa, na, ma), oa = a
    (tb, pb, nb, mb), ob = b
    hit = np.isfinite(ta)
    return (np.array_equal(ta.view(np.uint64), tb.view(np.uint64)) and np.array_equal(ma, mb) and np.array_equal(oa, ob) and
            np.array_equal(pa[hit], pb[hit]) and np.array_equal(na[hit], nb[hit]))


def _changed(a, b):
    (ta, _, _, ma), oa = a
    (tb, _, _, mb), ob = b
    return float(((ta.view(np.uint64) != tb.view(np.uint64)) | (ma != mb) | (oa != ob)).mean())


def _baked(state):
    if state not in _ANSWERS:
        c = MS.baked_posed()
        _ANSWERS[state] = _oracle(c.visible(state), *c.rays)
    return _ANSWERS[state]


def test_baked_posed_drops_at_most_a_hundredth_of_the_rays():
    c = MS.baked_posed()
    n = len(V.case("posed").rays[0])
    print(f"baked posed: {c.dropped} of {n} rays dropped")
    assert c.dropped <= n // 100 and len(c.rays[0]) == n - c.dropped
    assert len(c.scene.objects) == 12
    for o in c.scene.objects:                              # a static identity scene: Meshes under the identity
        assert isinstance(o, V.M.Mesh) and tuple(o.transform) == tuple(V.M.Mesh(id=0).transform)


@pytest.mark.parametrize("state", ["all", "third", "one"])
def test_baked_posed_is_tie_free_hits_and_differs(state):
    c = MS.baked_posed()
    O, D, tmax = c.rays
    vs = c.visible(state)
    got = _baked(state)
    assert _same(got, _oracle(V.reversed_objects(vs), O, D, tmax)), "the oracle's answers depend on the object order"
    gap = DS.closest_gap(V.all_triangles(vs), O, D, chunk=32)[1]
    assert gap.min() > MS.GAP, f"a ray has two triangles within {gap.min()} of its closest t"
    share = float(np.isfinite(got[0][0]).mean())
    print(f"baked posed/{state}: {len(vs.objects)} objects, hit share {share:.3f}")
    assert share >= 0.1
    if state != "all":
        ch = _changed(got, _baked("all"))
        print(f"baked posed/{state}: {ch:.3f} of the answers differ from the state all")
        assert ch >= 0.05


def test_stacked_ties_lie_inside_a_and_b_is_hit_first():
    O, D, tmax = MS.stacked_rays()
    for baked in (False, True):
        sc = MS.stacked(baked)
        gap = DS.closest_gap(V.object_triangles(sc, 0), O, D)[1]
        ties = int((gap == 0).sum())
        print(f"stacked (baked={baked}): {ties} of {len(O)} rays have two triangles of A at an equal closest t")
        assert ties >= 100
        got = {name: _oracle(MS.subset(sc, hidden), O, D, tmax) for name, hidden in MS.STACKED_SETS.items()}
        for name, hidden in MS.STACKED_SETS.items():
            rev = _oracle(V.reversed_objects(MS.subset(sc, hidden)), O, D, tmax)
            assert _same(got[name], rev), f"{name}: the oracle's answers depend on the object order"
        tA, tB, tAB = got["A"][0][0], got["B"][0][0], got["AB"][0][0]
        hitA = np.isfinite(tA)
        assert hitA.sum() >= 50
        assert np.isfinite(tB[hitA]).all() and (tB[hitA] < tA[hitA]).all()
        assert np.array_equal(tAB.view(np.uint64), tB.view(np.uint64))     # with both, B decides every answer
        # tmax lies between the two: a segment is blocked by B and never by A
        assert not got["A"][1].any() and np.array_equal(got["B"][1], np.isfinite(tB)) and got["B"][1].any()


@pytest.mark.parametrize("state", ["all", "third", "one"])
def test_posed_centre_rays_do_not_depend_on_the_object_order(state):
    c = V.case("posed")
    r = GR.first_rays(c.scene, 0, 0, 1, centre=True)
    O, D, tmin = r["origins"].reshape(-1, 3), r["dirs"].reshape(-1, 3), r["tmin"].reshape(-1)
    tmax = np.full(len(O), 1e3)
    vs = c.visible(state)
    got = _oracle(vs, O, D, tmax, tmin)
    assert _same(got, _oracle(V.reversed_objects(vs), O, D, tmax, tmin))
    share = float(np.isfinite(got[0][0]).mean())
    print(f"posed centre rays/{state}: hit share {share:.3f}")
    assert share > 0.0
