"""Instance visibility (rtcore.h "instance visibility"): instances of a dynamic scene are
hidden and shown again at a commit, with stable indices.

Every comparison of hits, frames and ray counts is with oracle.OracleScene(eng.visible_scene()): the
scene that holds only the visible objects, built fresh.  None is with the code under test.  The scenes,
states and ray sets are tests/visibility_scenes.py's; tests/test_visibility_inputs.py shows on the CPU
that each is free of equal-t ties between instances, hits, and differs from the all-visible state.  The
four-wide nodes are read back (rt_debug_wide_read) and checked slot by slot against the FP64
restatements of tests/wide_tree_check.py."""
import copy
import os
import sys

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import engine
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visibility_scenes as V                                                    # noqa: E402
import wide_tree_check as W                                                      # noqa: E402

pytestmark = pytest.mark.gpu

WALKS = {"transformed": {}, "transformed_tw": {"fit": 0}, "transformed_binary": {"wide": 0},
         "nested": {"unified_transformed": 0}}
FLT_MAX = np.float32(3.4028234663852886e38)


# ---------------------------------------------------------------- helpers
def _engine(sc, walk="transformed", devices=None, deformable=False):
    eng = M.RayTracerEngine(copy.deepcopy(sc), devices, dynamic=True, deformable=deformable)
    for k, v in WALKS[walk].items():
        eng.set_option(k, v)
    return eng


def _set_hidden(eng, hidden, rebuild=False):
    """Stages every object's flag (hidden: the object indices to hide) and commits."""
    n = len(eng.scene.objects)
    eng.set_visible_many(range(n), [i not in hidden for i in range(n)])
    cs = eng.commit(rebuild=rebuild)
    vs = eng.last_visibility_stats()
    assert vs.visible == n - len(hidden) and vs.instances == n
    assert [eng.is_visible(i) for i in range(n)] == [i not in hidden for i in range(n)]
    return cs, vs


_REF = {}


def _ref(eng, key, O, D, tmax, frame=False):
    """The oracle's answers for the scene of the engine's visible objects, once per key (a case and
    state: the engines of every walk then hold the same visible scene, which is asserted)."""
    vs = eng.visible_scene()
    sig = [(type(o).__name__, getattr(o, "id", None), tuple(o.transform)) for o in vs.objects]
    if key not in _REF:
        osc = oracle.OracleScene(vs)
        out = dict(sig=sig, rays=(osc.trace_rays(O, D), osc.occluded_rays(O, D, tmax)))
        if frame:
            out["frame"] = osc.render(0, threads=0, rgba=True)
        osc.close()
        _REF[key] = out
    assert _REF[key]["sig"] == sig, "another visible scene under the same key"
    return _REF[key]


def _assert_rays(eng, ref, O, D, tmax, slot=0):
    (to, po, no, mo), oo = ref["rays"]
    tg, pg, ng, mg = eng.trace_rays(O, D, slot=slot)
    hit = np.isfinite(to)
    assert np.array_equal(tg.view(np.uint64), to.view(np.uint64)), f"t differs on {int((tg != to).sum())} of {len(to)} rays"
    assert np.array_equal(mg, mo)
    assert np.array_equal(pg[hit], po[hit]) and np.array_equal(ng[hit], no[hit])
    og = eng.occluded_rays(O, D, tmax, slot=slot)
    assert np.array_equal(og, oo), f"occlusion differs on {int((og != oo).sum())} rays"


def _assert_frame(eng, ref):
    """The project's bar: L-inf <= 1e-5 on FP64, exact RGBA8, equal ray counts."""
    rgb, rgba, st = eng.render_rows(0, 0, 1, True)
    want, want8, ost = ref["frame"]
    assert float(np.abs(rgb - want).max()) <= 1e-5
    assert np.array_equal(rgba, want8)
    assert (st.primary_rays, st.shadow_rays, st.secondary_rays) == (ost.primary_rays, ost.shadow_rays, ost.secondary_rays)


def _check(eng, key, case, frame=None):
    O, D, tmax = case.rays
    frame = case.frame if frame is None else frame
    ref = _ref(eng, key, O, D, tmax, frame)
    _assert_rays(eng, ref, O, D, tmax)
    if frame:
        _assert_frame(eng, ref)
    return ref


# ---------------------------------------------------------------- 1. every walk
@pytest.mark.parametrize("walk", list(WALKS))
def test_every_walk_hides_a_third_and_shows_it_again(walk):
    c = V.case("posed")
    eng = _engine(c.scene, walk)
    cs, vs = _set_hidden(eng, c.states["third"])
    assert (vs.hidden, vs.shown, cs.instances_moved) == (4, 0, 0)
    _check(eng, ("posed", "third"), c)
    cs, vs = _set_hidden(eng, c.states["all"])
    assert (vs.hidden, vs.shown) == (0, 4)
    _check(eng, ("posed", "all"), c)
    eng.close()


# ---------------------------------------------------------------- 2. every object kind
@pytest.mark.parametrize("state", ["base", "instance", "sphere", "plane", "triangle", "mesh"])
def test_every_object_kind_hides(state):
    c = V.case("kinds")
    for walk in ("transformed", "nested"):
        eng = _engine(c.scene, walk)
        _set_hidden(eng, c.states[state])
        _check(eng, ("kinds", state), c, frame=walk == "transformed")
        eng.close()


# ---------------------------------------------------------------- 3. TLAS leaves and subtrees
@pytest.mark.parametrize("walk", ["transformed", "transformed_tw", "transformed_binary"])
def test_parts_of_a_tlas_leaf_the_leaf_and_a_subtree(walk):
    c = V.case("leaf6")
    eng = _engine(c.scene, walk)
    for state in ("some_of_leaf", "whole_leaf", "group_b", "all"):
        _set_hidden(eng, c.states[state])
        _check(eng, ("leaf6", state), c, frame=walk == "transformed")
    eng.close()


# ---------------------------------------------------------------- 4. all hidden
@pytest.mark.parametrize("walk", ["transformed", "transformed_binary"])
def test_all_hidden_is_the_scene_without_objects(walk):
    c = V.case("posed")
    O, D, tmax = c.rays
    eng = _engine(c.scene, walk)
    _set_hidden(eng, c.states["none"])
    assert eng.visible_scene().objects == []
    ref = _check(eng, ("posed", "none"), c)
    assert ref["frame"][2].shadow_rays == 0 and not np.isfinite(ref["rays"][0][0]).any()
    h = eng.query_closest(O, D, want=("t", "ids", "flags"))
    assert np.isinf(h.t).all() and (h.ids == -1).all() and not h.flags.any()
    assert not eng.query_occluded(O, D, tmax).any()
    _set_hidden(eng, c.states["one"])
    _check(eng, ("posed", "one"), c)
    eng.close()


# ---------------------------------------------------------------- 5. the nodes themselves
def _slot_test_fails(near, far):
    """wide_node's slot test restated for a slot's six rows in one octant copy (near / far planes
    per axis) over |1/d| = 2^-100, 1 and 2^100 with origin offsets up to 2^27 |1/d|: the entry
    distance is positive, the exit distance negative and neither is a NaN, so max(tn, weps) <=
    min(tf, lim) fails for every weps and lim."""
    for e in (-100, 0, 100):
        for off in (0.0, 2.0 ** 27, -2.0 ** 27):
            inv = np.ldexp(1.0, e)
            with np.errstate(over="ignore"):
                tn = np.float32(np.float64(near) * inv + off * inv).max()
                tf = np.float32(np.float64(far) * inv + off * inv).min()
            if not (tn > 0 > tf):
                return False
    return True


def _check_hidden_nodes(d, hidden_inst, leaf_of):
    """The read-back after a hiding plain commit: hidden slots carry the hidden encoding in every
    copy, inner slots are the unions of their child's visible slots, visible terminal slots are
    down / up of their restated FP64 boxes."""
    N = int(d["wide_copy"])
    near8, ref8, far8, _ = W.split_nodes(d["nodes"])
    near, ref, far = near8[:N], ref8[:N], far8[:N]
    full = near[:, 0, :] < W.INF32
    hid = full & (near[:, 0, :] > far[:, 0, :])
    assert np.array_equal(hid, full & (near == FLT_MAX).all(axis=1) & (far == -FLT_MAX).all(axis=1)), \
        "a slot with near > far that is not the hidden encoding"
    nt, mbase = int(d["tw_tlas_nodes"]), int(d["marker_base"])
    fr, fn = int(d["fit_root"]), int(d["fit_nodes"])
    fp = np.asarray(d["fpairs"], np.int64).reshape(-1, 2)
    ib = np.asarray(d["inst_bounds"], np.float64).reshape(-1, 6)
    lbox, l2w = np.asarray(d["lbox"], np.float64), np.asarray(d["l2w"], np.float64).reshape(-1, 16)
    ni = int(d["instances"])
    vis = np.array([k not in hidden_inst for k in range(ni)])
    # tbox restated: the union of the world bounds of the VISIBLE instances of the TLAS leaf
    tbox = np.full((ni, 6), np.nan)
    for leaf in np.unique(leaf_of):
        ks = np.flatnonzero((leaf_of == leaf) & vis)
        if len(ks):
            tbox[ks] = np.concatenate([ib[ks, :3].min(axis=0), ib[ks, 3:].max(axis=0)])
    got_tb = np.asarray(d["tbox"], np.float64).reshape(ni, 6)
    assert np.array_equal(got_tb[vis], tbox[vis]) and np.isnan(got_tb[~vis]).all()
    counts = dict(hidden_terminal=0, hidden_inner=0, visible_terminal=0, inner=0)
    for lo, hi, kind in ((0, nt, "tlas"), (fr, fr + fn, "fit")):
        for n in range(lo, hi):
            for s in range(4):
                if not full[n, s]:
                    continue
                r = int(ref[n, s])
                if r < 0:
                    e = ~r
                    inst = e - mbase if kind == "tlas" else int(fp[e, 1])
                    if inst in hidden_inst:
                        assert hid[n, s], (kind, n, s, "a hidden instance's slot has a box")
                        counts["hidden_terminal"] += 1
                        continue
                    assert not hid[n, s], (kind, n, s, "a visible instance's slot is hidden")
                    if kind == "tlas":
                        blo, bhi = tbox[inst, :3], tbox[inst, 3:]
                    else:
                        blo, bhi, _ = W.pair_boxes(lbox[fp[e:e + 1, 0]], l2w[fp[e:e + 1, 1]])
                        blo, bhi = blo[0], bhi[0]
                    assert np.array_equal(near[n, :, s], W.f32_down(blo)) and np.array_equal(far[n, :, s], W.f32_up(bhi)), (kind, n, s)
                    counts["visible_terminal"] += 1
                else:
                    seen = full[r] & ~hid[r]
                    if not seen.any():
                        assert hid[n, s], (kind, n, s, "nothing visible below, but the slot has a box")
                        counts["hidden_inner"] += 1
                    else:
                        assert np.array_equal(near[n, :, s], near[r][:, seen].min(axis=1)), (kind, n, s)
                        assert np.array_equal(far[n, :, s], far[r][:, seen].max(axis=1)), (kind, n, s)
                        counts["inner"] += 1
    # (a) no ray enters a hidden slot in any octant copy; (b) it is no structural empty
    for o in range(8):
        nr, fa, rf = near8[o * N:(o + 1) * N], far8[o * N:(o + 1) * N], ref8[o * N:(o + 1) * N]
        fl = nr[:, 0, :] < W.INF32
        assert np.array_equal(fl.sum(axis=1), full.sum(axis=1)), "a hidden slot became an empty one in a copy"
        hn, hs = np.nonzero(fl & (np.abs(nr[:, 0, :]) == FLT_MAX))
        assert len(hn) == int(hid.sum())
        for n, s in zip(hn, hs):
            sign = np.array([-1.0 if (o >> a) & 1 else 1.0 for a in range(3)])      # d < 0 along a: rows swapped
            assert np.array_equal(nr[n, :, s], (sign * FLT_MAX).astype(np.float32))
            assert np.array_equal(fa[n, :, s], (-sign * FLT_MAX).astype(np.float32))
            assert _slot_test_fails(nr[n, :, s] * sign, fa[n, :, s] * sign)
    return counts


def _instances_of(eng, objects):
    return {eng.instance_of(i) for i in objects}


def test_the_nodes_of_a_hiding_commit_two_replicas_and_twenty_rounds():
    c = V.case("leaf6")
    leaf_of = np.asarray(W.tlas_leaves(c.scene))
    eng = _engine(c.scene, devices=[0, 0])
    built = eng.wide_read(0)
    hidden = frozenset({2, 4, 5}) | frozenset(V.GROUP_B)         # part of the leaf of six, and all of group B
    _set_hidden(eng, hidden)
    d0, d1 = eng.wide_read(0), eng.wide_read(1)
    assert W.same_dump(d0, d1) is None, f"the replicas differ in {W.same_dump(d0, d1)}"
    counts = _check_hidden_nodes(d0, _instances_of(eng, hidden), leaf_of)
    print("slots checked:", counts)
    assert min(counts.values()) > 0, counts                       # every kind of slot occurred, hidden inner ones too
    # the scalars and tbox are those of the scene without the hidden objects (a dynamic engine of it,
    # after a plain commit that moves nothing: the refit's own formulas)
    other = M.RayTracerEngine(eng.visible_scene(), dynamic=True)
    other.set_transform(0, other.scene.objects[0].transform)
    other.commit()
    e = other.wide_read()
    other.close()
    assert (d0["wide_coord"], d0["fit_coord"], d0["fit_blocked"]) == (e["wide_coord"], e["fit_coord"], e["fit_blocked"])
    vis = np.array([k not in _instances_of(eng, hidden) for k in range(int(d0["instances"]))])
    rows = lambda a: a[np.lexsort(a.T[::-1])]
    assert np.array_equal(rows(np.asarray(d0["tbox"])[vis]), rows(np.asarray(e["tbox"])))
    hide_bytes = d0["nodes"].copy()
    # shown again: per node the build's (ref, box) multisets, TLAS part and fit tree
    _set_hidden(eng, frozenset())
    back = eng.wide_read(0)
    W.assert_ok(back, eng.scene, after_refit=True, leaf_of=leaf_of)
    fr, fn, nt = int(built["fit_root"]), int(built["fit_nodes"]), int(built["tw_tlas_nodes"])
    for lo, hi in ((fr, fr + fn), (0, nt)):
        assert np.array_equal(W.node_multisets(back, lo, hi), W.node_multisets(built, lo, hi))
    assert (back["wide_coord"], back["fit_blocked"]) == (built["wide_coord"], built["fit_blocked"])
    show_bytes = back["nodes"].copy()
    for _ in range(20):
        _set_hidden(eng, hidden)
        assert np.array_equal(eng.wide_read(0)["nodes"], hide_bytes)
        _set_hidden(eng, frozenset())
    assert np.array_equal(eng.wide_read(0)["nodes"], show_bytes) and np.array_equal(eng.wide_read(1)["nodes"], show_bytes)
    assert eng.last_visibility_stats().forced_rebuild == 0
    eng.close()


# ---------------------------------------------------------------- 6. compaction at the seams
def _fit_terminals(d):
    """The pair refs of the fit tree's terminal slots (copy 0), walked from its root."""
    N = int(d["wide_copy"])
    near, ref, far, _ = W.split_nodes(d["nodes"][:N])
    out, todo = [], [int(d["fit_root"])]
    while todo:
        n = todo.pop()
        for s in range(4):
            if near[n, 0, s] < W.INF32:
                (out if ref[n, s] < 0 else todo).append(int(~ref[n, s]) if ref[n, s] < 0 else int(ref[n, s]))
    return out


def _shuffled_start(c, seed):
    """The case's scene at another pose: the engine is built there, so the tree refit to the case's
    pose is a poor one and a rebuild has a cost to lower."""
    sc = copy.deepcopy(c.scene)
    sc.objects[0].transform = M.translation(1.0, -6.0, 0.5)
    for k in range(1, len(sc.objects)):
        sc.objects[k].transform = V.spread(k - 1, seed=seed)
    return sc


def _compacting_commit(c, state, builder, key):
    """Engine built at a shuffled pose; one plain commit brings the case's pose and the state's
    visibility (the refit-only tree: rays checked), then a rebuilding commit compacts."""
    O, D, tmax = c.rays
    eng = _engine(_shuffled_start(c, 3))
    for i, o in enumerate(c.scene.objects):
        eng.set_transform(i, o.transform)
    hidden = c.states[state]
    _set_hidden(eng, hidden)
    ref = _ref(eng, key, O, D, tmax)
    _assert_rays(eng, ref, O, D, tmax)
    before = eng.fit_cost()
    eng.commit(rebuild=builder)
    return eng, ref, before


@pytest.mark.parametrize("builder", [True, "clustered"])
@pytest.mark.parametrize("live", V.POOL_LIVE)
def test_compaction_by_live_pair_count(live, builder):
    c = V.case("pool")
    O, D, tmax = c.rays
    eng, ref, before = _compacting_commit(c, f"live{live}", builder, ("pool", live))
    rs, vs, dt = eng.last_rebuild_stats(), eng.last_visibility_stats(), eng.last_rebuild_detail()
    assert (vs.pairs, vs.pairs_visible, vs.forced_rebuild) == (V.POOL, live, 0)
    if live < 2:
        assert (rs.rebuilt, rs.reason) == (0, A.RT_REBUILD_NO_TREE)
        assert vs.pairs_in_tree == V.POOL and vs.fit_complete == 1     # the build's tree stays, refit
    else:
        assert (rs.rebuilt, rs.reason) == (1, A.RT_REBUILD_NONE)
        assert dt.builder == (2 if builder == "clustered" else 1)
        assert vs.pairs_in_tree == vs.pairs_visible == live and vs.fit_complete == 1
        d = eng.wide_read()
        fp = np.asarray(d["fpairs"], np.int64).reshape(-1, 2)
        want = sorted(int(p) for p in np.flatnonzero(np.isin(fp[:, 1], [eng.instance_of(i) for i in range(live)])))
        assert sorted(_fit_terminals(d)) == want, "the tree's pair refs are not the visible instances' pairs, once each"
        after = eng.fit_cost()
        print(f"live {live}, builder {builder}: fit_cost {before:.4f} -> {after:.4f}")
        assert after < before
    _assert_rays(eng, ref, O, D, tmax)
    eng.set_option("fit", 0)
    _assert_rays(eng, ref, O, D, tmax)
    eng.close()


@pytest.mark.parametrize("builder", [True, "clustered"])
def test_compaction_of_seventeen_thousand_pairs(builder):
    c = V.case("many_pairs")
    O, D, tmax = c.rays
    eng, ref, before = _compacting_commit(c, "every_other", builder, ("many_pairs", "every_other"))
    rs, vs = eng.last_rebuild_stats(), eng.last_visibility_stats()
    assert (rs.rebuilt, rs.reason) == (1, A.RT_REBUILD_NONE)
    assert vs.pairs == 270 * 64 and vs.pairs_in_tree == vs.pairs_visible == 135 * 64
    d = eng.wide_read()
    fp = np.asarray(d["fpairs"], np.int64).reshape(-1, 2)
    shown = [eng.instance_of(i) for i in range(270) if i not in c.states["every_other"]]
    assert sorted(_fit_terminals(d)) == sorted(int(p) for p in np.flatnonzero(np.isin(fp[:, 1], shown)))
    after = eng.fit_cost()
    print(f"builder {builder}: fit_cost {before:.4f} -> {after:.4f}, nodes {rs.nodes_before} -> {rs.nodes_after}")
    assert after < before
    _assert_rays(eng, ref, O, D, tmax)
    eng.close()


# ---------------------------------------------------------------- 7. forced rebuild
def test_showing_what_the_tree_lacks_rebuilds_on_its_own():
    c = V.case("pool")
    O, D, tmax = c.rays
    eng = _engine(c.scene)
    _set_hidden(eng, c.states["live255"], rebuild=True)
    assert eng.last_visibility_stats().pairs_in_tree == 255
    cs, vs = _set_hidden(eng, frozenset())                      # a plain commit
    rs, dt = eng.last_rebuild_stats(), eng.last_rebuild_detail()
    assert (vs.forced_rebuild, vs.fit_complete, vs.pairs_in_tree, vs.shown) == (1, 1, V.POOL, 45)
    assert (rs.rebuilt, rs.reason, rs.pairs, dt.builder) == (1, A.RT_REBUILD_NONE, V.POOL, 1)
    assert sorted(_fit_terminals(eng.wide_read())) == list(range(V.POOL))
    _assert_rays(eng, _ref(eng, ("pool", 300), O, D, tmax), O, D, tmax)
    # hiding again needs no rebuild: the tree holds every visible pair
    cs, vs = _set_hidden(eng, c.states["live257"])
    assert (vs.forced_rebuild, vs.fit_complete, eng.last_rebuild_stats().rebuilt) == (0, 1, 0)
    _assert_rays(eng, _ref(eng, ("pool", 257), O, D, tmax), O, D, tmax)
    eng.close()


def test_a_forced_rebuild_whose_guard_trips_leaves_the_walks_on_the_marker_tree():
    c = V.case("pool")
    O, D, tmax = c.rays
    eng = _engine(c.scene)
    _set_hidden(eng, c.states["live255"], rebuild=True)
    cap = eng.get_option("rebuild_depth_cap")
    eng.set_unsafe_option("rebuild_depth_cap", 2)
    cs, vs = _set_hidden(eng, frozenset())
    rs = eng.last_rebuild_stats()
    assert (rs.rebuilt, rs.reason) == (0, A.RT_REBUILD_TOO_DEEP)
    assert (vs.forced_rebuild, vs.fit_complete, vs.pairs_in_tree, vs.pairs_visible) == (0, 0, 255, V.POOL)
    ref = _ref(eng, ("pool", 300), O, D, tmax)
    _assert_rays(eng, ref, O, D, tmax)                           # option fit is on: the walks must not use the tree
    eng.set_unsafe_option("rebuild_depth_cap", cap)
    eng.commit(rebuild=True)
    vs = eng.last_visibility_stats()
    assert (eng.last_rebuild_stats().rebuilt, vs.fit_complete, vs.pairs_in_tree) == (1, 1, V.POOL)
    _assert_rays(eng, ref, O, D, tmax)
    eng.close()


# ---------------------------------------------------------------- 8. the constants follow visibility
def _mismatch(eng, ref, O, D):
    to, po, no, mo = ref
    tg, pg, ng, mg = eng.trace_rays(O, D)
    bad = (tg.view(np.uint64) != to.view(np.uint64)) | (mg != mo)
    hit = np.isfinite(to) & np.isfinite(tg)
    return bad | (hit & ((pg != po).any(1) | (ng != no).any(1)))


def test_constants_follow_visibility_in_both_directions():
    c = V.case("far")
    O, D, tmax = c.rays
    Of, Df, tf = c.far_rays
    eng = _engine(c.scene)
    full = eng.wide_read()
    assert full["wide_coord"] > 9.0e5 and full["fit_coord"] > 9.0e5
    _set_hidden(eng, c.states["far_hidden"])
    _assert_rays(eng, _ref(eng, ("far", "far_hidden"), O, D, tmax), O, D, tmax)
    d = eng.wide_read()
    other = M.RayTracerEngine(eng.visible_scene(), dynamic=True)
    other.set_transform(0, other.scene.objects[0].transform)
    other.commit()
    e = other.wide_read()
    other.close()
    assert (d["wide_coord"], d["fit_coord"]) == (e["wide_coord"], e["fit_coord"]) and d["wide_coord"] < 100.0
    # shown again: the widening is the far mesh's again - exact with it, teeth without it
    _set_hidden(eng, frozenset())
    back = eng.wide_read()
    assert (back["wide_coord"], back["fit_coord"] >= full["fit_coord"]) == (full["wide_coord"], True)
    osc = oracle.OracleScene(eng.visible_scene())
    ref = osc.trace_rays(Of, Df)
    occ = osc.occluded_rays(Of, Df, tf)
    osc.close()
    assert np.isfinite(ref[0]).mean() > 0.3
    assert not _mismatch(eng, ref, Of, Df).any() and np.array_equal(eng.occluded_rays(Of, Df, tf), occ)
    _assert_rays(eng, _ref(eng, ("far", "all"), O, D, tmax), O, D, tmax)
    eng.set_unsafe_option("wide_delta_scale", 0)
    bad = _mismatch(eng, ref, Of, Df)
    print(f"far mesh shown, no widening: {int(bad.sum())} of {len(Of)} closest hits differ")
    assert bad.any(), "no mismatch without the widening: the set does not reach the bound"
    eng.close()


# ---------------------------------------------------------------- 9. with the other commits
@pytest.mark.parametrize("walk", ["transformed", "transformed_binary"])
def test_visibility_transforms_and_positions_in_one_commit_and_a_hidden_pose(walk):
    sc, (O, D, tmax), steps = V.combined()
    eng = _engine(sc, walk, deformable=True)
    for k, st in enumerate(steps):
        for i, f in st["vis"].items():
            eng.set_visible(i, f)
        for i, m in st["moves"].items():
            eng.set_transform(i, m)
        for i, p in st["positions"].items():
            eng.set_positions(i, p)
        cs = eng.commit()
        vs = eng.last_visibility_stats()
        assert cs.instances_moved == len(st["moves"]) and vs.visible == 6 - len(st["hidden"])
        assert eng.last_deform_stats().meshes_deformed == len(st["positions"])
        assert [eng.is_visible(i) for i in range(6)] == [i not in st["hidden"] for i in range(6)]
        ref = _ref(eng, ("combined", k), O, D, tmax, True)
        _assert_rays(eng, ref, O, D, tmax)
        _assert_frame(eng, ref)
        # rt_scene_instance_bounds keeps reporting the box the instance has or would have
        tr = V.object_triangles(eng.scene, 2)
        lo, hi = eng.instance_bounds(eng.instance_of(2))
        assert np.all(lo <= tr.min(axis=(0, 1)) + 1e-9) and np.all(hi >= tr.max(axis=(0, 1)) - 1e-9)
        # ... and lies inside AABB.transformed of the mesh's whole local box (every triangle's box does)
        p = np.asarray(eng.scene.objects[2].positions, np.float64)
        olo, ohi = W.aabb_transformed(p.min(axis=0)[None], p.max(axis=0)[None], np.asarray(eng.scene.objects[2].transform))
        assert np.all(lo >= olo[0] - 1e-9) and np.all(hi <= ohi[0] + 1e-9)
    eng.close()


# ---------------------------------------------------------------- 10. queries
def test_queries_keep_their_indices_on_host_and_device_and_with_declared_bounds():
    import torch
    c = V.case("posed")
    O, D, tmax = c.rays
    n = len(O)
    eng = _engine(c.scene)
    inst = [eng.instance_of(i) for i in range(12)]
    _set_hidden(eng, c.states["third"])
    assert [eng.instance_of(i) for i in range(12)] == inst
    ref = _ref(eng, ("posed", "third"), O, D, tmax, True)
    (to, po, no, mo), oo = ref["rays"]
    want = ("t", "uv", "ids", "point", "normal", "flags")
    h = eng.query_closest(O, D, want=want)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    g = eng.query_closest(dev(O), dev(D), want=want)
    go = eng.query_occluded(dev(O), dev(D), dev(tmax))
    torch.cuda.synchronize()
    for f in want:
        a, b = getattr(h, f), getattr(g, f).cpu().numpy()
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), f
    assert np.array_equal(h.t.view(np.uint64), to.view(np.uint64)) and np.array_equal(h.ids[:, 3], mo)
    ho = eng.query_occluded(O, D, tmax)
    assert np.array_equal(ho.astype(bool), oo) and np.array_equal(ho, go.cpu().numpy())
    hit = np.isfinite(to)
    assert np.array_equal(h.point[hit], po[hit]) and (h.ids[~hit] == -1).all()
    # the ids name visible objects by their unchanged indices, and the hit lies on the named object
    objs = set(int(x) for x in h.ids[hit, 0])
    assert objs and not (objs & c.states["third"])
    for oi in objs:
        rows = np.flatnonzero(hit & (h.ids[:, 0] == oi))
        assert (h.ids[rows, 2] == inst[oi]).all()
        t1 = V.DS.closest_gap(np.concatenate([V.object_triangles(eng.scene, oi)] * 2), O[rows], D[rows])[0]
        assert np.allclose(t1, to[rows], rtol=1e-9, atol=0.0), oi
    # declared bounds: the same answers, nothing flagged beyond validity
    P = V.all_triangles(c.scene).reshape(-1, 3)
    ctr = 0.5 * (P.min(0) + P.max(0))
    b = (float(np.linalg.norm(O - ctr, axis=1).max() * 1.001 + np.abs(P - ctr).max()), float(np.abs(O).max()),
         float(np.linalg.norm(D, axis=1).max() * 1.001))
    hb = eng.query_closest(O, D, want=want, bounds=b)
    assert np.array_equal(hb.t.view(np.uint64), to.view(np.uint64)) and np.array_equal(hb.ids, h.ids) and (hb.flags <= 1).all()
    assert np.array_equal(eng.query_occluded(O, D, tmax, bounds=b).astype(bool), oo)
    eng.close()


# ---------------------------------------------------------------- 11. refusals and ordering
def test_refusals_and_ordering():
    c = V.case("posed")
    O, D, tmax = c.rays
    lib = M.load_library()
    static = M.RayTracerEngine(copy.deepcopy(c.scene))
    flags = (A.C.c_uint8 * 12)(*([0] * 12))
    assert lib.rt_scene_set_instance_visible(static._h, 0, 0) == A.RT_ERR_UNSUPPORTED
    assert lib.rt_scene_set_instances_visible(static._h, 0, 12, flags) == A.RT_ERR_UNSUPPORTED
    static.close()
    eng = _engine(c.scene)
    for k in (-1, 12, 1 << 30):
        assert lib.rt_scene_set_instance_visible(eng._h, k, 0) == A.RT_ERR_INVALID_ARG
    for first, count in ((-1, 2), (0, 13), (11, 2), (0, -1), (12, 1)):
        assert lib.rt_scene_set_instances_visible(eng._h, first, count, flags) == A.RT_ERR_INVALID_ARG
    assert lib.rt_scene_set_instances_visible(eng._h, 0, 12, None) == A.RT_ERR_INVALID_ARG
    cs = eng.commit()                                            # nothing was staged
    vs = eng.last_visibility_stats()
    assert (vs.visible, vs.hidden, vs.shown) == (12, 0, 0)
    ref_all = _ref(eng, ("posed", "all"), O, D, tmax, True)
    _assert_rays(eng, ref_all, O, D, tmax)
    # a second call for the same instance replaces the first; staging alone changes nothing
    eng.set_visible(11, False)
    eng.set_visible(11, True)
    eng.set_visible_many(sorted(c.states["third"]), False)
    _assert_rays(eng, ref_all, O, D, tmax)
    # a commit beside a submitted render: BUSY, the staging kept
    h, w = V.FRAME[1], V.FRAME[0]
    rgb = M.pinned_array((h, w, 3), np.float64)
    ticket = eng.submit_into(0, 0, 1, rgb, None)
    eng.set_visible(0, True)                                     # staging is legal while a render is in flight
    with pytest.raises(M.RenderError) as e:
        eng.commit()
    assert e.value.code == A.RT_ERR_BUSY
    eng.wait(ticket)
    assert float(np.abs(rgb - ref_all["frame"][0]).max()) <= 1e-5
    eng.commit()
    vs = eng.last_visibility_stats()
    assert (vs.visible, vs.hidden, vs.shown) == (8, 4, 0)
    ref_third = _ref(eng, ("posed", "third"), O, D, tmax, True)
    _assert_rays(eng, ref_third, O, D, tmax)
    # a refused commit (a transform beyond 1e30 staged with it) leaves visibility as it was
    before = eng.wide_read()
    eng.set_visible_many(range(12), True)
    pose = tuple(eng.scene.objects[3].transform)
    with pytest.raises(M.RenderError) as e:
        eng.set_transform(3, V.DS.m16(np.eye(3), (1.0e31, 0.0, 0.0)))
        eng.commit()
    assert e.value.code == A.RT_ERR_INVALID_ARG
    eng.scene.objects[3].transform = pose                        # the mirror follows staging: put it back
    assert [eng.is_visible(i) for i in range(12)] == [i not in c.states["third"] for i in range(12)]
    assert W.same_dump(before, eng.wide_read()) is None
    _assert_rays(eng, ref_third, O, D, tmax)
    assert eng.commit().instances_moved == 0 and eng.last_visibility_stats().visible == 8   # the staging was dropped
    eng.close()
