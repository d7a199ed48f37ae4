"""Ray masks (rtcore.h "ray masks"): every instance carries 32 mask bits, a masked query
gives every ray 32 mask bits, and a ray sees an instance iff the two share a bit and the instance is
visible.  No commit is involved.

Every comparison of hits is with the oracle on the scene that holds only the objects the ray sees
(engine.visible_subset, which RayTracerEngine.masked_scene calls with the committed flags and the
masks), built fresh; none is with the code under test.  The scenes, states and ray sets are those of
tests/visibility_scenes.py and tests/mask_scenes.py; tests/test_visibility_inputs.py and
tests/test_mask_inputs.py show on the CPU that each is free of equal-t ties between instances."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_rays as GR                                                        # noqa: E402
import mask_scenes as MS                                                         # noqa: E402
import visibility_scenes as V                                                    # noqa: E402
from test_gpu_visibility import WALKS                                            # noqa: E402

pytestmark = pytest.mark.gpu

ALL = ("t", "uv", "ids", "point", "normal", "flags")
STATIC_WALKS = {"wide": ({}, 1), "unified": ({"wide": 0}, 1), "general": ({"unified": 0}, 0)}


# ---------------------------------------------------------------- helpers
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _engine(sc, walk="transformed", devices=None, dynamic=True, options=None):
    eng = M.RayTracerEngine(copy.deepcopy(sc), devices, dynamic=dynamic)
    for k, v in (WALKS[walk] if options is None else options).items():
        eng.set_option(k, v)
    return eng


def _sig(sc):
    return [(type(o).__name__, getattr(o, "id", None), tuple(o.transform)) for o in sc.objects]


_REF = {}


def _ref(key, sc, O, D, tmax, tmin=None):
    """The oracle's answers for scene `sc`, once per key: ((t, point, normal, material), occluded)."""
    if key not in _REF:
        osc = oracle.OracleScene(sc)
        _REF[key] = dict(sig=_sig(sc), rays=(osc.trace_rays(O, D, tmin), osc.occluded_rays(O, D, tmax)))
        osc.close()
    assert _REF[key]["sig"] == _sig(sc), "another scene under the same key"
    return _REF[key]["rays"]


def _dev(a, dtype=np.float64):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda:0")


def _dev_mask(mask):
    """A per-ray mask array as the int32 tensor whose bits are the masks; an int stays an int."""
    return mask if isinstance(mask, int) else _dev(np.ascontiguousarray(mask, np.uint32).view(np.int32), np.int32)


def _both(eng, O, D, tmax, mask, tmin=None, **kw):
    """query_closest and query_occluded with `mask` from host arrays and from device tensors: the two
    paths agree bit for bit; returns the host path's (RayHits, occluded)."""
    import torch
    h = eng.query_closest(O, D, tmin, mask=mask, want=ALL, **kw)
    g = eng.query_closest(_dev(O), _dev(D), _dev(tmin), mask=_dev_mask(mask), want=ALL, **kw)
    oh = eng.query_occluded(O, D, tmax, mask=mask, **kw)
    og = eng.query_occluded(_dev(O), _dev(D), _dev(tmax), mask=_dev_mask(mask), **kw)
    torch.cuda.synchronize()
    for f in ALL:
        assert _same(getattr(h, f), getattr(g, f).cpu().numpy()), f"host and device paths differ in {f}"
    assert oh.dtype == np.uint8 and _same(oh, og.cpu().numpy()), "host and device paths differ in the occlusion"
    return h, oh


def _assert_group(eng, h, occ, ref, idx, objects):
    """Rays `idx` of the answers (h, occ) against rays `idx` of the oracle's `ref`; every hit names an
    object of `objects` (the ones these rays see) and that object's instance."""
    (to, po, no, mo), oo = ref
    to, po, no, mo, oo = to[idx], po[idx], no[idx], mo[idx], oo[idx]
    t, uv, ids, flags = h.t[idx], h.uv[idx], h.ids[idx], h.flags[idx]
    hit = np.isfinite(to)
    assert _same(t, to), f"t differs on {int((_bits(t) != _bits(to)).sum())} of {len(to)} rays"
    assert np.array_equal(ids[:, 3], mo)
    assert _same(h.point[idx][hit], po[hit]) and _same(h.normal[idx][hit], no[hit])
    assert np.array_equal(flags, hit.astype(np.uint8) * A.RT_HIT_VALID)
    assert (ids[~hit] == -1).all() and not uv[~hit].any()
    assert not h.point[idx][~hit].any() and not h.normal[idx][~hit].any()
    assert (uv[hit] >= 0).all() and (uv[hit].sum(axis=1) <= 1).all()
    assert set(np.unique(ids[hit, 0])) <= set(objects), "a hit on an object the ray does not see"
    inst = np.array([eng.instance_of(i) for i in range(len(eng.scene.objects))])
    assert np.array_equal(ids[hit, 2], inst[ids[hit, 0]])
    assert np.array_equal(occ[idx].astype(bool), oo), f"occlusion differs on {int((occ[idx].astype(bool) != oo).sum())} rays"
    assert occ[idx].max(initial=0) <= 1


def _visible_objects(case, state):
    return [i for i in range(len(case.scene.objects)) if i not in case.states[state]]


def _posed_refs(c, states=MS.POSED_STATES, key="posed"):
    O, D, tmax = c.rays
    return {s: _ref((key, s), c.visible(s), O, D, tmax) for s in states}


def _check_states_per_ray(eng, c, states, refs, **kw):
    """Ray i carries mask 1 << (i % len(states)): every wave mixes the states."""
    O, D, tmax = c.rays
    n, k = len(O), len(states)
    mask = (np.uint32(1) << (np.arange(n) % k).astype(np.uint32)).astype(np.uint32)
    h, occ = _both(eng, O, D, tmax, mask, **kw)
    for s, state in enumerate(states):
        _assert_group(eng, h, occ, refs[state], np.arange(s, n, k), _visible_objects(c, state))
    return h, occ


# ---------------------------------------------------------------- 1. every transformed walk
@pytest.mark.parametrize("walk", list(WALKS))
def test_every_walk_per_ray_and_batch_masks(walk):
    c = V.case("posed")
    O, D, tmax = c.rays
    refs = _posed_refs(c)
    eng = _engine(c.scene, walk)
    masks = MS.state_masks(c, MS.POSED_STATES)
    # before any mask is set there is no table: every instance is all-ones, every ray mask sees all
    h, occ = _both(eng, O, D, tmax, 0x80000000)
    _assert_group(eng, h, occ, refs["all"], np.arange(len(O)), range(12))
    eng.set_mask_many(range(12), masks)
    assert [eng.mask_of(i) for i in range(12)] == masks
    for s, state in enumerate(MS.POSED_STATES):
        assert _sig(eng.masked_scene(1 << s)) == _sig(c.visible(state))
    _check_states_per_ray(eng, c, MS.POSED_STATES, refs)
    st = eng.last_query_stats()
    assert (st.rays, st.out_of_bounds, st.non_finite) == (len(O), 0, 0)
    for s, state in enumerate(MS.POSED_STATES):                        # a batch mask, one call per state
        h, occ = _both(eng, O, D, tmax, 1 << s)
        _assert_group(eng, h, occ, refs[state], np.arange(len(O)), _visible_objects(c, state))
        if state == "none":
            assert np.isinf(h.t).all() and (h.ids == -1).all() and not h.flags.any() and not occ.any()
    h, occ = _both(eng, O, D, tmax, 0)                                 # mask 0 misses, unflagged, counted
    assert np.isinf(h.t).all() and (h.ids == -1).all() and not h.flags.any() and not occ.any()
    st = eng.last_query_stats()
    assert (st.rays, st.hits, st.out_of_bounds, st.non_finite) == (len(O), 0, 0, 0)
    eng.close()


# ---------------------------------------------------------------- 2. every object kind
@pytest.mark.parametrize("walk", ["transformed", "nested"])
def test_every_object_kind_masks(walk):
    c = V.case("kinds")
    O, D, tmax = c.rays
    eng = _engine(c.scene, walk)
    eng.set_mask_many(range(6), [1 << i for i in range(6)])            # one bit per object
    for state, hidden in c.states.items():
        m = sum(1 << i for i in range(6) if i not in hidden)
        assert _sig(eng.masked_scene(m)) == _sig(c.visible(state))
        h, occ = _both(eng, O, D, tmax, m)
        _assert_group(eng, h, occ, _ref(("kinds", state), c.visible(state), O, D, tmax), np.arange(len(O)),
                      _visible_objects(c, state))
    eng.close()


# ---------------------------------------------------------------- 3. parts of a TLAS leaf
@pytest.mark.parametrize("walk", ["transformed", "transformed_tw", "transformed_binary"])
def test_parts_of_a_tlas_leaf_per_ray(walk):
    c = V.case("leaf6")
    states = ("some_of_leaf", "whole_leaf", "group_b")
    eng = _engine(c.scene, walk)
    eng.set_mask_many(range(len(c.scene.objects)), MS.state_masks(c, states))
    _check_states_per_ray(eng, c, states, _posed_refs(c, states, "leaf6"))
    eng.close()


# ---------------------------------------------------------------- 4. identity walks
@pytest.mark.parametrize("walk", list(STATIC_WALKS))
def test_identity_walks_per_ray(walk):
    c = MS.baked_posed()
    options, walk_id = STATIC_WALKS[walk]
    eng = _engine(c.scene, dynamic=False, options=options)
    eng.set_mask_many(range(12), MS.state_masks(c, MS.POSED_STATES))
    _check_states_per_ray(eng, c, MS.POSED_STATES, _posed_refs(c, key="baked"))
    assert eng.last_query_stats().walk == walk_id
    assert _sig(eng.masked_scene(2)) == _sig(c.visible("third"))       # a static scene: masks alone select
    eng.close()


# ---------------------------------------------------------------- 5. ties keep the mask
@pytest.mark.parametrize("walk", ["transformed", "transformed_tw", "transformed_binary", "wide"])
def test_ties_keep_the_mask(walk):
    """Rays that meet A where two of its triangles give the same t are re-walked in the reference's
    order; B lies in front of A, so a re-walk that forgot the mask would answer with B."""
    baked = walk == "wide"
    sc = MS.stacked(baked)
    O, D, tmax = MS.stacked_rays()
    eng = _engine(sc, dynamic=False, options={}) if baked else _engine(sc, walk)
    eng.set_mask(0, 1)
    eng.set_mask(1, 2)
    for name, hidden in MS.STACKED_SETS.items():
        m = MS.STACKED_MASK[name]
        assert _sig(eng.masked_scene(m)) == _sig(MS.subset(sc, hidden))
        ref = _ref(("stacked", baked, name), MS.subset(sc, hidden), O, D, tmax)
        h, occ = _both(eng, O, D, tmax, m)
        _assert_group(eng, h, occ, ref, np.arange(len(O)), [i for i in (0, 1) if i not in hidden])
        hit = np.isfinite(ref[0][0])
        assert hit.sum() >= 50
        if name != "AB":                                               # ids: every hit is on the one object seen
            assert (h.ids[hit, 0] == (0 if name == "A" else 1)).all()
    if baked:
        assert eng.last_query_stats().walk == 1
    eng.close()


# ---------------------------------------------------------------- 6. seams
def test_launch_seams_and_small_batches():
    c = V.case("posed")
    O, D, tmax = c.rays
    refs = _posed_refs(c)
    eng = _engine(c.scene)
    eng.set_mask_many(range(12), MS.state_masks(c, MS.POSED_STATES))
    eng.set_option("query_batch", 64)                                  # 19 launches, offsets into the mask array
    _check_states_per_ray(eng, c, MS.POSED_STATES, refs)
    assert eng.last_query_stats().launches == (len(O) + 63) // 64
    mask = (np.uint32(1) << (np.arange(len(O)) % 4).astype(np.uint32)).astype(np.uint32)
    for n in (1, 63, 64, 65):
        h, occ = _both(eng, O[:n], D[:n], tmax[:n], mask[:n])
        for s, state in enumerate(MS.POSED_STATES):
            idx = np.arange(s, n, 4)
            if len(idx):
                _assert_group(eng, h, occ, refs[state], idx, _visible_objects(c, state))
    eng.close()


def test_masks_with_declared_bounds_flag_as_unmasked():
    """A mask array together with declared bounds: rays beyond the bounds and non-finite rays come back
    flagged and untraced, and their neighbours' answers are the oracle's."""
    c = V.case("posed")
    O, D, tmax = c.rays
    refs = _posed_refs(c)
    eng = _engine(c.scene)
    eng.set_mask_many(range(12), MS.state_masks(c, MS.POSED_STATES))
    eng.query_closest(O, D, want=("t",))                               # the exact maxima of the clean batch
    b = eng.last_query_stats().bounds
    bounds = (b.origin_reach, b.origin_coord, b.dir_norm)
    O2, D2 = O.copy(), D.copy()
    oob, nonf = np.arange(5, len(O), 97), np.arange(11, len(O), 131)
    O2[oob] *= 1.0e6
    D2[nonf[::2], 1] = np.nan
    O2[nonf[1::2], 0] = np.inf
    mask = (np.uint32(1) << (np.arange(len(O)) % 4).astype(np.uint32)).astype(np.uint32)
    h, occ = _both(eng, O2, D2, tmax, mask, bounds=bounds)
    bad = np.zeros(len(O), bool)
    bad[oob] = bad[nonf] = True
    assert (h.flags[oob] == A.RT_HIT_OUT_OF_BOUNDS).all() and (h.flags[nonf] == A.RT_HIT_NON_FINITE).all()
    assert np.isinf(h.t[bad]).all() and (h.ids[bad] == -1).all() and (occ[bad] == 2).all()
    st = eng.last_query_stats()
    assert (st.rays, st.out_of_bounds, st.non_finite, st.reduced) == (len(O), len(oob), len(nonf), 0)
    for s, state in enumerate(MS.POSED_STATES):
        idx = np.arange(s, len(O), 4)
        _assert_group(eng, h, occ, refs[state], idx[~bad[idx]], _visible_objects(c, state))
    eng.close()


# ---------------------------------------------------------------- 7. masks and commits
def test_masks_and_commits():
    c = V.case("posed")
    O, D, tmax = c.rays
    refs = _posed_refs(c)
    n = len(O)
    eng = _engine(c.scene, devices=[0, 0])
    masks = MS.state_masks(c, MS.POSED_STATES)
    eng.set_mask_many(range(12), masks)
    # hide the objects of "third" by commit: a ray of state s sees visible(s) without them
    eng.set_visible_many(range(12), [i not in c.states["third"] for i in range(12)])
    eng.commit()
    assert _sig(eng.masked_scene(4)) == _sig(c.visible("one"))         # "one" masked, "third" hidden: object 11
    seen = {"all": "third", "third": "third", "one": "one", "none": "none"}
    for slot in (0, 1):                                                # two replicas answer alike
        mask = (np.uint32(1) << (np.arange(n) % 4).astype(np.uint32)).astype(np.uint32)
        h, occ = _both(eng, O, D, tmax, mask, slot=slot)
        for s, state in enumerate(MS.POSED_STATES):
            _assert_group(eng, h, occ, refs[seen[state]], np.arange(s, n, 4), _visible_objects(c, seen[state]))
    # a mask set while the instance is hidden holds when it is shown
    eng.set_mask(2, 0)
    eng.set_visible_many(range(12), True)
    eng.commit()
    assert eng.mask_of(2) == 0 and [eng.mask_of(i) for i in range(12) if i != 2] == [m for i, m in enumerate(masks) if i != 2]
    without2 = eng.masked_scene(1)
    assert _sig(without2) == _sig(MS.subset(c.scene, {2}))
    for slot in (0, 1):
        h, occ = _both(eng, O, D, tmax, 1, slot=slot)
        _assert_group(eng, h, occ, _ref(("posed", "without2"), without2, O, D, tmax), np.arange(n),
                      [i for i in range(12) if i != 2])
    # an unmasked query ignores instance masks: object 2, mask 0, is there
    hu = eng.query_closest(O, D, want=ALL)
    ou = eng.query_occluded(O, D, tmax)
    assert _sig(eng.visible_scene()) == _sig(c.visible("all"))
    _assert_group(eng, hu, ou, refs["all"], np.arange(n), range(12))
    assert (hu.ids[:, 0] == 2).any()
    # masks survive commits of every kind: a transform, a rebuild, a clustered rebuild
    m = np.asarray(eng.scene.objects[11].transform, np.float64).reshape(4, 4).T.copy()
    m[:3, 3] += (1.0, 0.5, -1.0)
    eng.set_transform(11, tuple(float(x) for x in m.T.reshape(-1)))
    eng.commit()
    moved = eng.masked_scene(4)
    assert len(moved.objects) == 1 and _sig(moved) != _sig(c.visible("one"))
    ref = _ref(("posed", "one moved"), moved, O, D, tmax)
    assert np.isfinite(ref[0][0]).mean() > 0.05
    for rebuild in (None, True, "clustered"):
        if rebuild is not None:
            eng.commit(rebuild=rebuild)
            assert eng.last_rebuild_stats().rebuilt == 1
        assert [eng.mask_of(i) for i in range(12) if i != 2] == [mm for i, mm in enumerate(masks) if i != 2]
        h, occ = _both(eng, O, D, tmax, 4)
        _assert_group(eng, h, occ, ref, np.arange(n), [11])
    eng.close()


# ---------------------------------------------------------------- 8. first-hit buffers
_CENTRE = {}


def _centre_rays(sc):
    if "r" not in _CENTRE:
        _CENTRE["r"] = GR.first_rays(sc, 0, 0, 1, centre=True)
    return _CENTRE["r"]


def _torch_out(rows, width, names):
    import torch
    fields = dict(M.engine.FirstHits.RAYS, **M.engine.RayHits.FIELDS)
    dt = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}
    return {f: torch.full((rows, width, fields[f][0]) if fields[f][0] > 1 else (rows, width), 77, dtype=dt[fields[f][1]],
                          device="cuda:0") for f in names}


@pytest.mark.parametrize("centre", [True, False])
def test_first_hits_masked(centre):
    import torch
    c = V.case("posed")
    W, H = V.FRAME
    eng = _engine(c.scene)
    eng.set_mask_many(range(12), MS.state_masks(c, MS.POSED_STATES))
    names = ("origins", "dirs", "tmin", "time") + ALL
    for s, state in ((0, "all"), (1, "third"), (2, "one"), (3, "none")):
        m = 1 << s
        fh = eng.first_hits_masked(m, want=("rays",) + ALL, centre=centre)
        assert fh.rows == H and fh.hits.t.shape == (H, W)
        O, D = fh.origins.reshape(-1, 3), fh.dirs.reshape(-1, 3)
        tmin, time = fh.tmin.reshape(-1), fh.time.reshape(-1)
        # the record is the masked query's of the exported ray, bit for bit
        q = eng.query_closest(O, D, tmin, time, mask=m, want=ALL)
        for f in ALL:
            assert _same(getattr(fh.hits, f).reshape(getattr(q, f).shape), getattr(q, f)), f
        st = eng.last_query_stats()
        if centre:                                                     # ... and the oracle's of the masked scene
            r = _centre_rays(c.scene)
            Oc, Dc, tc = r["origins"].reshape(-1, 3), r["dirs"].reshape(-1, 3), r["tmin"].reshape(-1)
            assert np.abs(O - Oc).max() <= 1e-12 and np.abs(D - Dc).max() <= 1e-12 and not time.any()
            vs = eng.masked_scene(m)
            assert _sig(vs) == _sig(c.visible(state))
            ref = _ref(("posed centre", state), vs, O, D, np.full(len(O), 1e3), tmin)
            (to, po, no, mo) = ref[0]
            hit = np.isfinite(to)
            assert _same(q.t, to) and np.array_equal(q.ids[:, 3], mo)
            assert _same(q.point[hit], po[hit]) and _same(q.normal[hit], no[hit])
            assert set(np.unique(q.ids[hit, 0])) <= set(_visible_objects(c, state))
            assert hit.any() == (state != "none")
        # device tensors, both lane mappings, and the frame layout: the same record
        for tiles in (0, 1):
            eng.set_option("gbuffer_tiles", tiles)
            out = _torch_out(H, W, names)
            eng.first_hits_masked(m, centre=centre, out=out)
            torch.cuda.synchronize()
            for f in ALL:
                assert _same(out[f].cpu().numpy(), getattr(fh.hits, f)), (tiles, f)
            assert _same(out["origins"].cpu().numpy(), fh.origins) and _same(out["tmin"].cpu().numpy(), fh.tmin)
        part = eng.first_hits_masked(m, 0, 1, 2, want=("t", "ids"), centre=centre, frame_layout=True)
        rows = [j for k in range(1, (H + 7) // 8, 2) for j in range(8 * k, min(8 * k + 8, H))]
        assert _same(part.hits.t[rows], fh.hits.t[rows]) and _same(part.hits.ids[rows], fh.hits.ids[rows])
        packed = eng.first_hits_masked(m, 0, 1, 2, want=("t",), centre=centre)
        assert _same(packed.hits.t, fh.hits.t[rows])
    eng.close()


# ---------------------------------------------------------------- 9. refusals and accounting
def test_refusals_leave_everything_untouched():
    import torch
    c = V.case("posed")
    O, D, tmax = c.rays
    n = len(O)
    lib = M.load_library()
    eng = _engine(c.scene, devices=[0, 0])
    ni = eng.info().instances
    assert ni == 12
    # the table: allocated by the first call, once, 4 bytes per instance (per replica)
    _both(eng, O, D, tmax, 1)                                          # (asking for ids uploads the face table, once)
    b0 = eng.info().device_bytes
    _both(eng, O, D, tmax, 1)
    assert eng.info().device_bytes == b0, "a masked query allocates no table"
    buf = (C.c_uint32 * 12)(*([5] * 12))
    for first, count in ((-1, 2), (0, 13), (11, 2), (12, 1), (3, -1)):
        assert lib.rt_scene_set_instance_masks(eng.handle, first, count, buf) == A.RT_ERR_INVALID_ARG, (first, count)
    assert lib.rt_scene_set_instance_masks(eng.handle, 0, 3, None) == A.RT_ERR_INVALID_ARG
    got = C.c_uint32(9)
    assert lib.rt_scene_instance_mask(eng.handle, 12, C.byref(got)) == A.RT_ERR_INVALID_ARG and got.value == 9
    assert lib.rt_scene_instance_mask(eng.handle, 0, None) == A.RT_ERR_INVALID_ARG
    assert eng.info().device_bytes == b0 and all(eng.mask_of(i) == 0xFFFFFFFF for i in range(12))
    eng.set_mask(3, 6)
    b1 = eng.info().device_bytes
    assert b1 - b0 == 4 * ni
    eng.set_mask_many(range(12), 7)
    eng.set_mask(3, 6)
    assert eng.info().device_bytes == b1, "the table is allocated once"
    assert lib.rt_scene_set_instance_masks(eng.handle, 12, 0, None) == A.RT_OK          # an empty range inside the scene
    assert lib.rt_scene_set_instance_masks(eng.handle, 11, 2, buf) == A.RT_ERR_INVALID_ARG
    assert [eng.mask_of(i) for i in range(12)] == [7, 7, 7, 6] + [7] * 8
    # masked queries: a host array under RT_QUERY_DEVICE, and (with a second GPU) another device's array
    od, dd = _dev(O), _dev(D)
    t = torch.full((n,), 77.0, dtype=torch.float64, device="cuda:0")
    occ = torch.full((n,), 77, dtype=torch.uint8, device="cuda:0")
    rays = A.rt_ray_batch(od.data_ptr(), dd.data_ptr(), None, None)
    hb = A.rt_hit_batch()
    hb.t = t.data_ptr()
    host_masks = np.full(n, 1, np.uint32)
    wrong = [host_masks.ctypes.data]
    if torch.cuda.device_count() > 1:
        other = torch.ones(n, dtype=torch.int32, device="cuda:1")
        wrong.append(other.data_ptr())
    for p in wrong:
        rm = A.rt_ray_masks(p, 0, 0)
        assert lib.rt_query_closest_masked(eng.handle, 0, n, C.byref(rays), C.byref(hb), None, A.RT_QUERY_DEVICE, None,
                                           C.byref(rm)) == A.RT_ERR_UNSUPPORTED
        assert lib.rt_query_occluded_masked(eng.handle, 0, n, C.byref(rays), C.c_void_p(occ.data_ptr()), None, A.RT_QUERY_DEVICE, None,
                                            C.byref(rm)) == A.RT_ERR_UNSUPPORTED
    good = torch.ones(n, dtype=torch.int32, device="cuda:0")          # the same calls with a device array go through
    rm = A.rt_ray_masks(good.data_ptr(), 0, 0)
    assert lib.rt_query_occluded_masked(eng.handle, 0, n, C.byref(rays), C.c_void_p(occ.data_ptr()), None,
                                        A.RT_QUERY_DEVICE, None, C.byref(rm)) == A.RT_OK
    torch.cuda.synchronize()
    assert (occ <= 1).all()
    occ.fill_(77)
    rm = A.rt_ray_masks(None, 1, 0)
    assert lib.rt_query_closest_masked(eng.handle, 2, n, C.byref(rays), C.byref(hb), None, A.RT_QUERY_DEVICE, None,
                                       C.byref(rm)) == A.RT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (t == 77.0).all() and (occ == 77).all()
    with pytest.raises(ValueError):
        eng.query_closest(O, D, mask=np.ones(n - 1, np.uint32))
    with pytest.raises(ValueError):
        eng.query_closest(O, D, mask=1 << 32)
    with pytest.raises(ValueError):
        eng.first_hits_masked(-1)
    # masks == NULL is the unmasked call
    assert lib.rt_query_closest_masked(eng.handle, 0, n, C.byref(rays), C.byref(hb), None, A.RT_QUERY_DEVICE, None,
                                       None) == A.RT_OK
    torch.cuda.synchronize()
    assert _same(t.cpu().numpy(), _ref(("posed", "all"), c.visible("all"), O, D, tmax)[0][0])
    # a lost scene (debug_fail_commit_step: a host-side early return that launches nothing)
    eng.set_transform(0, eng.scene.objects[0].transform)
    eng.set_unsafe_option("debug_fail_commit_step", 1)
    with pytest.raises(M.RenderError) as e:
        eng.commit()
    assert e.value.code == A.RT_ERR_DEVICE
    t.fill_(77.0)
    for call in (lambda: eng.query_closest(O, D, mask=1), lambda: eng.query_occluded(O, D, tmax, mask=1),
                 lambda: eng.first_hits_masked(1), lambda: eng.set_mask(0, 1)):
        with pytest.raises(M.RenderError) as e:
            call()
        assert e.value.code == A.RT_ERR_DEVICE
    assert lib.rt_query_closest_masked(eng.handle, 0, n, C.byref(rays), C.byref(hb), None, A.RT_QUERY_DEVICE, None,
                                       C.byref(rm)) == A.RT_ERR_DEVICE
    torch.cuda.synchronize()
    assert (t == 77.0).all() and eng.mask_of(0) == 7
    eng.close()
