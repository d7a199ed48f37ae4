"""First-hit buffers (rt_render_gbuffer): per pixel the first primary ray the render
casts and the record rt_query_closest returns for it.

1. The exported rays against the independent restatement tests/gbuffer_rays.py (which
   tests/test_gbuffer_inputs.py ties to the oracle's render on the CPU): time exactly, the origin
   exactly without a lens, the rest to 1e-12.  The bound is derived, not measured: the device
   normalises with v * (1 / sqrt), the restatement with v / sqrt; the chain from the camera constants
   to a direction or tmin is under 64 roundings of 2^-53 = 7.1e-15; its only cancellation is sp - eye,
   conditioned by |eye| / near_distance, which the test cameras keep <= 100: 7.1e-13 < 1e-12.  A wrong
   draw, seed or sub-cell moves a direction by about 1 / W = 0.03.
2. The records bit for bit against query_closest on the exported rays (same engine) and against the
   oracle's intersectTLAS on them, on every walk.
3. The render casts these rays: on the ambient scene every pixel of rt_render's FP64 frame is the
   colour the record's material names, bit for bit.
4. Layout and seams, 5. live scenes, 6. the contract (refusals, statistics, bytes, a lost scene, a
   degenerate camera)."""
import copy
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A
from myraytracer_amd import scenes
import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_rays as G                                                         # noqa: E402
import test_gpu_rays as R                                                        # noqa: E402

pytestmark = pytest.mark.gpu
RAYS = ("origins", "dirs", "tmin", "time")
REC = ("t", "uv", "ids", "point", "normal", "flags")
ALL = RAYS + REC
COLS = dict(M.engine.FirstHits.RAYS, **M.engine.RayHits.FIELDS)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _get(fh, name):
    a = getattr(fh if name in RAYS else fh.hits, name)
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


def _assert_equal(a, b, names=ALL, rows=slice(None), what=""):
    for f in names:
        assert _same(_get(a, f), _get(b, f)[rows]), f"{what}: {f} differs"


def _tensors(rows, W, names=ALL, fill=None):
    import torch
    dt = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}
    out = {}
    for f in names:
        cols, t = COLS[f]
        shape = (rows, W, cols) if cols > 1 else (rows, W)
        out[f] = torch.empty(shape, dtype=dt[t], device="cuda:0") if fill is None else \
            torch.full(shape, fill, dtype=dt[t], device="cuda:0")
    return out


def _with_camera(sc, cam):
    sc = copy.deepcopy(sc)
    sc.cameras = [cam]
    return sc


# ---------------------------------------------------------------- 1. rays against the restatement
@pytest.mark.parametrize("centre", [False, True])
@pytest.mark.parametrize("name", ["lookat", "lookat4", "nearplane", "dof"])
def test_rays_match_the_independent_restatement(name, centre):
    worst = {}
    for W, H in ((37, 21), (8, 8), (1, 1)):
        cam = G.cameras(W, H)[name]
        assert np.linalg.norm(cam.position) / cam.near_distance <= 100
        sc = _with_camera(G.ambient_scene(), cam)
        ref = G.first_rays(sc, centre=centre)
        with M.RayTracerEngine(copy.deepcopy(sc)) as eng:
            fh = eng.first_hits(want=("rays",), centre=centre)
        assert fh.origins.shape == (H, W, 3) and fh.time.shape == (H, W) and fh.hits.t is None
        lens = name == "dof" and not centre
        err = {"time": np.abs(fh.time - ref["time"]).max(),
               "dirs": np.abs(fh.dirs - ref["dirs"]).max(),
               "tmin": (np.abs(fh.tmin - ref["tmin"]) / np.abs(ref["tmin"])).max(),
               "origins": (np.abs(fh.origins - ref["origins"]).max(-1) / np.linalg.norm(ref["origins"], axis=-1)).max()}
        for k, v in err.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
        assert _same(fh.time, ref["time"]), "time is u32 * 2^-32: exact"
        if not lens:
            assert _same(fh.origins, ref["origins"])
        assert err["dirs"] <= 1e-12 and err["tmin"] <= 1e-12 and err["origins"] <= 1e-12, err
        assert np.abs(np.linalg.norm(fh.dirs, axis=-1) - 1.0).max() <= 2.0 ** -50
        assert (fh.tmin > 0).all() and ((fh.time == 0).all() if centre else (fh.time > 0).all())
    print(f"{name} centre={centre}: largest differences {worst}")


# ---------------------------------------------------------------- 2. records, bit for bit
def _special():
    sc = scenes.scaled(scenes.scene_c2(inline=True), 37, 21)
    base = sc.objects[0]
    base.motion_blur = (0.0, 0.2, 0.0)
    sc.objects = [base,
                  M.MeshInstance(id=11, base_mesh_id=base.id, material="1", motion_blur=(0.3, 0.0, 0.0),
                                 transform=(2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 3.0, 0.5, -2.0, 1)),
                  M.Sphere(center=(-2.5, 0.3, 0.5), radius=0.7, material="1"),
                  M.Plane(center=(0.0, -1.5, 0.0), normal=(0.0, 1.0, 0.0), material="1"),
                  M.Triangle(vertices=((-3, -1, -3), (3, -1, -3), (0, 2, -3.5)), material="1")]
    sc.cameras[0] = dataclasses.replace(sc.cameras[0], position=(0.5, 1.0, 7.5), fovy=60.0)
    return sc


_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        if name == "c2":
            sc = scenes.scaled(scenes.scene_c2(inline=True), 37, 21)
        elif name == "instances":
            sc = scenes.scaled(R._transformed_instances(), 37, 21)
            sc.cameras[0] = dataclasses.replace(sc.cameras[0], position=(0.5, 1.0, 9.0), fovy=55.0)
        else:
            sc = _special()
        _SCENES[name] = sc
    return copy.deepcopy(_SCENES[name])


def _assert_oracle(fh, sc):
    n = fh.rows * fh.width
    to, po, no, mo = oracle.OracleScene(sc).trace_rays(fh.origins.reshape(n, 3), fh.dirs.reshape(n, 3),
                                                       fh.tmin.reshape(n), fh.time.reshape(n))
    h = fh.hits
    hit = np.isfinite(to)
    assert _same(h.t.reshape(n), to), f"t differs on {int((_bits(h.t.reshape(n)) != _bits(to)).sum())} of {n} pixels"
    assert np.array_equal(h.ids.reshape(n, 4)[:, 3], mo)
    assert _same(h.point.reshape(n, 3)[hit], po[hit]) and _same(h.normal.reshape(n, 3)[hit], no[hit])
    assert np.array_equal(h.flags.reshape(n), hit.astype(np.uint8) * A.RT_HIT_VALID)
    assert (h.ids.reshape(n, 4)[~hit] == -1).all() and not h.point.reshape(n, 3)[~hit].any()
    return hit


RECORDS = [("c2", "wide", 1), ("c2", "unified", 1), ("c2", "general", 0), ("instances", "transformed", 3),
           ("instances", "transformed_tw", 2), ("special", "transformed", 2)]


@pytest.mark.parametrize("name,walk,walk_id", RECORDS)
def test_records_are_the_query_of_the_exported_rays(name, walk, walk_id):
    sc = _scene(name)
    eng = R._engine(_scene(name), walk)
    fh = eng.first_hits(want=ALL)
    st = eng.last_query_stats()
    n = fh.rows * fh.width
    assert (fh.rows, fh.width) == (21, 37) and fh.hits.ids.shape == (21, 37, 4)
    q = eng.query_closest(fh.origins.reshape(n, 3), fh.dirs.reshape(n, 3), fh.tmin.reshape(n), fh.time.reshape(n), want=REC)
    for f in REC:
        assert _same(_get(fh, f).reshape(getattr(q, f).shape), getattr(q, f)), f"{f} differs from the query's"
    # the bounds it reports can be declared to a query of these rays: nothing is flagged, the same records
    b = st.bounds
    qd = eng.query_closest(fh.origins.reshape(n, 3), fh.dirs.reshape(n, 3), fh.tmin.reshape(n), fh.time.reshape(n),
                           want=REC, bounds=(b.origin_reach, b.origin_coord, b.dir_norm))
    for f in REC:
        assert _same(getattr(qd, f), getattr(q, f)), f"{f} differs under the declared camera bounds"
    eng.close()
    hit = _assert_oracle(fh, sc)
    print(f"{name}/{walk}: {int(hit.sum())} of {n} pixels hit")
    assert hit.any() and (~hit).any()
    assert (st.rays, st.hits, st.non_finite, st.out_of_bounds, st.reduced, st.walk) == (n, int(hit.sum()), 0, 0, 0, walk_id)
    if name == "special":
        assert len(set(fh.time.ravel())) > n // 2, "time varies per pixel"


# ---------------------------------------------------------------- 3. the render casts these rays
def test_the_render_casts_these_rays():
    sc = G.ambient_scene()
    with M.RayTracerEngine(copy.deepcopy(sc)) as eng:
        rgb = eng.render_rows(0, want_rgba=False)[0]
        fh = eng.first_hits(want=("ids", "flags"))
    hit = (fh.hits.flags & A.RT_HIT_VALID) != 0
    want = G.ambient_colours(sc, fh.hits.ids[..., 3], hit)
    bad = (_bits(want) != _bits(rgb)).any(-1)
    assert rgb.shape == (21, 37, 3) and not bad.any(), f"{int(bad.sum())} pixels of the frame name another material"
    assert 0.1 <= (~hit).mean() <= 0.9 and len(set(fh.hits.ids[..., 0][hit])) == len(sc.objects)


# ---------------------------------------------------------------- 4. layout and seams
@pytest.fixture(scope="module")
def full():
    with M.RayTracerEngine(G.ambient_scene()) as eng:
        return eng.first_hits(want=ALL)


def _rows_of(first, step, H=21):
    return [j for c in range(first, (H + 7) // 8, step) for j in range(8 * c, min(8 * c + 8, H))]


@pytest.mark.parametrize("tiles", [1, 0])
def test_chunk_selections_and_the_frame_layout(full, tiles):
    import torch
    with M.RayTracerEngine(G.ambient_scene()) as eng:
        eng.set_option("gbuffer_tiles", tiles)
        for first, step in ((0, 1), (1, 2), (2, 3)):
            rows = _rows_of(first, step)
            h = eng.first_hits(0, first, step, want=ALL)
            assert h.rows == len(rows) == M.rows_for_chunks(21, first, step)
            _assert_equal(h, full, rows=rows, what=f"host {first, step}")
            g = eng.first_hits(0, first, step, out=_tensors(len(rows), 37))
            torch.cuda.synchronize()
            _assert_equal(g, h, what=f"device {first, step}")
            others = [j for j in range(21) if j not in rows]
            fr = eng.first_hits(0, first, step, frame_layout=True, out=_tensors(21, 37, fill=7))
            torch.cuda.synchronize()
            host = {f: np.full((21, 37, COLS[f][0]) if COLS[f][0] > 1 else (21, 37), 7, COLS[f][1]) for f in ALL}
            gb = A.rt_gbuffer()
            for f in ALL:
                setattr(gb if f in RAYS else gb.hits, M.engine.FirstHits.ABI.get(f, f), host[f].ctypes.data)
            assert M.load_library().rt_render_gbuffer(eng.handle, 0, 0, first, step, C.byref(gb),
                                                      A.RT_GBUFFER_FRAME_LAYOUT, None) == A.RT_OK
            for f in ALL:
                a = _get(fr, f)
                assert _same(a[rows], _get(full, f)[rows]) and _same(host[f][rows], _get(full, f)[rows]), (first, step, f)
                assert (a[others] == 7).all() and (host[f][others] == 7).all(), f"{f}: an unselected row was written"


def test_staging_passes_and_left_out_outputs(full):
    import torch
    with M.RayTracerEngine(G.ambient_scene()) as eng:
        for batch in (64, 192):
            eng.set_option("query_batch", batch)
            _assert_equal(eng.first_hits(want=ALL), full, what=f"query_batch {batch}")
            assert eng.last_query_stats().launches == (21 * 37 + batch - 1) // batch > 1
            _assert_equal(eng.first_hits(0, 1, 2, want=ALL), full, rows=_rows_of(1, 2), what=f"query_batch {batch}, (1, 2)")
        for drop in ALL:                                       # every single output left out in turn
            want = tuple(f for f in ALL if f != drop)
            h = eng.first_hits(want=want)
            g = eng.first_hits(out=_tensors(21, 37, want))
            torch.cuda.synchronize()
            assert _get(h, drop) is None and getattr(g if drop in RAYS else g.hits, drop) is None
            _assert_equal(h, full, want, what=f"host without {drop}")
            _assert_equal(g, full, want, what=f"device without {drop}")
        for rays in (eng.first_hits(want=("rays",)), eng.first_hits(want=("rays",), out=None, frame_layout=True),
                     eng.first_hits(out=_tensors(21, 37, RAYS))):      # rays only: the small kernel
            torch.cuda.synchronize()
            _assert_equal(rays, full, RAYS, what="rays only")
            st = eng.last_query_stats()
            assert (st.rays, st.hits) == (21 * 37, 0)
        eng.first_hits(want=("t",))
        before = eng.last_query_stats()
        assert M.load_library().rt_render_gbuffer(eng.handle, 0, 0, 0, 1, C.byref(A.rt_gbuffer()), 0, None) == A.RT_OK
        after = eng.last_query_stats()
        assert (after.rays, after.hits, after.launches) == (before.rays, before.hits, before.launches) and before.hits > 0


# ---------------------------------------------------------------- 5. live scenes
def test_live_scenes_follow_commits():
    sc = G.ambient_scene()
    eng = M.RayTracerEngine(copy.deepcopy(sc), deformable=True)
    first = eng.first_hits(want=ALL)
    _assert_oracle(first, sc)
    eng.set_transform(0, G.IS.trs((-1.2, 0.9, 1.0), (0, 1, 1), 50.0, (1.1, 0.8, 1.3)))      # set_transform + commit
    eng.set_transform(4, G.IS.trs((1.0, 2.3, -0.4), (1, 0, 0), 15.0, (0.8, 0.8, 0.8)))
    eng.commit()
    moved = eng.first_hits(want=ALL)
    _assert_oracle(moved, eng.scene)
    assert not _same(moved.hits.t, first.hits.t) and _same(moved.dirs, first.dirs)
    p = np.asarray(eng.scene.objects[2].positions, np.float64)                           # set_positions + commit
    eng.set_positions(2, p * (1.0 + 0.25 * np.sin(3.0 * p[:, :1])) + np.array([0.0, 0.2, 0.0]))
    eng.commit()
    bent = eng.first_hits(want=ALL)
    _assert_oracle(bent, eng.scene)
    assert not _same(bent.hits.t, moved.hits.t)
    eng.set_visible(1, False)                                                            # a hidden instance is absent
    eng.commit()
    hidden = eng.first_hits(want=ALL)
    vis = eng.visible_scene()
    assert len(vis.objects) == len(sc.objects) - 1
    _assert_oracle(hidden, vis)
    assert not (hidden.hits.ids[..., 0] == 1).any() and (bent.hits.ids[..., 0] == 1).any()
    eng.set_transform(3, G.IS.trs((0.0, -0.2, 0.0), (0, 1, 0), 10.0))
    eng.commit(rebuild=True)                                                             # commit(rebuild=True)
    rebuilt = eng.first_hits(want=ALL)
    _assert_oracle(rebuilt, eng.visible_scene())
    eng.close()


def test_two_replicas_answer_alike():
    sc = _scene("instances")
    with M.RayTracerEngine(_scene("instances"), devices=[0, 0]) as eng:
        a = eng.first_hits(want=ALL, slot=0)
        b = eng.first_hits(want=ALL, slot=1)
        assert eng.last_query_stats(1).rays == 21 * 37
    _assert_equal(b, a, what="slot 1")
    _assert_oracle(b, sc)


# ---------------------------------------------------------------- 6. contract
def test_refusals_leave_the_outputs_untouched():
    import torch
    eng = M.RayTracerEngine(G.ambient_scene(), dynamic=True)
    lib = M.load_library()
    host = {f: np.full((21, 37, COLS[f][0]), 7, COLS[f][1]) for f in ALL}
    dev = _tensors(21, 37, fill=7)

    def buf(arrays):
        gb = A.rt_gbuffer()
        for f, a in arrays.items():
            setattr(gb if f in RAYS else gb.hits, M.engine.FirstHits.ABI.get(f, f), M.engine._ptr(a))
        return gb

    gh, gd = buf(host), buf(dev)

    def call(slot=0, cam=0, first=0, step=1, out=gh, flags=0):
        return lib.rt_render_gbuffer(eng.handle, slot, cam, first, step, C.byref(out) if out is not None else None,
                                     flags, None)

    for flags, out in ((0, gh), (A.RT_GBUFFER_DEVICE, gd)):
        assert call(slot=1, out=out, flags=flags) == A.RT_ERR_INVALID_ARG
        assert call(slot=-1, out=out, flags=flags) == A.RT_ERR_INVALID_ARG
        assert call(cam=1, out=out, flags=flags) == A.RT_ERR_INVALID_CAMERA
        assert call(cam=-1, out=out, flags=flags) == A.RT_ERR_INVALID_CAMERA
        assert call(first=-1, out=out, flags=flags) == A.RT_ERR_INVALID_ARG
        assert call(step=0, out=out, flags=flags) == A.RT_ERR_INVALID_ARG
        assert call(out=out, flags=flags | 8) == A.RT_ERR_INVALID_ARG
        assert call(out=None, flags=flags) == A.RT_ERR_INVALID_ARG
    assert call(out=gh, flags=A.RT_GBUFFER_DEVICE) == A.RT_ERR_UNSUPPORTED      # host pointers are not device pointers
    mixed = buf(dict(dev, flags=host["flags"]))
    assert call(out=mixed, flags=A.RT_GBUFFER_DEVICE) == A.RT_ERR_UNSUPPORTED
    assert lib.rt_render_gbuffer(None, 0, 0, 0, 1, C.byref(gh), 0, None) == A.RT_ERR_NO_SCENE
    with pytest.raises(ValueError):
        eng.first_hits(want=("t", "colour"))
    # a lost scene (debug_fail_commit_step: a host-side early return that launches nothing)
    eng.set_transform(0, G.IS.trs((0.0, 1.0, 0.0)))
    eng.set_unsafe_option("debug_fail_commit_step", 1)
    with pytest.raises(M.RenderError) as e:
        eng.commit()
    assert e.value.code == A.RT_ERR_DEVICE
    for flags, out in ((0, gh), (A.RT_GBUFFER_DEVICE, gd)):
        assert call(out=out, flags=flags) == A.RT_ERR_DEVICE and b"lost" in lib.rt_last_error()
    with pytest.raises(M.RenderError) as e:
        eng.first_hits()
    assert e.value.code == A.RT_ERR_DEVICE
    torch.cuda.synchronize()
    for f in ALL:
        assert (host[f] == 7).all() and bool((dev[f] == 7).all()), f"{f} was written by a refused call"
    eng.close()


def test_statistics_and_byte_accounting():
    sc = _scene("instances")
    tab = M.engine.query_tables(sc)
    with M.RayTracerEngine(_scene("instances")) as eng:
        i0 = eng.info()
        h = eng.first_hits(want=("rays", "t", "uv", "point", "normal", "flags"))
        st = eng.last_query_stats()
        hits = int(np.isfinite(h.hits.t).sum())
        assert (st.rays, st.hits, st.non_finite, st.reduced, st.walk, st.launches) == (21 * 37, hits, 0, 0, 3, 1) and hits > 0
        cam = np.asarray(sc.cameras[0].position)
        assert st.bounds.origin_coord == np.abs(cam).max() and 1.0 <= st.bounds.dir_norm <= 1.0 + 2.0 ** -49
        i1 = eng.info()
        assert i1.device_bytes == i0.device_bytes, "no ids asked for: the same device_bytes"
        eng.first_hits(want=("ids",))
        i2 = eng.info()
        assert i2.device_bytes - i1.device_bytes == 4 * len(tab["face"]) + 4 * len(tab["inst_object"])
        eng.first_hits(want=ALL)
        eng.query_closest(h.origins.reshape(-1, 3), h.dirs.reshape(-1, 3), want=("ids",))
        assert eng.info().device_bytes == i2.device_bytes, "the face table is uploaded once"
        eng.set_option("fit", 0)
        eng.first_hits(0, 1, 2)
        st = eng.last_query_stats()
        assert (st.rays, st.walk) == (8 * 37, 2)


def test_a_degenerate_camera_is_flagged_and_not_traced():
    sc = G.ambient_scene()
    cam = sc.cameras[0]
    gaze = np.asarray(cam.gaze_point) - np.asarray(cam.position)
    sc.cameras[0] = dataclasses.replace(cam, up=tuple(float(x) for x in 2.0 * gaze))      # up parallel to the gaze
    with M.RayTracerEngine(sc) as eng:
        h = eng.first_hits(want=ALL)
        st = eng.last_query_stats()
    assert not np.isfinite(h.dirs).all(-1).any()
    assert (h.hits.flags == A.RT_HIT_NON_FINITE).all() and np.isinf(h.hits.t).all() and (h.hits.ids == -1).all()
    assert not h.hits.point.any() and not h.hits.normal.any() and not h.hits.uv.any()
    assert (st.rays, st.hits, st.non_finite) == (21 * 37, 0, 21 * 37)
