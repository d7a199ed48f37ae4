"""The oracle against an independent restatement of the reference (CPU; DESIGN.md §2 "Pinning").

oracle/rt_oracle.cpp and the kernels were written from one reading of the Swift reference.
tests/independent_tracer.py is a second reading, brute force and without a BVH, and
tests/golden/independent/*.npz are its frozen frames (make_independent_golden.py).  Here the
tracer is re-run against those files and the oracle is compared with it: frames within the CPU
bound on every pixel, RGBA8 and ray counts exactly, explicit rays hit by hit.

The CPU bound is 1e-9 absolute on radiance (the scenes stay below 1e3), the project's figure from
test_oracle_kat.py::test_c1_centre_pixel_closed_form: a cap, not a measurement.  The measured
maxima are printed and recorded in DESIGN.md §2.
"""
import numpy as np
import pytest

import independent_scenes as IS
import independent_tracer as IT
import oracle

CPU_BOUND = 1e-9
RERUN_BOUND = 1e-12
CASES = IS.cases()
frozen, frozen_selection = IS.frozen, IS.frozen_selection
_cache = {}


def tracer(name):
    if ("tracer", name) not in _cache:
        _cache["tracer", name] = IT.IndependentTracer(IS.scene(name), np.float64)
    return _cache["tracer", name]


def oracle_scene(name):
    if ("oracle", name) not in _cache:
        _cache["oracle", name] = oracle.OracleScene(IS.scene(name))
    return _cache["oracle", name]


@pytest.mark.parametrize("name, cam", CASES)
def test_rerun_matches_the_frozen_frame(name, cam):
    """Not bit-exact (pow, exp and tan differ between libm builds), but to 1e-12, with equal tallies."""
    t = tracer(name)
    H = frozen(name)[f"rgb_{cam}"].shape[0]
    parts = [t.render_chunk(cam, k) for k in range((H + 7) // 8)]
    rgb, rgba, _, _ = IT.gather(parts, frozen(name)[f"rgb_{cam}"].shape[1])
    z = frozen(name)
    assert list(z["ray_names"]) == list(IT.RAYS) and list(z["branch_names"]) == list(IT.BRANCHES)
    diff = float(np.abs(rgb - z[f"rgb_{cam}"]).max())
    print(f"{name} camera {cam}: max |re-run - frozen| = {diff:.3e}")
    assert rgb.shape == z[f"rgb_{cam}"].shape and diff <= RERUN_BOUND
    assert np.array_equal(rgba, z[f"rgba_{cam}"])
    assert [[p[1][n] for n in IT.RAYS] for p in parts] == z[f"rays_{cam}"].tolist()
    assert [[p[2][n] for n in IT.BRANCHES] for p in parts] == z[f"branches_{cam}"].tolist()
    assert float(z[f"ld_{cam}"]) <= CPU_BOUND              # the maker's longdouble guard, as recorded


@pytest.mark.parametrize("first, step", [(0, 1), (1, 2)])
@pytest.mark.parametrize("name, cam", CASES)
def test_oracle_frame_against_the_independent_tracer(name, cam, first, step):
    """Every pixel compared, none exempted: L-inf within the CPU bound, RGBA8 and ray counts equal."""
    ref, ref8, rays = frozen_selection(name, cam, first, step)
    rgb, rgba, st = oracle_scene(name).render(cam, first, step, threads=0, rgba=True)
    assert rgb.shape == ref.shape
    diff = float(np.abs(rgb - ref).max()) if rgb.size else 0.0
    print(f"{name} camera {cam} chunks ({first}, {step}): max |oracle - independent| = {diff:.3e}")
    assert diff <= CPU_BOUND, f"{int((np.abs(rgb - ref) > CPU_BOUND).any(axis=-1).sum())} pixels beyond the bound"
    assert np.array_equal(rgba, ref8)
    assert (st.primary_rays, st.shadow_rays, st.secondary_rays) == rays


def _rays(seed, n=300):
    """Origins around the scenes, directions towards them (half of them not unit length), a tMin
    for half of the rays, times in [0, 1), segment lengths for the occlusion test."""
    r = np.random.RandomState(seed)
    o = r.uniform((-5.0, -0.5, -5.0), (5.0, 5.0, 7.0), (n, 3))
    d = r.uniform((-2.5, -1.0, -3.0), (2.5, 2.5, 3.0), (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[n // 2:] *= r.uniform(0.3, 3.0, (n - n // 2, 1))
    tmin = np.where(r.uniform(size=n) < 0.5, 0.0, r.uniform(0.0, 3.0, n))
    return o, d, tmin, r.uniform(0.0, 1.0, n), r.uniform(0.5, 12.0, n)


@pytest.mark.parametrize("k, name", list(enumerate(IS.NAMES)))
def test_explicit_rays(k, name):
    """Brute-force closest and occluded against the oracle's intersectTLAS / occludedTLAS: which
    separates an intersection disagreement from a shading one."""
    o, d, tmin, time, tmax = _rays(4000 + k)
    t, p, n, mat = oracle_scene(name).trace_rays(o, d, tmin, time)
    occ = oracle_scene(name).occluded_rays(o, d, tmax, time)
    tr = tracer(name)
    hits, worst = 0, 0.0
    for i in range(len(o)):
        h = tr.closest(o[i], d[i], tmin[i], time[i])
        assert (h is not None) == bool(np.isfinite(t[i])), f"ray {i}: hit/miss differs"
        assert tr.occluded(o[i], d[i], tmax[i], time[i]) == bool(occ[i]), f"ray {i}: occlusion differs"
        if h is None:
            continue
        hits += 1
        assert h.mat == int(mat[i]), f"ray {i}: material {h.mat} against {int(mat[i])}"
        err = max(abs(h.t - t[i]) / max(1.0, abs(t[i])),
                  float(np.abs(h.p - p[i]).max()) / max(1.0, float(np.abs(p[i]).max())),
                  float(np.abs(h.n - n[i]).max()))
        worst = max(worst, err)
        assert err <= CPU_BOUND, f"ray {i}: t / point / normal off by {err:.3e}"
    print(f"{name}: {hits} hits of {len(o)} rays, {int(occ.sum())} occluded, worst relative error {worst:.3e}")
    if name not in ("empty", "all_miss"):
        assert hits > len(o) // 4 and 0 < int(occ.sum()) < len(o)


def test_every_branch_is_reached():
    """The scenes together fire every branch the tally names, so the frames depend on each."""
    total = dict.fromkeys(IT.BRANCHES, 0)
    for name, cam in CASES:
        for b, v in zip(IT.BRANCHES, frozen(name)[f"branches_{cam}"].sum(axis=0)):
            total[b] += int(v)
    print(total)
    assert all(v > 0 for v in total.values()), total


def test_longdouble_tracer_runs():
    """The tracer is generic over its scalar type: one chunk in np.longdouble against float64."""
    sc = IS.scene("glass")
    a = IT.IndependentTracer(sc, np.longdouble).render_chunk(0, 1)
    b = tracer("glass").render_chunk(0, 1)
    assert a[0].dtype == np.longdouble and a[1] == b[1] and a[2] == b[2]
    assert float(np.abs(a[0] - b[0]).max()) <= CPU_BOUND
