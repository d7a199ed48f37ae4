"""tests/gbuffer_rays.py is a sound yardstick for tests/test_gpu_gbuffer.py: shown with the oracle and
numpy alone (no GPU, none of the code under test).

The ambient scene has no lights, so the oracle's FP64 frame at one sample per pixel is, at every
pixel, ambient_light * (the ambient of the material its primary ray hit), or the background.  The
helper's rays, traced by the oracle's intersectTLAS, must name that material at every one of the
37 x 21 pixels, bit for bit, none left out: were a seed, a draw, a sub-cell or the image-plane tMin
of the restatement off, silhouette pixels would name another object.  Both branches and the
silhouettes are shown to be in play: a tenth of the pixels miss, and ten adjacent pairs differ in
material.  These are conditions on the inputs, not measurements of the code."""
import os
import sys

import numpy as np

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_rays as G                                                         # noqa: E402


def test_the_oracle_renders_the_helper_rays():
    sc = G.ambient_scene()
    W, H = sc.cameras[0].image_resolution
    assert (W, H) == (37, 21) and sc.cameras[0].num_samples == 1 and not sc.point_lights and not sc.area_lights
    prod = np.asarray(sc.ambient_light) * np.asarray([m.ambient for m in sc.materials])
    assert len({tuple(p) for p in prod}) == len(sc.materials) == len(sc.objects)
    assert not (prod == np.asarray(sc.background_color)).all(1).any() and (np.asarray(sc.ambient_light) != 0).all()
    rays = G.first_rays(sc)
    osc = oracle.OracleScene(sc)
    frame, _ = osc.render(0)
    t, _, _, mat = osc.trace_rays(rays["origins"].reshape(-1, 3), rays["dirs"].reshape(-1, 3), rays["tmin"].reshape(-1),
                                  rays["time"].reshape(-1))
    osc.close()
    hit = np.isfinite(t).reshape(H, W)
    mat = mat.reshape(H, W)
    want = G.ambient_colours(sc, mat, hit)
    bad = (want.view(np.uint64) != np.ascontiguousarray(frame).view(np.uint64)).any(-1)
    assert frame.shape == (H, W, 3) and int(bad.sum()) <= 0, f"{int(bad.sum())} pixels of {W * H} differ"
    miss = float((~hit).mean())
    seen = np.where(hit, mat, 0)
    pairs = int((seen[:, 1:] != seen[:, :-1]).sum() + (seen[1:] != seen[:-1]).sum())
    print(f"misses {miss:.3f}, adjacent pairs with different materials {pairs}, materials seen {sorted(set(seen.ravel()))}")
    assert miss >= 0.1 and pairs >= 10
    assert set(seen[hit]) == set(range(1, len(sc.materials) + 1)), "every object is seen"


def test_the_pixel_centre_rays_are_the_undrawn_ones():
    """centre=True: the rays of the same camera through pixel centres - the origin is the eye, time is 0,
    and the direction is the jittered one's to within a pixel; chunk selections pack their rows."""
    sc = G.ambient_scene()
    a, c = G.first_rays(sc), G.first_rays(sc, centre=True)
    assert not c["time"].any() and (a["time"] > 0).all() and (a["time"] < 1).all()
    assert np.array_equal(c["origins"], a["origins"]) and (c["origins"] == np.asarray(sc.cameras[0].position)).all()
    step = np.linalg.norm(c["dirs"][:, 1:] - c["dirs"][:, :-1], axis=-1).max()
    assert 0 < np.linalg.norm(c["dirs"] - a["dirs"], axis=-1).max() <= step
    sel = G.first_rays(sc, 0, 1, 2)
    assert sel["dirs"].shape == (8, 37, 3) and np.array_equal(sel["dirs"], a["dirs"][8:16])
    assert np.array_equal(G.first_rays(sc, 0, 2, 3)["tmin"], a["tmin"][16:21])
