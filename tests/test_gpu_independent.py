"""GPU frames against the independent tracer's frozen frames, not against the oracle
(DESIGN.md §2 "Pinning"): tests/golden/independent/*.npz come from tests/independent_tracer.py, a
second brute-force reading of the reference without a BVH, so a misreading that the oracle and the
kernels share fails here.  The Python tracer itself never runs in this file.

The bar is the one every GPU frame test holds: per-channel L-inf <= 1e-5 on the FP64 frame, exact
RGBA8, equal primary / shadow / secondary ray counts.  Every scene runs on the default path and on
every render path whose options apply to it."""
import numpy as np
import pytest

import myraytracer_amd as M
import independent_scenes as IS

pytestmark = pytest.mark.gpu
TOL = 1e-5

MIRROR = [("mirrors", 0), ("mirrors", 1), ("mirrors", 2), ("blur_quirk", 0)]
PATHS = [(n, c, {}, (0, 1)) for n, c in IS.cases()]
# compacted bounce render and the bounce megakernel (mirror / conductor scenes)
PATHS += [(n, c, o, (0, 1)) for n, c in MIRROR
          for o in ({"queue": 0}, {"queue": 1, "queue_tail": 0}, {"queue": 1, "queue_tail": 2})]
# structure of the full trace() passes (glass and area lights)
PATHS += [("glass", 0, o, (0, 1)) for o in ({"levels": 0}, {"nodeshade": 0}, {"node_lists": 0}, {"node_lists": 1},
                                             {"hitlog": 1}, {"levels": 0, "node_lists": 0})]
# the walks
PATHS += [(n, c, o, (0, 1)) for n, c in (("phong", 0), ("mirrors", 0), ("glass", 0))
          for o in ({"wide": 0}, {"unified": 0}, {"fit": 0}, {"unified_transformed": 0})]
# chunk selection
PATHS += [(n, c, {}, (1, 2)) for n, c in (("phong", 0), ("mirrors", 1), ("glass", 0), ("blur_quirk", 0))]


def _check(name, cam, rgb, rgba, st, first, step, what):
    ref, ref8, rays = IS.frozen_selection(name, cam, first, step)
    assert rgb.shape == ref.shape
    diff = np.abs(rgb - ref)
    linf = float(diff.max()) if diff.size else 0.0
    print(f"{name} camera {cam} {what} chunks ({first}, {step}): max |gpu - independent| = {linf:.3e}")
    assert linf <= TOL, f"L-inf {linf:.3e} on {int((diff > TOL).any(axis=-1).sum())} pixels"
    assert np.array_equal(rgba, ref8), f"RGBA8 mismatch on {int((rgba != ref8).any(axis=-1).sum())} pixels"
    assert (st.primary_rays, st.shadow_rays, st.secondary_rays) == rays


def _id(v):
    return ",".join(f"{k}={x}" for k, x in v.items()) or "default" if isinstance(v, dict) else None


@pytest.mark.parametrize("name, cam, options, chunks", PATHS, ids=_id)
def test_frame_against_the_independent_tracer(name, cam, options, chunks):
    eng = M.RayTracerEngine(IS.scene(name))
    for k, v in options.items():
        eng.set_option(k, v)
    rgb, rgba, st = eng.render_rows(cam, chunks[0], chunks[1], True)
    eng.close()
    _check(name, cam, rgb, rgba, st, chunks[0], chunks[1], options or "default")


def test_submitted_render_against_the_independent_tracer():
    """rt_render_submit / rt_render_wait into page-locked arrays: two cameras in flight."""
    eng = M.RayTracerEngine(IS.scene("mirrors"))
    outs = [eng.alloc_frame(cam, 0, 1) for cam in (0, 2)]
    tickets = [eng.submit_into(cam, 0, 1, rgb=o[0], rgba=o[1]) for cam, o in zip((0, 2), outs)]
    stats = [eng.wait(t) for t in reversed(tickets)][::-1]
    for cam, o, st in zip((0, 2), outs, stats):
        _check("mirrors", cam, o[0], o[1], st, 0, 1, "submitted")
    eng.close()
