#!/usr/bin/env python3
"""Freeze the independent tracer's frames (test infrastructure; run by hand like make_frame_golden.py).

Every scene of tests/independent_scenes.py and every camera is rendered by
tests/independent_tracer.py in np.float64 and in np.longdouble.  Nothing is written unless the two
agree within 1e-9 on every channel of every pixel and count the same rays and branches: a scene
that fails sits on a branch edge somewhere and is ill-conditioned, so change its seed, camera or
geometry, never the bound.  Then independent/<scene>.npz holds, per camera k:
  rgb_k       float64 frame (H, W, 3)
  rgba_k      RGBA8 (RayTracer.swift:186-194)
  rays_k      per 8-row chunk: primary, shadow, secondary rays     (names in `ray_names`)
  branches_k  per 8-row chunk: how often each branch fired         (names in `branch_names`)
  ld_k        max |float64 - longdouble| of the frame
The GPU tests read only these files.   python tests/golden/make_independent_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import independent_scenes as IS  # noqa: E402
import independent_tracer as IT  # noqa: E402

OUT = os.path.join(HERE, "independent")
BOUND = 1e-9


def chunks_of(tracer, cam):
    H = max(1, int(tracer.scene.cameras[cam].image_resolution[1]))
    return [tracer.render_chunk(cam, k) for k in range((H + IT.CHUNK - 1) // IT.CHUNK)]


def main():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        sys.exit("np.longdouble is no wider than float64 on this machine: the guard would prove nothing")
    os.makedirs(OUT, exist_ok=True)
    for name in IS.NAMES:
        sc = IS.scene(name)
        t64, tld = IT.IndependentTracer(sc, np.float64), IT.IndependentTracer(sc, np.longdouble)
        rec = {"ray_names": np.array(IT.RAYS), "branch_names": np.array(IT.BRANCHES)}
        for k in range(len(sc.cameras)):
            a, b = chunks_of(t64, k), chunks_of(tld, k)
            rgb = np.concatenate([p[0] for p in a])
            ld = float(np.abs(rgb.astype(np.longdouble) - np.concatenate([p[0] for p in b])).max())
            same = all(p[1] == q[1] and p[2] == q[2] for p, q in zip(a, b))
            print(f"{name} camera {k}: {rgb.shape}, max radiance {rgb.max():.4g}, |f64 - longdouble| {ld:.3e}, "
                  f"tallies {'equal' if same else 'DIFFER'}")
            if not (ld <= BOUND and same):
                sys.exit(f"{name} camera {k}: float64 and longdouble disagree; fix the scene, not the bound")
            rec[f"rgb_{k}"] = rgb
            rec[f"rgba_{k}"] = IT.to_rgba8(rgb)
            rec[f"rays_{k}"] = np.array([[p[1][n] for n in IT.RAYS] for p in a], np.int64)
            rec[f"branches_{k}"] = np.array([[p[2][n] for n in IT.BRANCHES] for p in a], np.int64)
            rec[f"ld_{k}"] = np.float64(ld)
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **rec)


if __name__ == "__main__":
    main()
