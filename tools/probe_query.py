"""What does a ray query cost, and what is the order of the rays worth?  

C3 (1.02M triangles, the four-wide identity walk), three sets of 2^22 rays:
  primary   the camera's primary rays in pixel order: the rays the render casts, exported by
            rt_render_gbuffer (the frame's camera, at the resolution that gives 2^22 pixels; the
            figures of DESIGN.md §11 were measured on pinhole rays through pixel centres)
  shuffled  the same rays in random order
  random    uniformly random origins in the scene box, random directions
each through rt_query_closest (want t, uv, ids) and rt_query_occluded (tMax = +inf), as:
  debug           engine.trace_rays / occluded_rays (rt_debug_*): what a caller had before (the
                  hooks call the host-array query now: this row is `host` plus their repacking)
  host            numpy arrays in, numpy arrays out (staged through the slot's query scratch)
  device          torch tensors on the GPU, bounds reduced on the device (one synchronisation)
  device+bounds   ... bounds declared (the call only enqueues)
(The coherence reorder this probe was written to judge lost on every set and was removed; its
figures are in DESIGN.md §11.  primary against shuffled still shows what ray order is worth.)
Every figure is the median (min .. max) in ms of `--reps` timed calls after two warm-up calls, on
the host clock around the call and a device synchronise, all in one process; Mrays/s from the
median.  Prints text and one JSON line per figure, with the library's sha-256 prefix.
usage: probe_query.py [--log2 22] [--reps 7] [--scene c3]
The probe needs a GPU; nothing falls back."""
import argparse
import dataclasses
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def primary_resolution(cam, n):
    """The resolution of `cam`'s aspect that has at least n pixels."""
    W0, H0 = cam.image_resolution
    k = np.sqrt(n / (W0 * H0))
    W, H = int(np.ceil(W0 * k)), int(np.ceil(H0 * k))
    while W * H < n:
        H += 1
    return W, H


def primary_rays(eng, n):
    """The first n primary rays the render casts, in pixel order: exported by rt_render_gbuffer
    (engine.first_hits), not restated here."""
    fh = eng.first_hits(want=("origins", "dirs"))
    return (np.ascontiguousarray(fh.origins.reshape(-1, 3)[:n]), np.ascontiguousarray(fh.dirs.reshape(-1, 3)[:n]))


def ray_sets(sc, eng, n, seed=5):
    P = np.asarray(sc.objects[0].positions, np.float64)
    lo, hi = P.min(0), P.max(0)
    rng = np.random.RandomState(seed)
    Oa, Da = primary_rays(eng, n)
    perm = rng.permutation(n)
    Oc = rng.uniform(lo, hi, size=(n, 3))
    Dc = rng.normal(size=(n, 3))
    Dc /= np.linalg.norm(Dc, axis=1, keepdims=True)
    return {"primary": (Oa, Da), "shuffled": (Oa[perm].copy(), Da[perm].copy()), "random": (Oc, Dc)}, (lo, hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scene", default="c3", choices=["c3", "c2"])
    args = ap.parse_args()
    import torch
    import myraytracer_amd as M
    from myraytracer_amd import scenes
    assert torch.cuda.is_available(), "probe_query.py needs a GPU"
    sha = hashlib.sha256(open(M.engine.LIB_PATH, "rb").read()).hexdigest()[:16]
    sc = {"c3": scenes.scene_c3, "c2": scenes.scene_c2}[args.scene](inline=True)
    n = 1 << args.log2
    sc.cameras[0] = dataclasses.replace(sc.cameras[0], image_resolution=primary_resolution(sc.cameras[0], n))
    eng = M.RayTracerEngine(sc)
    sets, (lo, hi) = ray_sets(sc, eng, n)
    centre = 0.5 * (lo + hi)
    print(f"probe_query: {args.scene}, {n} rays per set, {args.reps} reps, libmyrt sha256 {sha}", flush=True)

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    for name, (O, D) in sets.items():
        bounds = (float(np.linalg.norm(O - centre, axis=1).max() * 1.01 + 1.0), float(np.abs(O).max() * 1.01),
                  float(np.linalg.norm(D, axis=1).max() * 1.001))
        Od, Dd = torch.as_tensor(O, device="cuda:0"), torch.as_tensor(D, device="cuda:0")
        inf = np.full(n, np.inf)
        variants = {
            "closest": [("debug", lambda: eng.trace_rays(O, D)),
                        ("host", lambda: eng.query_closest(O, D)),
                        ("device", lambda: eng.query_closest(Od, Dd)),
                        ("device+bounds", lambda: eng.query_closest(Od, Dd, bounds=bounds))],
            "occluded": [("debug", lambda: eng.occluded_rays(O, D, inf)),
                         ("host", lambda: eng.query_occluded(O, D)),
                         ("device", lambda: eng.query_occluded(Od, Dd)),
                         ("device+bounds", lambda: eng.query_occluded(Od, Dd, bounds=bounds))]}
        # declared bounds must not change a result: one comparison per set before anything is timed
        a, b = eng.query_closest(Od, Dd), eng.query_closest(Od, Dd, bounds=bounds)
        torch.cuda.synchronize()
        assert torch.equal(a.t, b.t) and torch.equal(a.ids, b.ids) and torch.equal(a.uv, b.uv), "bounds changed a result"
        st = eng.last_query_stats()
        assert st.out_of_bounds == 0 and st.non_finite == 0
        hits = float(torch.isfinite(a.t).double().mean())
        for kind, vs in variants.items():
            for vname, fn in vs:
                ms = timed(fn)
                med = statistics.median(ms)
                rec = {"probe": "query", "scene": args.scene, "set": name, "kind": kind, "variant": vname, "rays": n,
                       "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                       "mrays_s": round(n / med / 1e3, 1), "hit_fraction": round(hits, 4), "lib_sha256": sha}
                print(f"{name:9s} {kind:9s} {vname:19s} {med:9.3f} ms ({min(ms):.3f} .. {max(ms):.3f})  "
                      f"{rec['mrays_s']:9.1f} Mrays/s", flush=True)
                print("JSON " + json.dumps(rec), flush=True)
        del Od, Dd
    eng.close()


if __name__ == "__main__":
    main()
