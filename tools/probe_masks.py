"""What does a ray mask cost, and what does it buy?  

C3i (terrain + 24 instances of one icosphere: 25 instances, the flattened instance tree), the camera's
primary rays at 1920x1080 in pixel order as exported by rt_render_gbuffer, traced by rt_query_closest
(want t, ids) and rt_query_occluded (tMax = +inf) from device tensors with declared bounds, so a call
only enqueues.  Timed as tools/probe_query.py times: median (min .. max) in ms of `--reps` timed calls
after two warm-up calls, on the host clock around the call and a device synchronise, in one process.
  unmasked            the unmasked entry points (the kernels of the parent commit)
  masked_no_table     a batch mask of all-ones before any instance mask was set: the masked kernels,
                      no table to load
  masked_all_ones     ... with the table present and every instance all-ones: the price of the test
  masked_13           a batch mask that keeps the terrain and 12 spheres (every other sphere masked out)
  hidden_13           unmasked, the same 12 spheres hidden by a commit (refit only), and after a
  hidden_13_rebuilt   compacting rebuild
  static_13           unmasked, a static scene created with only the 13 objects
  per_ray_two_layers  per-ray masks alternating two layers ray by ray: even rays see the terrain and 12
                      spheres, odd rays the terrain and the other 12
Before a variant is timed the probe checks that masked_all_ones equals unmasked bit for bit in t, and
prints on how many rays masked_13 differs in t from hidden_13 and from static_13 (other TLASes: an
equal-t tie between two instances may fall the other way there; the tests' inputs are free of those).
Prints text and one JSON line per figure, with the library's sha-256.
usage: probe_masks.py [--reps 7] [--width 1920 --height 1080]
The probe needs a GPU; nothing falls back."""
import argparse
import copy
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import torch
    import myraytracer_amd as M
    from myraytracer_amd import scenes
    assert torch.cuda.is_available(), "probe_masks.py needs a GPU"
    sha = hashlib.sha256(open(M.engine.LIB_PATH, "rb").read()).hexdigest()[:16]
    sc = scenes.scene_c3_instanced(width=args.width, height=args.height, inline=True)
    HIDE = list(range(2, 25, 2))                          # 12 of the sphere objects 1 .. 24
    dyn = M.RayTracerEngine(copy.deepcopy(sc), dynamic=True)
    fh = dyn.first_hits(want=("origins", "dirs"))
    O, D = np.ascontiguousarray(fh.origins.reshape(-1, 3)), np.ascontiguousarray(fh.dirs.reshape(-1, 3))
    n = len(O)
    b = dyn.last_query_stats().bounds                     # the camera's bounds, as rt_render_gbuffer reports them
    # (the reach is measured from the scene's centre, which moves a little when spheres are hidden)
    bounds = (b.origin_reach + 20.0, b.origin_coord + 1.0, b.dir_norm)
    Od, Dd = torch.as_tensor(O, device="cuda:0"), torch.as_tensor(D, device="cuda:0")
    print(f"probe_masks: C3i, {n} primary rays, {args.reps} reps, libmyrt sha256 {sha}", flush=True)

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

    def report(name, eng, mask, note=""):
        kw = {} if mask is None else {"mask": mask}
        for kind, fn in (("closest", lambda: eng.query_closest(Od, Dd, want=("t", "ids"), bounds=bounds, **kw)),
                         ("occluded", lambda: eng.query_occluded(Od, Dd, bounds=bounds, **kw))):
            ms = timed(fn)
            med = statistics.median(ms)
            rec = {"probe": "masks", "scene": "c3i", "variant": name, "kind": kind, "rays": n, "median_ms": round(med, 3),
                   "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "mrays_s": round(n / med / 1e3, 1),
                   "walk": eng.last_query_stats().walk, "lib_sha256": sha}
            print(f"{name:20s} {kind:9s} {med:9.3f} ms ({min(ms):.3f} .. {max(ms):.3f})  {rec['mrays_s']:9.1f} Mrays/s {note}",
                  flush=True)
            print("JSON " + json.dumps(rec), flush=True)

    def closest_t(eng, mask=None):
        h = eng.query_closest(Od, Dd, want=("t",), bounds=bounds, **({} if mask is None else {"mask": mask}))
        torch.cuda.synchronize()
        st = eng.last_query_stats()
        assert st.out_of_bounds == 0 and st.non_finite == 0
        return h.t

    ALL1 = 0xFFFFFFFF
    t_all = closest_t(dyn)
    report("unmasked", dyn, None)
    assert torch.equal(closest_t(dyn, ALL1), t_all), "the masked kernels without a table differ from the unmasked ones"
    report("masked_no_table", dyn, ALL1)
    dyn.set_mask_many(range(25), ALL1)
    assert torch.equal(closest_t(dyn, ALL1), t_all), "masked with an all-ones table differs from unmasked"
    report("masked_all_ones", dyn, ALL1)
    # layer bit 0: the terrain and the 12 spheres that stay; bit 1: the terrain and the other 12
    dyn.set_mask_many(range(25), [3 if i == 0 else (2 if i in HIDE else 1) for i in range(25)])
    t_13 = closest_t(dyn, 1)
    report("masked_13", dyn, 1)
    layers = torch.as_tensor((1 + (np.arange(n) & 1)).astype(np.int32), device="cuda:0")
    t_layers = closest_t(dyn, layers)
    assert torch.equal(t_layers[0::2], t_13[0::2]) and torch.equal(t_layers[1::2], closest_t(dyn, 2)[1::2])
    report("per_ray_two_layers", dyn, layers)
    dyn.set_visible_many(HIDE, False)
    dyn.commit()
    print(f"masked_13 against hidden_13: t differs on {int((closest_t(dyn) != t_13).sum())} of {n} rays", flush=True)
    report("hidden_13", dyn, None)
    dyn.commit(rebuild=True)
    assert dyn.last_rebuild_stats().rebuilt == 1
    report("hidden_13_rebuilt", dyn, None)
    dyn.close()
    only = M.engine.visible_subset(sc, [i not in HIDE for i in range(len(sc.objects))])
    static = M.RayTracerEngine(copy.deepcopy(only))
    print(f"masked_13 against static_13: t differs on {int((closest_t(static) != t_13).sum())} of {n} rays", flush=True)
    report("static_13", static, None)
    static.close()


if __name__ == "__main__":
    main()
