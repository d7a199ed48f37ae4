"""What does hiding instances cost, and what does it buy?  C3i (terrain + 24 instances of one icosphere)
created dynamic; 12 of the 24 sphere instances (every other one) are hidden.

Reports (one JSON line, and the same as text):
  commit         median / min / max (host clock around the blocking call) of: a plain commit that moves
                 the 12 instances by 1 % of their diameter (what the parent could do), the hiding commit,
                 the showing commit (plain: the tree holds every pair), the compacting rebuild of the
                 hidden state (both builders) and the show after a compacting rebuild (forced rebuild)
  mrays          Mrays/s (primary + shadow rays traversed) of the public submit/wait path, 16 renders in
                 flight, whole 1920x1080 frames, median / min / max of three windows: all visible; hidden
                 with refit only; hidden with a rebuild (Morton, clustered); a static scene created with
                 only the 13 visible objects (the target); the same 12 instances parked 1e6 away by
                 set_transform (the workaround visibility replaces)
  fit_cost       rt_scene_fit_cost of each (the static scene's from a dynamic engine of the same objects)
With a library that lacks the visibility entry points (MYRT_LIB = a parent build) only the moving commit,
the all-visible and the parked figures are taken.
usage: probe_visibility.py [--frames 100] [--commits 20]
The scene needs a GPU; nothing falls back."""
import argparse
import copy
import hashlib
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")     # one queue per render in flight, as bench.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import myraytracer_amd as M  # noqa: E402
from myraytracer_amd import _abi as A  # noqa: E402
from myraytracer_amd import scenes  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--frames", type=int, default=100)
p.add_argument("--commits", type=int, default=20)
p.add_argument("--scenes", default=os.path.join(ROOT, "scenes_cache"))
args = p.parse_args()


def throughput(eng, frames):
    """Mrays/s of `frames` whole frames through submit/wait with RT_MAX_IN_FLIGHT in flight."""
    W, H = eng.scene.cameras[0].image_resolution
    Q = A.RT_MAX_IN_FLIGHT
    bufs = [M.pinned_array((H, W, 4), np.uint8) for _ in range(Q)]
    submit, wait = eng.frame_pipeline(0, 0, 1, bufs)

    def run(n):
        rays = 0
        tickets = []
        t0 = time.perf_counter()
        for k in range(n):
            if len(tickets) == Q:
                st = wait(tickets.pop(0))
                rays += st.primary_rays + st.shadow_rays_traced
            tickets.append(submit(k))
        for t in tickets:
            st = wait(t)
            rays += st.primary_rays + st.shadow_rays_traced
        return rays, time.perf_counter() - t0
    run(2 * Q)                                          # warm-up: every slot's stream, arenas, code objects
    res = []
    for _ in range(3):
        rays, dt = run(frames)
        res.append(rays / dt / 1e6)
    return {"median": statistics.median(res), "min": min(res), "max": max(res)}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


lib_path = os.environ.get("MYRT_LIB") or M.engine.LIB_PATH
HAS = hasattr(M.load_library(), "rt_scene_set_instance_visible")
sc = scenes.scene_c3_instanced(path_dir=args.scenes)
HIDE = list(range(2, 25, 2))                          # 12 of the sphere objects 1 .. 24
out = {"scene": "C3i", "lib_sha256_16": hashlib.sha256(open(lib_path, "rb").read()).hexdigest()[:16],
       "frames": args.frames, "commits": args.commits, "visibility": HAS, "hidden_objects": HIDE}
commit, mrays, cost = {}, {}, {}
dyn = M.RayTracerEngine(copy.deepcopy(sc), dynamic=True)
mrays["all_visible"] = throughput(dyn, args.frames)
cost["all_visible"] = dyn.fit_cost()
home = {i: np.array(sc.objects[i].transform, dtype=np.float64) for i in HIDE}
jit = np.random.RandomState(10)


def move(eng, offset=None):
    for i, m0 in home.items():
        m = m0.copy()
        if offset is None:
            m[12:15] += jit.normal(scale=0.01 * 2.0 * m0[0], size=3)
        else:
            m[12:15] += offset
        eng.set_transform(i, m)


def moving_commit():
    move(dyn)
    return timed(dyn.commit)


commit["move_12"] = spread([moving_commit() for _ in range(args.commits)])
for i, m0 in home.items():
    dyn.set_transform(i, m0)
dyn.commit()

if HAS:
    hide, show = [], []
    for _ in range(args.commits):
        dyn.set_visible_many(HIDE, False)
        hide.append(timed(dyn.commit))
        dyn.set_visible_many(HIDE, True)
        show.append(timed(dyn.commit))
    commit["hide_12"], commit["show_12"] = spread(hide), spread(show)
    dyn.set_visible_many(HIDE, False)
    dyn.commit()
    vs = dyn.last_visibility_stats()
    out["pairs"] = {"all": vs.pairs, "visible": vs.pairs_visible}
    mrays["hidden_refit"] = throughput(dyn, args.frames)
    cost["hidden_refit"] = dyn.fit_cost()
    for name, flag in (("morton", True), ("clustered", "clustered")):
        commit["compacting_rebuild_" + name] = spread([timed(lambda: dyn.commit(rebuild=flag)) for _ in range(args.commits)])
        rs, v2 = dyn.last_rebuild_stats(), dyn.last_visibility_stats()
        assert rs.rebuilt == 1 and v2.pairs_in_tree == v2.pairs_visible
        out["rebuilt_tree_" + name] = {"nodes": rs.nodes_after, "depth": rs.depth_after, "sort_ms": rs.sort_ms,
                                       "build_ms": rs.build_ms}
        mrays["hidden_rebuilt_" + name] = throughput(dyn, args.frames)
        cost["hidden_rebuilt_" + name] = dyn.fit_cost()
    forced = []
    for _ in range(max(3, args.commits // 4)):
        dyn.set_visible_many(HIDE, True)
        forced.append(timed(dyn.commit))
        assert dyn.last_visibility_stats().forced_rebuild == 1
        dyn.set_visible_many(HIDE, False)
        dyn.commit(rebuild=True)
    commit["show_12_forced_rebuild"] = spread(forced)
    dyn.set_visible_many(HIDE, True)
    dyn.commit(rebuild=True)

keep = [i not in HIDE for i in range(len(sc.objects))]
only = M.engine.visible_subset(sc, keep) if hasattr(M.engine, "visible_subset") else None
if only is None:
    only = copy.copy(sc)
    only.objects = [o for o, k in zip(sc.objects, keep) if k]      # the base mesh (object 1) stays: no conversion
static = M.RayTracerEngine(copy.deepcopy(only))
mrays["static_13_objects"] = throughput(static, args.frames)
static.close()
twin = M.RayTracerEngine(copy.deepcopy(only), dynamic=True)
cost["static_13_objects"] = twin.fit_cost()
twin.close()

dyn.close()
dyn = M.RayTracerEngine(copy.deepcopy(sc), dynamic=True)    # the build's tree again, not a rebuilt one
move(dyn, offset=np.array([1.0e6, 0.0, 0.0]))
commit["park_12_at_1e6"] = spread([timed(dyn.commit)])
mrays["parked_1e6"] = throughput(dyn, args.frames)
cost["parked_1e6"] = dyn.fit_cost()
dyn.close()

out["commit_ms"], out["mrays"], out["fit_cost"] = commit, mrays, cost
t = mrays["static_13_objects"]["median"]
out["over_static"] = {k: v["median"] / t for k, v in mrays.items()}
for k, v in out.items():
    print(f"{k}: {v}")
print(json.dumps(out))
