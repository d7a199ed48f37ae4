"""What does rebuilding the flattened instance tree buy, and what does it cost?  C3i (terrain + 24
instances of one icosphere) created dynamic; its 24 spheres are moved by 1, 4 and 16 of their own
diameters (tools/probe_refit.py's directions), and at each displacement three scenes are rendered:
the refit one (plain commits: the topology of the pose the scene was created at), the rebuilt one
(rt_scene_commit_ex with RT_COMMIT_REBUILD_FIT at that pose) and a fresh static scene created there.

Reports (one JSON line, and the same as text):
  mrays            Mrays/s (primary + shadow rays traversed) of the public submit/wait path, 16 renders
                   in flight, whole 1920x1080 frames, median / min / max of three windows, per
                   displacement: refit, rebuilt, fresh; and the ratios to fresh
  plain_commit     median / min / max of the plain commits that walk to the displacements
  rebuild_commit   median / min / max of 20 rebuilding commits at the last displacement (each moves
                   every sphere by 1 % of its diameter first), host clock around the blocking call,
                   with the rt_rebuild_stats split (rb_sort_ms, rb_build_ms, rb_total_ms) and the tree's size
  create           rt_scene_create of the fresh scenes (build_ms + upload_ms of rt_scene_info)
With --builder clustered the rebuilding commits take RT_COMMIT_REBUILD_FIT_CLUSTERED, and the rebuild rows
and the rebuild_commit spread also carry cluster_ms, iterations, cost_before and cost_after
(rt_rebuild_detail); --builder morton (the default) is the Morton builder and the output above.
usage: probe_rebuild.py [--frames 200] [--commits 20] [--diameters 1,4,16] [--builder morton|clustered]
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
p.add_argument("--frames", type=int, default=200)
p.add_argument("--commits", type=int, default=20)
p.add_argument("--diameters", default="1,4,16")
p.add_argument("--scenes", default=os.path.join(ROOT, "scenes_cache"))
p.add_argument("--builder", choices=("morton", "clustered"), default="morton")
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


def rebuild_stats(eng):
    r = eng.last_rebuild_stats()
    st = {"rb_" + f: getattr(r, f) for f, _ in A.rt_rebuild_stats._fields_}
    if CLUSTERED:
        d = eng.last_rebuild_detail()
        assert d.builder == A.RT_BUILDER_CLUSTERED and not d.fell_back, "the clustered builder did not build the tree"
        st.update({f: getattr(d, f) for f in DETAIL})
    return st


CLUSTERED = args.builder == "clustered"
DETAIL = ("cluster_ms", "iterations", "cost_before", "cost_after")
sc = scenes.scene_c3_instanced(path_dir=args.scenes)
out = {"scene": "C3i", "lib_sha256_16": hashlib.sha256(open(M.engine.LIB_PATH, "rb").read()).hexdigest()[:16],
       "frames": args.frames}
if CLUSTERED:
    out["builder"] = args.builder
dyn = M.RayTracerEngine(sc, dynamic=True)
i0 = dyn.info()
out["create_dynamic_ms"] = i0.build_ms + i0.upload_ms
out["mrays_initial"] = throughput(dyn, args.frames)

# the 24 spheres are objects 1..24 (scale r, centre (cx, 5 + r, cz)): each moves along its own
# direction in the xz plane
rng = np.random.RandomState(9)
start = {i: np.array(sc.objects[i].transform, dtype=np.float64) for i in range(1, 25)}
dirs = {i: (lambda a: np.array([np.cos(a), 0.0, np.sin(a)]))(rng.uniform(0, 2 * np.pi)) for i in start}


def stage(diam, jitter=None):
    for i, m0 in start.items():
        m = m0.copy()
        m[12:15] += dirs[i] * (2.0 * m0[0]) * diam
        if jitter is not None:
            m[12:15] += jitter.normal(scale=0.01 * 2.0 * m0[0], size=3) * np.array([1.0, 0.0, 1.0])
        dyn.set_transform(i, m)


def timed_commit(rebuild):
    t0 = time.perf_counter()
    st = dyn.commit(rebuild="clustered" if rebuild and CLUSTERED else rebuild)
    return {"wall_ms": (time.perf_counter() - t0) * 1e3, "total_ms": st.total_ms, "refit_ms": st.refit_ms}


diams = [float(x) for x in args.diameters.split(",")]
plain, at = [], 0.0
out["displacements"] = []
for d in diams:
    for c in range(1, args.commits + 1):                   # plain commits walk there: the kept topology
        stage(at + (d - at) * c / args.commits)
        plain.append(timed_commit(False))
    at = d
    row = {"diameters": d, "refit": throughput(dyn, args.frames)}
    wall = timed_commit(True)                              # nothing staged: rebuilt at this pose
    row["rebuild"] = {**wall, **rebuild_stats(dyn)}
    row["rebuilt"] = throughput(dyn, args.frames)
    fresh = M.RayTracerEngine(copy.deepcopy(dyn.scene))
    fi = fresh.info()
    row["create_fresh_ms"] = fi.build_ms + fi.upload_ms
    row["fresh"] = throughput(fresh, args.frames)
    fresh.close()
    row["refit_over_fresh"] = row["refit"]["median"] / row["fresh"]["median"]
    row["rebuilt_over_fresh"] = row["rebuilt"]["median"] / row["fresh"]["median"]
    row["rebuilt_over_refit"] = row["rebuilt"]["median"] / row["refit"]["median"]
    out["displacements"].append(row)
    # back to the kept topology's state for the next displacement?  No: a rebuilt tree stays, and the
    # next displacement's "refit" figure would then start from it.  A new engine walks from the start.
    if d != diams[-1]:
        dyn.close()
        dyn = M.RayTracerEngine(copy.deepcopy(sc), dynamic=True)
        at = 0.0
for key in ("wall_ms", "total_ms", "refit_ms"):
    out["plain_commit_" + key] = spread([c[key] for c in plain])

jit = np.random.RandomState(10)
reb = []
for c in range(args.commits):
    stage(at, jit)
    r = timed_commit(True)
    r.update(rebuild_stats(dyn))
    reb.append(r)
assert all(r["rb_rebuilt"] == 1 for r in reb), "a rebuilding commit did not rebuild"
for key in ("wall_ms", "total_ms", "refit_ms", "rb_sort_ms", "rb_build_ms", "rb_total_ms") + (DETAIL if CLUSTERED else ()):
    out["rebuild_commit_" + key] = spread([r[key] for r in reb])
out["rebuild_tree"] = {k: reb[-1]["rb_" + k] for k in ("pairs", "nodes_before", "nodes_after", "depth_before", "depth_after")}
dyn.close()
out["ratio_rebuild_over_plain_commit"] = out["rebuild_commit_wall_ms"]["median"] / out["plain_commit_wall_ms"]["median"]
out["ratio_rebuild_over_create"] = out["rebuild_commit_wall_ms"]["median"] / out["displacements"][-1]["create_fresh_ms"]
for k, v in out.items():
    print(f"{k}: {v}")
print(json.dumps(out))
