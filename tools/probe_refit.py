"""What does moving a scene cost?  C3i (terrain + 24 instances of one icosphere, the 25-instance
scene of the README's instanced figure) created static and dynamic, its 24 spheres moved by about
their own diameter through 20 commits, and a fresh scene created at the final pose.

Reports (one JSON line, and the same as text):
  create_ms        rt_scene_create: build_ms + upload_ms of rt_scene_info (PLY parse, SAH build, upload)
  commit_ms        median / min / max of the 20 rt_scene_commit calls (host clock around a call that
                   blocks until every replica is updated), with its bounds_ms and refit_ms parts
  mrays            Mrays/s (primary + shadow rays traversed) of the public submit/wait path, 16 renders
                   in flight, whole 1920x1080 frames: static and dynamic at the initial pose, the
                   dynamic scene after the moves (kept TLAS and fit-tree topology), and a fresh static
                   scene at that final pose
usage: probe_refit.py [--frames 200] [--commits 20]
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


def create_ms(eng):
    i = eng.info()
    return {"build_ms": i.build_ms, "upload_ms": i.upload_ms, "create_ms": i.build_ms + i.upload_ms}


sc = scenes.scene_c3_instanced(path_dir=args.scenes)
out = {"scene": "C3i", "lib_sha256_16": hashlib.sha256(open(M.engine.LIB_PATH, "rb").read()).hexdigest()[:16],
       "frames": args.frames}

static = M.RayTracerEngine(copy.deepcopy(sc))
out["create_static"] = create_ms(static)
out["mrays_static_initial"] = throughput(static, args.frames)
static.close()

dyn = M.RayTracerEngine(sc, dynamic=True)
out["create_dynamic"] = create_ms(dyn)
out["mrays_dynamic_initial"] = throughput(dyn, args.frames)

# the 24 spheres are objects 1..24 (scale r, centre (cx, 5 + r, cz)): each moves 2r along its own
# direction in the xz plane over the commits
rng = np.random.RandomState(9)
start = {i: np.array(sc.objects[i].transform, dtype=np.float64) for i in range(1, 25)}
dirs = {i: (lambda a: np.array([np.cos(a), 0.0, np.sin(a)]))(rng.uniform(0, 2 * np.pi)) for i in start}
commits = []
for c in range(1, args.commits + 1):
    for i, m0 in start.items():
        m = m0.copy()
        m[12:15] += dirs[i] * (2.0 * m0[0]) * c / args.commits
        dyn.set_transform(i, m)
    t0 = time.perf_counter()
    st = dyn.commit()
    commits.append({"wall_ms": (time.perf_counter() - t0) * 1e3, "total_ms": st.total_ms, "bounds_ms": st.bounds_ms,
                    "refit_ms": st.refit_ms, "moved": int(st.instances_moved)})
for key in ("wall_ms", "total_ms", "bounds_ms", "refit_ms"):
    v = [c[key] for c in commits]
    out["commit_" + key] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
out["commit_moved"] = commits[-1]["moved"]
out["mrays_dynamic_moved"] = throughput(dyn, args.frames)
final = copy.deepcopy(dyn.scene)
dyn.close()

fresh = M.RayTracerEngine(final)
out["create_fresh_final"] = create_ms(fresh)
out["mrays_fresh_final"] = throughput(fresh, args.frames)
fresh.close()

out["ratio_commit_over_create"] = out["commit_wall_ms"]["median"] / out["create_static"]["create_ms"]
out["ratio_dynamic_over_static"] = out["mrays_dynamic_initial"]["median"] / out["mrays_static_initial"]["median"]
out["ratio_refit_over_fresh"] = out["mrays_dynamic_moved"]["median"] / out["mrays_fresh_final"]["median"]
for k, v in out.items():
    print(f"{k}: {v}")
print(json.dumps(out))
