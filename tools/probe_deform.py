"""What does deforming a mesh cost?  C3's 1.02M-triangle mesh as a deformable scene, every vertex
displaced sinusoidally through 20 commits (rt_scene_set_mesh_positions + rt_scene_commit, deform.h),
against rt_scene_create of the same scene in the same process.

Reports (one JSON line, and the same as text):
  create_ms        rt_scene_create: build_ms + upload_ms of rt_scene_info, for the static, the dynamic
                   and the deformable scene, and for a fresh static scene at the deformed pose
  commit_*         median / min / max of the commits: the host clock around the call (positions staged
                   from a host array before the clock starts), rt_commit_stats.total_ms, and the
                   rt_deform_stats split (validate_ms, deform_ms, blas_refit_ms); with --device the
                   positions are a torch tensor on the GPU, passed in place
  mrays            Mrays/s (primary + shadow rays traversed) of the public submit/wait path, 16 renders
                   in flight, whole frames: the deformable scene at rest against the RT_SCENE_DYNAMIC
                   scene (the price of the FP64 layouts) and the static one, the deformed scene against
                   a fresh static scene built at that pose (refit / fresh)
usage: probe_deform.py [--frames 100] [--commits 20] [--device]
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
p.add_argument("--device", action="store_true", help="positions as a torch tensor on the GPU")
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
    return {"build_ms": i.build_ms, "upload_ms": i.upload_ms, "create_ms": i.build_ms + i.upload_ms,
            "device_bytes": int(i.device_bytes)}


def displaced(pos, c, n):
    """Every vertex moved: a travelling sine of 0.4 world units in y, a quarter of it in x and z."""
    ph = 2.0 * np.pi * c / n
    out = pos.copy()
    out[:, 1] += 0.4 * np.sin(0.35 * pos[:, 0] + 0.27 * pos[:, 2] + ph)
    out[:, 0] += 0.1 * np.sin(0.5 * pos[:, 2] + ph)
    out[:, 2] += 0.1 * np.cos(0.5 * pos[:, 0] + ph)
    return out


sc = scenes.scene_c3(inline=True)
rest = np.asarray(sc.objects[0].positions, np.float64).copy()
out = {"scene": "C3", "lib_sha256_16": hashlib.sha256(open(M.engine.LIB_PATH, "rb").read()).hexdigest()[:16],
       "frames": args.frames, "device_positions": bool(args.device)}

static = M.RayTracerEngine(copy.deepcopy(sc))
out["create_static"] = create_ms(static)
out["mrays_static_rest"] = throughput(static, args.frames)
static.close()

dyn = M.RayTracerEngine(copy.deepcopy(sc), dynamic=True)
out["create_dynamic"] = create_ms(dyn)
out["mrays_dynamic_rest"] = throughput(dyn, args.frames)
dyn.close()

dfm = M.RayTracerEngine(sc, deformable=True)
out["create_deformable"] = create_ms(dfm)
out["mrays_deformable_rest"] = throughput(dfm, args.frames)

commits = []
for c in range(1, args.commits + 1):
    q = displaced(rest, c, args.commits)
    if args.device:
        import torch
        t = torch.from_numpy(q).to("cuda:0").contiguous()
        torch.cuda.synchronize()
        dfm.set_positions(0, t, mirror=(c == args.commits))
    else:
        dfm.set_positions(0, q, mirror=(c == args.commits))
    t0 = time.perf_counter()
    st = dfm.commit()
    wall = (time.perf_counter() - t0) * 1e3
    ds = dfm.last_deform_stats()
    commits.append({"wall_ms": wall, "total_ms": st.total_ms, "bounds_ms": st.bounds_ms, "refit_ms": st.refit_ms,
                    "validate_ms": ds.validate_ms, "deform_ms": ds.deform_ms, "blas_refit_ms": ds.blas_refit_ms})
for key in commits[0]:
    v = [c[key] for c in commits]
    out["commit_" + key] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
out["commit_triangles"] = int(dfm.last_deform_stats().triangles)
out["mrays_deformable_deformed"] = throughput(dfm, args.frames)
final = copy.deepcopy(dfm.scene)
dfm.close()

fresh = M.RayTracerEngine(final)
out["create_fresh_final"] = create_ms(fresh)
out["mrays_fresh_final"] = throughput(fresh, args.frames)
fresh.close()

out["ratio_create_over_commit"] = out["create_deformable"]["create_ms"] / out["commit_wall_ms"]["median"]
out["ratio_deformable_over_dynamic"] = out["mrays_deformable_rest"]["median"] / out["mrays_dynamic_rest"]["median"]
out["ratio_refit_over_fresh"] = out["mrays_deformable_deformed"]["median"] / out["mrays_fresh_final"]["median"]
for k, v in out.items():
    print(f"{k}: {v}")
print(json.dumps(out))
