"""What does a first-hit buffer cost, in which lane mapping, and against the routes a caller had?


C3 at 1920x1080 (the four-wide identity walk), then C3i (the flattened instance tree), on device
tensors, outputs t + ids + normal:
  gbuffer tiles   rt_render_gbuffer, one 8x8 tile per wave in xcd_tile order (gbuffer_tiles = 1)
  gbuffer rows    rt_render_gbuffer, 64 consecutive pixels of a row per wave (gbuffer_tiles = 0)
  gbuffer rays    rt_render_gbuffer asking for the rays alone (the small kernel)
  query           rt_query_closest with declared bounds on those same rays with their tmin and time,
                  exported once beforehand: the route the parent commit offered, given correct rays
  frame           rt_render_device of the frame itself, for scale
Before anything is timed the three record routes are compared: they must agree bit for bit.
Every figure is the median (min .. max) in ms of `--reps` timed calls after two warm-up calls, on
the host clock around the call and a device synchronise, all in one process.  Prints text and one
JSON line per figure, with the library's sha-256 prefix.
usage: probe_gbuffer.py [--reps 7] [--scenes c3,c3i] [--width 1920 --height 1080]
The probe needs a GPU; nothing falls back."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="c3,c3i")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import torch
    import myraytracer_amd as M
    from myraytracer_amd import _abi as A
    from myraytracer_amd import scenes
    assert torch.cuda.is_available(), "probe_gbuffer.py needs a GPU"
    lib = M.load_library()
    sha = hashlib.sha256(open(M.engine.LIB_PATH, "rb").read()).hexdigest()[:16]
    W, H = args.width, args.height
    n = W * H
    print(f"probe_gbuffer: {W}x{H}, {args.reps} reps, libmyrt sha256 {sha}", flush=True)

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

    def dev(shape, dtype):
        return torch.empty(shape, dtype=dtype, device="cuda:0")

    for name in args.scenes.split(","):
        sc = {"c3": scenes.scene_c3, "c3i": scenes.scene_c3_instanced}[name](width=W, height=H, inline=True)
        eng = M.RayTracerEngine(sc)
        rays = {"origins": dev((H, W, 3), torch.float64), "dirs": dev((H, W, 3), torch.float64),
                "tmin": dev((H, W), torch.float64), "time": dev((H, W), torch.float64)}
        eng.first_hits(out=rays)                             # the rays, exported once
        b = eng.last_query_stats().bounds
        bounds = A.rt_query_bounds(b.origin_reach, b.origin_coord, b.dir_norm)
        rec = [{"t": dev((H, W), torch.float64), "ids": dev((H, W, 4), torch.int32),
                "normal": dev((H, W, 3), torch.float64)} for _ in range(3)]
        frame = dev((H, W, 3), torch.float64)
        stream = torch.cuda.current_stream().cuda_stream
        rb = A.rt_ray_batch(rays["origins"].data_ptr(), rays["dirs"].data_ptr(), rays["tmin"].data_ptr(),
                            rays["time"].data_ptr())
        hb = A.rt_hit_batch()
        hb.t, hb.ids, hb.normal = rec[2]["t"].data_ptr(), rec[2]["ids"].data_ptr(), rec[2]["normal"].data_ptr()

        def gbuffer(tiles, out):
            eng.set_option("gbuffer_tiles", tiles)
            eng.first_hits(out=out)

        def query():
            rc = lib.rt_query_closest(eng.handle, 0, n, C.byref(rb), C.byref(hb), C.byref(bounds), A.RT_QUERY_DEVICE,
                                      C.c_void_p(stream or None))
            assert rc == A.RT_OK, lib.rt_last_error()

        gbuffer(1, rec[0]); gbuffer(0, rec[1]); query()
        torch.cuda.synchronize()
        st = eng.last_query_stats()
        assert st.out_of_bounds == 0 and st.non_finite == 0, "the camera's bounds flagged a ray"
        for f in rec[0]:
            assert torch.equal(rec[0][f], rec[1][f]) and torch.equal(rec[0][f], rec[2][f]), f"{f}: the routes differ"
        hits = float(torch.isfinite(rec[0]["t"]).double().mean())
        variants = [("gbuffer tiles", lambda: gbuffer(1, rec[0])), ("gbuffer rows", lambda: gbuffer(0, rec[1])),
                    ("gbuffer rays", lambda: eng.first_hits(out=rays)), ("query", query),
                    ("frame", lambda: eng.render_device(frame.data_ptr(), 0, 0, 1, stream=stream))]
        for vname, fn in variants:
            ms = timed(fn)
            med = statistics.median(ms)
            r = {"probe": "gbuffer", "scene": name, "variant": vname, "pixels": n, "walk": int(st.walk),
                 "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                 "mpixels_s": round(n / med / 1e3, 1), "hit_fraction": round(hits, 4), "lib_sha256": sha}
            print(f"{name:4s} {vname:14s} {med:9.3f} ms ({min(ms):.3f} .. {max(ms):.3f})  {r['mpixels_s']:9.1f} Mpixels/s",
                  flush=True)
            print("JSON " + json.dumps(r), flush=True)
        eng.close()
        del rays, rec, frame


if __name__ == "__main__":
    main()
