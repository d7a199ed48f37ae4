"""The first primary ray of every selected pixel, restated in numpy; test helper (no GPU, none of
the code under test).

first_rays() follows independent_tracer.IndependentTracer.render_chunk (its pixel loop, the lines
from `for j in range(r0, r1)` to the `timg` line) for the first sample, sx = sy = 0, with that
tracer's own camera() and PCG32: the seed with Swift's precedence quirk, two draws for the jitter,
the lens draws when aperture > 0 and focus > 0, one draw for time, the image-plane tMin.  With
centre=True it is the deterministic ray through (i + 0.5, j + 0.5): no lens offset, time 0, the
same tMin formula, nothing drawn.  tests/test_gbuffer_inputs.py shows that the oracle renders
exactly these rays before any GPU is involved.

ambient_scene() is the scene whose frame names the object every primary ray hit: no lights, so a
pixel is ambient_light * (its material's ambient), bit for bit, or the background."""
import numpy as np

import myraytracer_amd as M

import independent_scenes as IS
import independent_tracer as IT


def first_rays(scene, camera_index=0, chunk_first=0, chunk_step=1, centre=False):
    """dict(origins (rows, W, 3), dirs (rows, W, 3), tmin (rows, W), time (rows, W)) of the selected
    8-row chunks, rows packed in chunk order."""
    T = np.float64
    tr = IT.IndependentTracer.__new__(IT.IndependentTracer)     # camera() needs the scalar type only
    tr.T = T
    tr._vec = lambda v: np.array([T(x) for x in v], T)
    c = tr.camera(scene.cameras[camera_index])
    W, H, eye, u, v, w = c["W"], c["H"], c["eye"], c["u"], c["v"], c["w"]
    n = int(np.floor(np.sqrt(np.float64(c["spp"]))))
    dof = c["aperture"] > 0 and c["focus"] > 0
    plane_pt = eye - w * c["nd"]
    rows = [j for k in range(chunk_first, (H + 7) // 8, chunk_step) for j in range(8 * k, min(8 * k + 8, H))]
    out = dict(origins=np.zeros((len(rows), W, 3)), dirs=np.zeros((len(rows), W, 3)), tmin=np.zeros((len(rows), W)),
               time=np.zeros((len(rows), W)))
    with np.errstate(all="ignore"):
        for r, j in enumerate(rows):
            for i in range(W):
                rng = IT.PCG32((((j << 32) ^ i) + 0x9E3779B97F4A7C15) & IT.MASK64)
                if centre:
                    ci, cj = T(i) + T(0.5), T(j) + T(0.5)
                else:
                    x1 = rng.next_unit(T)
                    x2 = rng.next_unit(T)
                    ci = T(i) + (T(0) + x1) / T(n)
                    cj = T(j) + (T(0) + x2) / T(n)
                s = (c["q00"] - v * (cj * c["dv"])) + u * (ci * c["du"])
                d0 = IT.unit(s - eye)
                d, org = d0, eye
                if dof and not centre:
                    den = IT.dot(d0, -w)
                    tf = c["focus"] if abs(den) < 1e-6 else c["focus"] / den
                    ur = rng.next_unit(T) - 0.5
                    vr = rng.next_unit(T) - 0.5
                    org = eye + (ur * u + vr * v) * c["aperture"]
                    d = IT.unit((eye + d0 * tf) - org)
                time = T(0.0) if centre else rng.next_unit(T)
                den = IT.dot(d, w)
                timg = IT.dot(plane_pt - org, w) / (den if den != 0 else T(5e-324))
                out["origins"][r, i], out["dirs"][r, i] = org, d
                out["tmin"][r, i], out["time"][r, i] = max(timg, T(0.0)), time
    return out


# ------------------------------------------------------------------------------------ cameras
# |eye| / near_distance <= 100 on every one of them (tests/test_gpu_gbuffer.py derives its bound
# of 1e-12 from that).
def cameras(width=37, height=21):
    eye, at = (0.4, 2.2, 6.5), (0.1, 0.4, 0.0)
    return {
        "lookat": M.Camera(position=eye, gaze_point=at, up=(0.0, 1.0, 0.0), fovy=48.0, near_distance=1.0,
                           image_resolution=(width, height), num_samples=1),
        "lookat4": M.Camera(position=eye, gaze_point=at, up=(0.1, 1.0, 0.0), fovy=48.0, near_distance=0.5,
                            image_resolution=(width, height), num_samples=4),
        "nearplane": M.Camera(position=(0.2, 1.0, 7.0), up=(0.0, 1.0, 0.1), type="nearPlane", gaze=(0.0, -0.1, -1.0),
                              near_distance=1.5, near_plane=(-1.1, 0.9, -0.6, 0.7), image_resolution=(width, height),
                              num_samples=1),
        "dof": M.Camera(position=eye, gaze_point=at, up=(0.0, 1.0, 0.0), fovy=48.0, near_distance=1.0,
                        image_resolution=(width, height), num_samples=1, aperture_size=0.3, focus_distance=6.0),
    }


def ambient_scene(width=37, height=21):
    """Five objects, each with its own material and a distinct ambient; no lights; the background
    equals no product ambient_light * ambient."""
    amb = [(0.11, 0.23, 0.31), (0.47, 0.13, 0.29), (0.19, 0.53, 0.17), (0.37, 0.41, 0.59), (0.61, 0.07, 0.43)]
    mats = [M.Material(ambient=a, diffuse=(0.5, 0.5, 0.5), specular=(0.3, 0.3, 0.3), phong=16.0) for a in amb]
    objs = [IS.box_mesh(1, "1", transform=IS.trs((-1.9, 0.2, 0.4), (0, 1, 0), 25.0, (1.3, 1.3, 1.3))),
            IS.ico_mesh(2, "2", 1, "smooth", transform=IS.trs((0.3, 0.6, 0.0), s=(1.1, 1.1, 1.1))),
            IS.ico_mesh(3, "3", 1, "flat", transform=IS.trs((2.1, 0.9, -0.8), (1, 1, 0), 35.0, (0.7, 1.2, 0.8))),
            IS.quad_mesh(4, "4", [[-3.0, -0.7, 2.5], [3.0, -0.7, 2.5], [3.0, -0.7, -2.5], [-3.0, -0.7, -2.5]]),
            M.MeshInstance(id=5, base_mesh_id=2, material="5", transform=IS.trs((-0.5, 2.1, -1.2), s=(0.6, 0.6, 0.6)))]
    return M.Scene(cameras=[cameras(width, height)["lookat"]], materials=mats, objects=objs,
                   ambient_light=(13.0, 17.0, 19.0), background_color=(3.0, 5.0, 7.0), max_recursion_depth=2)


def ambient_colours(scene, mat, hit):
    """The frame the ambient scene's records name: ambient_light * materials[clamp(mat - 1)].ambient
    where `hit`, the background elsewhere; the shape of `mat` plus a colour axis."""
    al = np.asarray(scene.ambient_light, np.float64)
    amb = np.asarray([m.ambient for m in scene.materials], np.float64)
    idx = np.clip(np.asarray(mat, np.int64) - 1, 0, len(amb) - 1)
    return np.where(np.asarray(hit)[..., None], al * amb[idx], np.asarray(scene.background_color, np.float64))
