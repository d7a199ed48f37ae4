"""Scenes, poses and ray sets of the deforming-mesh tests (tests/test_deform_inputs.py on the CPU,
tests/test_gpu_deform.py on the GPU).  Everything here is input: the CPU test shows that every
deformed pose compared with the oracle is free of equal-t ties (a refit tree re-walks ties in the
kept tree's order, a fresh oracle build in its own), the GPU tests use the same objects."""
import copy
import dataclasses

import numpy as np

import myraytracer_amd as M
from myraytracer_amd import scenes

# a single leaf run, a single record, and levels and reductions below, at and above a wave and a
# 256-thread block
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 5000)
VARIANTS = ("flat", "supplied_keep", "supplied_new", "smooth", "blur", "special")
FRAME = (48, 40)


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def m16(lin, t):
    m = np.eye(4)
    m[:3, :3] = lin
    m[:3, 3] = t
    return tuple(float(x) for x in m.T.reshape(-1))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def base_scene(variant="flat", sizes=SIZES, pose_seed=1):
    """Pose A.  Heightfield meshes of `sizes` triangles, each with a MeshInstance, under random
    poses (some mirrored); by variant: flat normals, supplied per-vertex normals, derived smooth
    normals, one blurred mesh, or flat with a sphere and a plane (no four-wide tree)."""
    assert variant in VARIANTS
    hp, hf = scenes.heightfield(50, 20.0, 2.0, 5)
    hp = hp.astype(np.float32).astype(np.float64)
    rng = np.random.RandomState(pose_seed)
    objs = []

    def pose(flip):
        s = rng.uniform(0.5, 2.0, size=3) * np.array([-1.0 if flip else 1.0, 1.0, 1.0])
        return m16(rotation(rng) @ np.diag(s), rng.uniform(-10.0, 10.0, size=3))

    for k, n in enumerate(sizes):
        blur = (0.1, 0.2, 0.05) if (variant == "blur" and n == 257) else (0.0, 0.0, 0.0)
        nrm = _unit(np.random.RandomState(900 + k), len(hp)) if variant.startswith("supplied") else None
        objs.append(M.Mesh(id=100 + k, material="1", positions=hp.copy(), indices=hf[:n].astype(np.int32),
                           indices_one_based=False, shading_mode="smooth" if variant == "smooth" else "flat",
                           normals=nrm, transform=pose(k % 3 == 1), motion_blur=blur))
    for k, n in enumerate(sizes):
        objs.append(M.MeshInstance(id=200 + k, base_mesh_id=100 + k, material="1", transform=pose(k % 4 == 0)))
    if variant == "special":
        objs.append(M.Sphere(center=(3.0, 6.0, -2.0), radius=2.5, material="1"))
        objs.append(M.Plane(center=(0.0, -30.0, 0.0), normal=(0.0, 1.0, 0.0), material="1"))
    sc = scenes.scaled(scenes.scene_c1(8, 8), *FRAME)
    sc.cameras[0] = M.Camera(position=(5.0, 38.0, 60.0), gaze_point=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=50.0,
                             near_distance=1.0, image_resolution=FRAME, type="lookAt")
    sc.point_lights = [M.PointLight((20.0, 60.0, 40.0), (9e3, 9e3, 9e3))]
    sc.objects = objs
    return sc


def mesh_indices(sc):
    return [i for i, o in enumerate(sc.objects) if isinstance(o, M.Mesh)]


def pose_b(sc, seed=7, with_normals=False, stretch=(2.5, 1.5, 3.0), noise=0.05):
    """object index -> (positions, normals or None): every mesh deformed by seeded noise plus a
    non-uniform stretch that moves geometry outside every old box."""
    out = {}
    for i in mesh_indices(sc):
        rng = np.random.RandomState(seed + 13 * i)
        p = np.asarray(sc.objects[i].positions, np.float64)
        q = p * np.asarray(stretch) + rng.normal(scale=noise, size=p.shape)
        out[i] = (q, _unit(rng, len(p)) if with_normals else None)
    return out


def small_step(pos, k, seed=3):
    """The k-th of a series of small deformations."""
    rng = np.random.RandomState(seed + k)
    return pos + rng.normal(scale=0.01, size=pos.shape) + 0.05 * np.sin(pos[:, [2, 0, 1]] + 0.3 * k)


def degenerate_pose(mesh, kind):
    """"point": every vertex at one point.  "zero_area": a few triangles far apart lose an edge (one
    vertex moved onto another); no two triangles become coincident."""
    p = np.asarray(mesh.positions, np.float64).copy()
    if kind == "point":
        return np.tile(p[0], (len(p), 1))
    idx = np.asarray(mesh.indices).reshape(-1, 3) - (1 if mesh.indices_one_based else 0)
    for t in range(0, len(idx), 50):
        p[idx[t, 1]] = p[idx[t, 0]]
    return p


def applied(sc, pose):
    """A copy of the scene with the pose written into its meshes (what the engine's mirror holds
    after set_positions)."""
    out = copy.deepcopy(sc)
    for i, (p, n) in pose.items():
        out.objects[i].positions = np.asarray(p, np.float64).copy()
        if n is not None:
            out.objects[i].normals = np.asarray(n, np.float64).copy()
    return out


def derived_vertex_normals(pos, idx):
    """The builder's derived smooth normals restated (RTContext.swift:303-330): unit face normals
    added to their three vertices in ascending triangle order, then normalised.  Vertices no
    triangle uses come out NaN (0 / 0) and are never read."""
    pos = np.asarray(pos, np.float64)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)

    def normalize(v):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = 1.0 / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            return v * r[:, None]

    a, b = pos[idx[:, 1]] - pos[idx[:, 0]], pos[idx[:, 2]] - pos[idx[:, 0]]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    acc = np.zeros_like(pos)
    np.add.at(acc, idx.reshape(-1), np.repeat(normalize(c), 3, axis=0))   # unbuffered, in index order
    return normalize(acc)


def reversed_faces(sc):
    """The same scene with each mesh's face list reversed in order (winding kept).  A mesh with
    derived smooth normals is given them as supplied normals: their sums depend on the face order,
    which is no tie."""
    out = copy.deepcopy(sc)
    for i in mesh_indices(out):
        o = out.objects[i]
        idx = np.asarray(o.indices).reshape(-1, 3) - (1 if o.indices_one_based else 0)
        if o.shading_mode == "smooth" and o.normals is None:
            o.normals = derived_vertex_normals(o.positions, idx)
        o.indices = np.ascontiguousarray(idx[::-1].astype(np.int32))
        o.indices_one_based = False
    return out


def axis_dirs():
    d = []
    for a in range(3):
        for s in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]; v[a] = s; d.append(v)
    return np.array(d)


def ray_set(n_random=1500, seed=23, center=(0.0, 0.0, 0.0), radius=25.0):
    """Random origins and random non-axis directions, plus a few axis-parallel rays; tmax for the
    occlusion queries; a ray time (used by blurred meshes)."""
    rng = np.random.RandomState(seed)
    c = np.asarray(center, np.float64)
    o = c + rng.uniform(-radius, radius, size=(n_random, 3))
    d = _unit(rng, n_random)
    ax = axis_dirs()
    oa = c + rng.uniform(-0.3 * radius, 0.3 * radius, size=(len(ax), 3))
    O, D = np.concatenate([o, oa]), np.concatenate([d, ax])
    tmax = rng.uniform(0.1, 60.0, size=len(O))
    time = rng.uniform(0.0, 1.0, size=len(O))
    return O, D, tmax, time


def aimed_ray_set(sc, n=1200, seed=9, radius=25.0):
    """Rays from random origins towards random interior points of the scene's triangles (sparse
    scenes), plus the random set's tmax and time."""
    rng = np.random.RandomState(seed)
    tris = world_triangles(sc)
    t = tris[rng.randint(len(tris), size=n)]
    w = rng.dirichlet((2.0, 2.0, 2.0), size=n)
    target = np.einsum("nk,nkc->nc", w, t)
    O = target.mean(0) + rng.uniform(-radius, radius, size=(n, 3))
    D = target - O
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    return O, D, rng.uniform(0.1, 60.0, size=n), rng.uniform(0.0, 1.0, size=n)


def combined_case():
    """Deformation and motion in one commit: the scene, the staged positions of mesh object 2 (257
    triangles), and object -> new transform for its MeshInstance (object 5) and for an instance of a
    mesh that keeps its shape (object 0)."""
    sc = base_scene("flat", sizes=(3, 65, 257))
    pose = {2: pose_b(sc)[2]}
    moves = {}
    for obj, d in ((5, (7.0, -3.0, 2.0)), (0, (0.0, 5.0, 0.0))):
        m = np.asarray(sc.objects[obj].transform, np.float64).reshape(4, 4).T.copy()
        m[:3, 3] += d
        moves[obj] = tuple(float(x) for x in m.T.reshape(-1))
    return sc, pose, moves


def grown_case(grown=True):
    """Two meshes and their instances under unit poses 5 apart in y (no coincident triangles), and
    the factor 2^18 their vertices grow by (|coordinate| about 10 -> 2.6e6); grown: at that pose."""
    sc = base_scene("flat", sizes=(65, 257))
    s = 2.0 ** 18
    for k, o in enumerate(sc.objects):
        o.transform = m16(np.eye(3), (0.0, 5.0 * k, 0.0))
        if grown and isinstance(o, M.Mesh):
            o.positions = np.asarray(o.positions, np.float64) * s
    return sc, s


def ply_case(directory):
    """base_scene("flat", (65, 257)) with its second mesh read from a PLY that carries per-vertex
    normals, and pose B for both meshes."""
    sc = base_scene("flat", sizes=(65, 257))
    o = sc.objects[1]
    path = directory + "/deform_257.ply"
    scenes.write_ply(path, np.asarray(o.positions), np.asarray(o.indices).reshape(-1, 3),
                     normals=_unit(np.random.RandomState(77), len(o.positions)))
    sc.objects[1] = M.Mesh(id=o.id, material=o.material, ply_path=path, shading_mode="smooth", transform=o.transform)
    return sc, pose_b(base_scene("flat", sizes=(65, 257)))


def world_triangles(sc):
    """(T, 3, 3) world-space vertices of every instance's triangles (no blur)."""
    by_id, out = {}, []
    for o in sc.objects:
        if isinstance(o, M.Mesh):
            pos = np.asarray(o.positions, np.float64)
            idx = np.asarray(o.indices, np.int64).reshape(-1, 3) - (1 if o.indices_one_based else 0)
            by_id[o.id] = pos[idx]
    for o in sc.objects:
        if isinstance(o, (M.Mesh, M.MeshInstance)):
            v = by_id[o.id if isinstance(o, M.Mesh) else o.base_mesh_id]
            m = np.asarray(o.transform, np.float64).reshape(4, 4).T
            out.append(v @ m[:3, :3].T + m[:3, 3])
    return np.concatenate(out)


def closest_gap(tris, O, D, eps=1e-6, chunk=64):
    """Vectorised Moeller-Trumbore over all (ray, triangle) pairs: per ray the smallest t and the
    relative gap (t2 - t1) / t1 to the second smallest (inf with fewer than two hits)."""
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    t1 = np.full(len(O), np.inf)
    gap = np.full(len(O), np.inf)
    for a in range(0, len(O), chunk):
        o, d = O[a:a + chunk, None, :], D[a:a + chunk, None, :]
        p = np.cross(d, e2[None])
        det = np.einsum("rtk,tk->rt", p, e1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s = o - v0[None]
            u = np.einsum("rtk,rtk->rt", s, p) * inv
            q = np.cross(s, e1[None])
            v = np.einsum("rtk,rtk->rt", np.broadcast_to(d, q.shape), q) * inv
            t = np.einsum("rtk,tk->rt", q, e2) * inv
        ok = (np.abs(det) >= eps * 1e-6) & (u >= -1e-9) & (v >= -1e-9) & (u + v <= 1 + 1e-9) & (t > 0)
        t = np.where(ok, t, np.inf)
        part = np.partition(t, 1, axis=1)[:, :2]
        t1[a:a + chunk] = part[:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap[a:a + chunk] = np.where(np.isfinite(part[:, 1]), (part[:, 1] - part[:, 0]) / part[:, 0], np.inf)
    return t1, gap


# ---- a C2-like mirror mesh (full frames: shadows, reflections, optionally a dielectric sphere)
def c2_like(dielectric):
    sc = scenes.scaled(scenes.scene_c2(inline=True), 64, 48)
    pos, faces = scenes.geometry_c2(48, 26)
    sc.objects[0].positions = pos.astype(np.float32).astype(np.float64)
    sc.objects[0].indices = faces.astype(np.int32)
    sc.materials[0] = dataclasses.replace(sc.materials[0], mirror=(0.5, 0.5, 0.5), type="mirror")
    sc.max_recursion_depth = 3
    if dielectric:
        sc.materials.append(M.Material(ambient=(0.05, 0.05, 0.05), diffuse=(0.1, 0.1, 0.1), specular=(0.3, 0.3, 0.3),
                                       phong=16.0, mirror=(0.9, 0.9, 0.9), ior=1.5, absorption=(0.02, 0.03, 0.01),
                                       type="dielectric"))
        sc.objects.append(M.Sphere(center=(1.3, 0.2, 1.0), radius=0.45, material=str(len(sc.materials))))
    return sc


def wobble(pos, k=1.0):
    return pos * np.array([1.15, 0.85, 1.1]) + 0.06 * k * np.sin(5.0 * pos[:, [1, 2, 0]] + 0.7)
