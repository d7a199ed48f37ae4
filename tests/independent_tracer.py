"""A second, BVH-free restatement of the reference's Whitted tracer (test helper, like
wide_tree_check.py).

Written from the Swift text alone, without reading oracle/rt_oracle.cpp or the kernels, so that a
misreading shared by the oracle and the kernels shows up as a disagreement between three
implementations (tests/test_independent_oracle.py, tests/test_gpu_independent.py).

What it restates, with the reference's lines (paths below Sources/RayTracer):
  pixel loop, chunks, seeds, sub-samples, DOF, time draw   Extensions/Object+Extension.swift:58-93, 285-356
  trace(): lights, mirror, dielectric, conductor, NaN guard Extensions/Object+Extension.swift:96-283
  camera basis                                               Extensions/Object+Extension.swift:382-427
  reflect, Beer, both Fresnels, orthonormalBasis             Extensions/Object+Extension.swift:467-552
  PCG32, stratified jitter table                             Extensions/Object+Extension.swift:556-589, 646-659
  scene assembly, smooth normals, instances, material index  Models/RTContext.swift:24-30, 122-401, 423-457
  triangle / sphere / plane intersectors                     Models/RTContext.swift:479-538
  world <-> local and the hit transfer                       Models/RTContext.swift:657-705
  shadow intersectors                                        Models/RTContext.swift:832-870
  RGBA8 clamp and truncate                                   RayTracer.swift:186-194

Structure: no BVH, and no boxes but the one named below.  The closest hit is the smallest accepted t over every primitive of
every instance; occlusion is any primitive passing the shadow test.  Every triangle of every
instance sits in one flat table and a ray is tested against the whole table at once (numpy over the
table; the ray itself is traced in plain Python).  The matrix inverse is Gauss-Jordan elimination
with partial pivoting.  Everything is generic over the scalar type: np.float64 and np.longdouble.

Assumptions about ParsingKit (absent from the reference tree): `Ray(origin:dir:time:)` starts with
tMin = 0, tMax = +inf and hit.t = +inf; `MeshInstance.transform` of the Scene dataclass is the
already-composed localToWorld.  Base meshes become instances in scene order (the reference walks a
Dictionary there, RTContext.swift:403, whose order is unspecified).

Deliberately out of scope:
  * Instance motion blur (`MeshInstance.motion_blur`).  The reference's instance bounds ignore the
    motion (makeInstance, RTContext.swift:437-457), so what it culls depends on how the TLAS groups
    instances into leaves; only a BVH restatement reproduces that.  The constructor refuses such a
    scene.  test_gpu_parity.py::test_motion_blur_instance and
    test_gpu_rays.py::test_motion_blur_times_and_tmin keep that case against the oracle.
  * Equal-t ties: order-dependent, covered in test_gpu_rays.py.  Here the first table entry wins.
  * Box culling at rounding distance, and plane hits beyond the plane's +-1e5 local box
    (RTContext.swift:172-174): `closest` raises if a scene produces one.
  * PLY meshes (`Mesh.ply_path`).

Disagreements settled so far (all in this file's disfavour):
  * A moving `Triangle` object.  The first version tested it wherever it moved and differed from
    the oracle on three pixels of the blur_quirk scene.  The reference gives the one-triangle BLAS
    the box of the resting triangle (RTContext.swift:212-223) and tests that box with the unshifted
    ray before the triangle (:557-571), so the part of the sweep that leaves the resting box is
    never hit.  That box depends on no tree, so it is restated here (`self.boxed`), for moving
    `Triangle` objects only.  Mesh triangles' boxes cover their sweep (:283-289, :348-354).

Ray tally: a primary ray per traced sub-sample, a shadow ray per call of `occluded`, a secondary ray
per recursive call of trace().
"""
from __future__ import annotations

import numpy as np

from myraytracer_amd import scene as S

CHUNK = 8                                                   # Object+Extension.swift:75
BRANCHES = ("tir", "beer_applied", "beer_skipped", "backface_glass_no_direct", "area_skip_ndotl",
            "rough_mirror", "rough_conductor", "rough_dielectric", "depth_limit", "miss",
            "smooth_hit", "neg_det_hit", "beer_not_entering")
# beer_not_entering: the refracted ray of a back-faced hit reached the same absorbing material, so
# only the reference's `entering` condition keeps Beer away (Object+Extension.swift:245)
RAYS = ("primary", "shadow", "secondary")
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------ PCG32
class PCG32:
    """Object+Extension.swift:556-589."""

    def __init__(self, seed: int):
        self.state = 0
        self.inc = ((seed << 1) | 1) & MASK64
        self.next()
        self.state = (self.state + 0x9E3779B97F4A7C15) & MASK64
        self.next()

    def next(self) -> int:
        old = self.state
        self.state = (old * 6364136223846793005 + self.inc) & MASK64
        x = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((x >> rot) | (x << ((-rot) & 31))) & 0xFFFFFFFF

    def next_unit(self, T):
        return T(self.next()) * T(2.0 ** -32)               # :585-588, exact in both types


def jitter_table(T):
    """buildStratifiedJitter, Object+Extension.swift:92-93, 646-659."""
    rng = PCG32(0x123456789ABCDEF)
    xs, ys = [], []
    for gy in range(10):
        for gx in range(10):
            xs.append(T(gx) + rng.next_unit(T))
            ys.append(T(gy) + rng.next_unit(T))
    return xs, ys


# ------------------------------------------------------------------------------- small maths
def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def unit(a):
    return a / np.sqrt(dot(a, a))


def inverse(m):
    """Gauss-Jordan with partial pivoting, in m's own scalar type."""
    n = m.shape[0]
    a = np.concatenate([m.copy(), np.eye(n, dtype=m.dtype)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        if a[p, c] == 0:
            raise ValueError("singular transform")
        if p != c:
            a[[c, p]] = a[[p, c]]
        a[c] = a[c] / a[c, c]
        for r in range(n):
            if r != c:
                a[r] = a[r] - a[r, c] * a[c]
    return a[:, n:]


def det3(m):
    return (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def tangent_frame(n, T):
    """orthonormalBasis, Object+Extension.swift:531-552."""
    s = T(1.0) if n[2] >= 0 else T(-1.0)
    a = T(-1.0) / (s + n[2])
    b = n[0] * n[1] * a
    tan = unit(np.array([T(1.0) + s * n[0] * n[0] * a, s * b, -s * n[0]], dtype=T))
    bit = unit(np.array([b, s + n[1] * n[1] * a, -n[1]], dtype=T))
    return tan, bit


def mirror_dir(d, n):
    """reflect, Object+Extension.swift:467."""
    return d - (2.0 * dot(d, n)) * n


def fresnel_dielectric(n1, n2, cos_i):
    """Object+Extension.swift:477-490: (R, cos of the refracted angle or None, sin^2 of it)."""
    c = min(max(abs(cos_i), 0.0), 1.0)
    eta = n1 / n2
    s2 = eta * eta * max(0.0, 1.0 - c * c)
    if s2 > 1.0:
        return 1.0, None, s2
    cp = np.sqrt(max(0.0, 1.0 - s2))
    rs = (n2 * c - n1 * cp) / (n2 * c + n1 * cp)
    rp = (n1 * c - n2 * cp) / (n1 * c + n2 * cp)
    return 0.5 * (rs * rs + rp * rp), cp, s2


def fresnel_conductor(eta, k, cos_i):
    """Object+Extension.swift:493-505; eta and k are scalars, so the three channels are equal."""
    c = min(max(abs(cos_i), 0.0), 1.0)
    c2 = c * c
    e = eta * eta + k * k
    two = 2.0 * eta * c
    rs = (e - two + c2) / (e + two + c2)
    rp = (e * c2 - two + 1.0) / (e * c2 + two + 1.0)
    return 0.5 * (rs + rp)


# ----------------------------------------------------------------------------------- hits
class Hit:
    __slots__ = ("t", "p", "n", "mat", "smooth", "neg_det", "kind", "inst")

    def __init__(self, t, p, n, mat, smooth, neg_det, kind, inst):
        self.t, self.p, self.n, self.mat = t, p, n, mat
        self.smooth, self.neg_det, self.kind, self.inst = smooth, neg_det, kind, inst


class _Instance:
    """makeInstance (RTContext.swift:437-457) without the bounds."""

    def __init__(self, m16, material, T):
        self.M = np.array([T(x) for x in np.asarray(m16, dtype=np.float64).reshape(-1)], dtype=T).reshape(4, 4).T
        self.Minv = inverse(self.M)
        self.NM = inverse(self.M[:3, :3]).T                 # normalTransformMatrix, :24-30
        self.neg = bool(det3(self.M[:3, :3]) < 0)            # :691-698
        self.material = int(material)


class IndependentTracer:
    def __init__(self, scene: S.Scene, dtype=np.float64):
        T = self.T = dtype
        self.scene = scene
        self.eps = T(scene.intersection_test_epsilon)
        self.seps = T(scene.shadow_ray_epsilon)
        self.max_depth = int(scene.max_recursion_depth)
        vec = self._vec
        self.materials = scene.materials
        self.background = vec(scene.background_color)
        self.ambient = vec(scene.ambient_light)
        self.mat_cache = {}
        self.jx, self.jy = jitter_table(T)
        self.point_lights = [(vec(l.position), vec(l.intensity)) for l in scene.point_lights]
        self.area_lights = [(vec(l.position), vec(l.normal), vec(l.radiance), T(l.size)) for l in scene.area_lights]
        self._assemble(scene)

    def _vec(self, v):
        return np.array([self.T(float(x)) for x in v], dtype=self.T)

    # ---------------------------------------------------------------- RTContext.init, :120-410
    def _assemble(self, scene):
        T = self.T
        insts, spheres, planes, tris = [], [], [], []       # primitives carry their instance's index
        by_id, mesh_ids, pending = {}, [], []
        for o in scene.objects:
            mat = S.material_index(o.material)               # :121, :423-426
            if isinstance(o, S.Sphere):                      # :122-160
                spheres.append((len(insts), self._vec(o.center), T(o.radius)))
                insts.append(_Instance(o.transform, mat, T))
            elif isinstance(o, S.Plane):                     # :161-192
                planes.append((len(insts), self._vec(o.center), self._vec(o.normal)))
                insts.append(_Instance(o.transform, mat, T))
            elif isinstance(o, S.Triangle):                  # :193-235: flat, its own instance
                v = [self._vec(p) for p in o.vertices]
                tris.append(([(len(insts))], [dict(v0=v[0], v1=v[1], v2=v[2], n=None, smooth=False,
                                                    mb=self._vec(o.motion_blur), own_box=True)]))
                insts.append(_Instance(o.transform, mat, T))
            elif isinstance(o, S.MeshInstance):              # :236-241
                m = o.material
                if m is None or m == "":
                    m = next((b.material for b in scene.objects if getattr(b, "id", None) == o.base_mesh_id), None)
                pending.append((o, S.material_index(m)))
            elif isinstance(o, S.Mesh):                      # :242-377
                if o.ply_path is not None:
                    raise NotImplementedError("PLY meshes are outside the independent tracer")
                recs = self._mesh_triangles(o)
                if recs:
                    by_id[o.id] = (recs, mat, o.transform)
                mesh_ids.append(o.id)
            else:
                raise TypeError(type(o))
        groups = []
        for o, mat in pending:                               # :384-401
            if any(float(x) != 0.0 for x in o.motion_blur):
                raise NotImplementedError("instance motion blur is outside the independent tracer")
            base = by_id.get(o.base_mesh_id)
            if base is None:
                continue
            groups.append((len(insts), base[0]))
            insts.append(_Instance(o.transform, mat, T))
            by_id[o.id] = (base[0], mat, o.transform)
        for mid in mesh_ids:                                 # :403-410
            base = by_id.get(mid)
            if base is not None:
                groups.append((len(insts), base[0]))
                insts.append(_Instance(base[2], base[1], T))
        for k, recs in groups:
            tris.append(([k] * len(recs), recs))
        self.insts, self.spheres, self.planes = insts, spheres, planes
        K = len(insts)
        self.A = np.stack([i.Minv[:3, :3] for i in insts]) if K else np.zeros((0, 3, 3), T)
        self.b = np.stack([i.Minv[:3, 3] for i in insts]) if K else np.zeros((0, 3), T)
        flat = [(k, r) for ks, rs in tris for k, r in zip(ks, rs)]
        self.ntri = len(flat)
        col = lambda f: np.array([f(r) for _, r in flat], dtype=T).reshape(-1, 3).T.copy()
        self.t_inst = np.array([k for k, _ in flat], dtype=np.int64)
        self.v0 = col(lambda r: r["v0"])
        self.e1 = col(lambda r: r["v1"] - r["v0"])          # :205, :277, :337
        self.e2 = col(lambda r: r["v2"] - r["v0"])
        self.mb = col(lambda r: r["mb"])
        self.t_smooth = [r["smooth"] for _, r in flat]
        # a moving Triangle object keeps the box of its resting position (:212): the one box here
        self.boxed = [(j, np.minimum(r["v0"], np.minimum(r["v1"], r["v2"])),
                       np.maximum(r["v0"], np.maximum(r["v1"], r["v2"])))
                      for j, (_, r) in enumerate(flat) if r.get("own_box") and bool((r["mb"] != 0).any())]
        self.t_norm = [r["n"] for _, r in flat]

    def _mesh_triangles(self, m):
        """:262-363 for inline meshes: positions + faces, optional per-vertex normals."""
        T = self.T
        pos = np.array([[T(float(x)) for x in p] for p in np.asarray(m.positions, np.float64).reshape(-1, 3)], dtype=T)
        idx = np.asarray(m.indices, np.int64).reshape(-1, 3) - (1 if m.indices_one_based else 0)
        smooth = m.shading_mode == "smooth"
        mb = self._vec(m.motion_blur)
        if m.normals is not None:                            # :267-297
            vn = np.array([[T(float(x)) for x in p] for p in np.asarray(m.normals, np.float64).reshape(-1, 3)], dtype=T)
        else:                                                # :298-326
            vn = np.zeros_like(pos)
            if smooth:
                for a, b, c in idx:
                    fn = unit(cross(pos[b] - pos[a], pos[c] - pos[a]))
                    vn[a] += fn
                    vn[b] += fn
                    vn[c] += fn
                with np.errstate(invalid="ignore", divide="ignore"):
                    vn = np.array([unit(v) for v in vn], dtype=T)
        out = []
        for a, b, c in idx:
            out.append(dict(v0=pos[a], v1=pos[b], v2=pos[c], smooth=smooth, mb=mb,
                            n=(vn[a], vn[b], vn[c]) if smooth else None))
        return out

    # ------------------------------------------------------------ world -> local, :657-669
    def _local(self, o, d):
        return self.A @ o + self.b, self.A @ d

    def _tri_candidates(self, ol, dl, time):
        """Moeller-Trumbore over the whole table (:479-494, :832-847): t and the rejection mask
        of everything but the t window."""
        k = self.t_inst
        org = ol.T[:, k] - self.mb * time
        dr = dl.T[:, k]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            pv = cross(dr, self.e2)
            det = dot(self.e1, pv)
            inv = 1.0 / det
            tv = org - self.v0
            u = dot(tv, pv) * inv
            q = cross(tv, self.e1)
            v = dot(dr, q) * inv
            t = dot(self.e2, q) * inv
            rej = (np.abs(det) < self.eps) | (u < 0) | (u > 1) | (v < 0) | (u + v > 1)
            for j, lo, hi in self.boxed:                     # hitAABB, :557-565, on the unshifted ray
                o, inv_d = ol[k[j]], 1.0 / dl[k[j]]
                t1, t2 = (lo - o) * inv_d, (hi - o) * inv_d
                near, far = np.fmin(t1, t2).max(), np.fmax(t1, t2).min()
                if not far >= max(near, self.eps):
                    rej[j] = True
        return t, u, v, rej

    def closest(self, o, d, tmin=0.0, time=0.0):
        """intersectTLAS (:619-720) without the tree: the accepted hit of least t, or None."""
        T = self.T
        if not self.insts:
            return None
        o, d, tmin, time = self._vec(o), self._vec(d), T(tmin), T(time)
        lim = max(self.eps, tmin)
        ol, dl = self._local(o, d)
        best_t, best = T(np.inf), None
        if self.ntri:
            t, u, v, rej = self._tri_candidates(ol, dl, time)
            with np.errstate(invalid="ignore"):
                ok = ~(rej | (t <= lim))
            if ok.any():
                j = int(np.argmin(np.where(ok, t, T(np.inf))))
                best_t, best = t[j], ("tri", j, u[j], v[j])
        for k, c, r in self.spheres:                         # :513-527
            oc = ol[k] - c
            a = dot(dl[k], dl[k])
            b = 2.0 * dot(oc, dl[k])
            disc = b * b - 4.0 * a * (dot(oc, oc) - r * r)
            if disc < 0:
                continue
            sd = np.sqrt(disc)
            t = (-b - sd) / (2.0 * a)
            if t < self.eps:
                t = (-b + sd) / (2.0 * a)
            if t <= lim or t >= best_t:
                continue
            best_t, best = t, ("sphere", k, c)
        for k, c, n in self.planes:                          # :530-538
            den = dot(n, dl[k])
            if abs(den) < self.eps:
                continue
            t = dot(c - ol[k], n) / den
            if t <= lim or t >= best_t:
                continue
            best_t, best = t, ("plane", k, n)
        if best is None:
            return None
        smooth = False
        if best[0] == "tri":                                 # :496-509
            j, u, v = best[1], best[2], best[3]
            k = int(self.t_inst[j])
            smooth = self.t_smooth[j]
            if smooth:
                n0, n1, n2 = self.t_norm[j]
                nl = unit((1.0 - u - v) * n0 + u * n1 + v * n2)
            else:
                nl = unit(cross(self.e1[:, j], self.e2[:, j]))
            pl = self.v0[:, j] + u * self.e1[:, j] + v * self.e2[:, j]
        elif best[0] == "sphere":
            k = best[1]
            pl = ol[k] + dl[k] * best_t
            nl = unit(pl - best[2])
        else:
            k = best[1]
            pl = ol[k] + dl[k] * best_t
            nl = unit(best[2])
            if np.abs(pl).max() > 1e5:
                raise ValueError("plane hit beyond the reference's +-1e5 plane box: out of scope")
        inst = self.insts[k]                                 # :679-705
        pw = inst.M[:3, :3] @ pl + inst.M[:3, 3]
        nw = unit(inst.NM @ nl)
        if inst.neg:
            nw = -nw
        return Hit(best_t, pw, nw, inst.material, smooth, inst.neg, best[0], k)

    def occluded(self, o, d, tmax, time=0.0, tmin=0.0):
        """occludedTLAS (:724-781) without the tree: any primitive passing its shadow test."""
        T = self.T
        if not self.insts:
            return False
        o, d, tmax, time = self._vec(o), self._vec(d), T(tmax), T(time)
        lim = max(self.eps, T(tmin))
        ol, dl = self._local(o, d)
        if self.ntri:                                        # :832-848
            t, _, _, rej = self._tri_candidates(ol, dl, time)
            with np.errstate(invalid="ignore"):
                if (~rej & (t > lim) & (t < tmax)).any():
                    return True
        for k, c, r in self.spheres:                         # :851-862
            oc = ol[k] - c
            a = dot(dl[k], dl[k])
            b = 2.0 * dot(oc, dl[k])
            disc = b * b - 4.0 * a * (dot(oc, oc) - r * r)
            if disc < 0:
                continue
            sd = np.sqrt(disc)
            t = (-b - sd) / (2.0 * a)
            if t < lim:
                t = (-b + sd) / (2.0 * a)
            if t > lim and t < tmax:
                return True
        for k, c, n in self.planes:                          # :865-870
            den = dot(n, dl[k])
            if abs(den) < self.eps:
                continue
            t = dot(c - ol[k], n) / den
            if t > lim and t < tmax:
                return True
        return False

    # ------------------------------------------------------------------ camera, :382-427
    def camera(self, cam):
        T = self.T
        W, H = max(1, int(cam.image_resolution[0])), max(1, int(cam.image_resolution[1]))
        eye, nd = self._vec(cam.position), T(cam.near_distance)
        if (cam.type or "").lower() == "lookat":
            w = -unit(self._vec(cam.gaze_point) - eye)
            if cam.fovy is not None:
                top = nd * np.tan(T(cam.fovy) * (np.arctan(T(1.0)) * 4) / T(360.0))
            else:
                top = nd * T(0.5)
            right = top * (T(W) / T(H))
            l, r, b, t = -right, right, -top, top
        else:
            l, r, b, t = (T(x) for x in cam.near_plane)
            w = -unit(self._vec(cam.gaze))
        u = unit(cross(unit(self._vec(cam.up)), w))
        v = unit(cross(w, u))
        return dict(W=W, H=H, eye=eye, u=u, v=v, w=w, nd=nd, du=(r - l) / T(W), dv=(t - b) / T(H),
                    q00=(eye - w * nd) + u * l + v * t, spp=max(1, int(cam.num_samples)),
                    aperture=T(cam.aperture_size), focus=T(cam.focus_distance))

    # ------------------------------------------------------------------- trace, :96-283
    def _material(self, raw):
        i = max(0, min(len(self.materials) - 1, raw - 1))    # :105
        m = self.mat_cache.get(i)
        if m is None:
            s, T = self.materials[i], self.T
            m = dict(ambient=self._vec(s.ambient), diffuse=self._vec(s.diffuse), specular=self._vec(s.specular),
                     mirror=self._vec(s.mirror), absorption=self._vec(s.absorption), phong=T(s.phong), ior=T(s.ior),
                     k=T(s.absorption_index), rough=T(s.roughness), type=s.type)
            self.mat_cache[i] = m
        return m

    def _shadowed(self, o, d, tmax, time, st):
        st["shadow"] += 1
        return self.occluded(o, d, tmax, time)

    def _trace(self, o, d, tmin, time, depth, rng, st):
        """Returns (radiance, hit or None).  st carries the tallies and the chunk's jitterIndex."""
        T = self.T
        if depth > self.max_depth:                           # :97
            st["depth_gt_max"] += 1
            return self.background, None
        if not self.insts:                                   # :98: no TLAS
            return np.zeros(3, T), None
        hit = self.closest(o, d, tmin, time)
        if hit is None:                                      # :101-103
            st["miss"] += 1
            return self.background, None
        st["smooth_hit"] += bool(hit.smooth)
        st["neg_det_hit"] += bool(hit.neg_det)
        m = self._material(hit.mat)
        p = hit.p
        front = dot(d, hit.n) < 0                            # :109-110
        N = hit.n if front else -hit.n
        glassy = m["ior"] > 0
        direct = (not glassy) or front                       # :115
        Lo = self.ambient * m["ambient"] if direct else np.zeros(3, T)
        if not direct:
            st["backface_glass_no_direct"] += 1
        else:
            view = unit(-d)
            for pos, inten in self.point_lights:             # :118-143
                wi = pos - p
                dist = np.sqrt(dot(wi, wi))
                wi = unit(wi)
                if self._shadowed(p + wi * self.seps, wi, dist, time, st):
                    continue
                ndl = max(0.0, dot(N, wi))
                if ndl > 0:
                    h = unit(wi + view)
                    ndh = max(0.0, dot(N, h))
                    spec = m["specular"] * np.power(T(ndh), max(T(1.0), m["phong"]))
                    Lo = Lo + (m["diffuse"] * ndl + spec) * (inten / max(dist * dist, 1e-12))
            for pos, nrm, rad, size in self.area_lights:     # :145-186
                nl = unit(nrm)
                tan, bit = tangent_frame(nl, T)
                area = size * size
                ji = st["jitter"] % 100
                r1 = self.jx[ji] / 10.0 - 0.5
                r2 = self.jy[ji] / 10.0 - 0.5
                st["jitter"] += 1
                wi = (pos + tan * (r1 * size) + bit * (r2 * size)) - p
                d2 = dot(wi, wi)
                dist = np.sqrt(d2)
                wi = wi / dist
                ndl = dot(N, wi)
                if ndl <= 0:
                    st["area_skip_ndotl"] += 1
                    continue
                lcos = abs(dot(nl, -wi))
                if lcos <= 0:
                    continue
                if self._shadowed(p + wi * self.seps, wi, dist - self.seps, time, st):
                    continue
                h = unit(wi + view)
                spec = m["specular"] * np.power(T(max(0.0, dot(N, h))), m["phong"])
                Lo = Lo + (m["diffuse"] * ndl + spec) * rad * (lcos / d2) * area
        kind = m["type"]
        if kind in ("mirror", "dielectric", "conductor") and not depth < self.max_depth:
            st["depth_limit"] += 1
        elif kind == "mirror":                               # :189-206
            rd = self._glossy(unit(mirror_dir(d, N)), m, rng, st, "rough_mirror")
            st["secondary"] += 1
            Li, _ = self._trace(p + N * self.seps, rd, T(0.0), time, depth + 1, rng, st)
            Lo = Lo + m["mirror"] * Li
        elif kind == "dielectric":                           # :207-251
            mn = N
            if m["rough"] != 0:
                st["rough_dielectric"] += 1
                tan, bit = tangent_frame(N, T)
                r1 = rng.next_unit(T) * 2.0 - 1.0
                r2 = rng.next_unit(T) * 2.0 - 1.0
                mn = unit(N + tan * r1 * m["rough"] + bit * r2 * m["rough"])
            n1, n2 = (T(1.0), m["ior"]) if front else (m["ior"], T(1.0))
            cos_i = -dot(d, mn)
            R, cos_t, s2 = fresnel_dielectric(n1, n2, cos_i)
            rd = unit(mirror_dir(d, mn))
            st["secondary"] += 1
            LiR, _ = self._trace(p + rd * self.seps, rd, T(0.0), time, depth + 1, rng, st)
            if cos_t is None or s2 > 1:
                st["tir"] += 1
                Lo = Lo + LiR
            else:
                eta = n1 / n2
                td = unit(d * eta + mn * (eta * cos_i - cos_t))
                st["secondary"] += 1
                LiT, thit = self._trace(p + td * self.seps, td, T(0.0), time, depth + 1, rng, st)
                if bool((m["absorption"] != 0).any()):                # :245-248
                    same = thit is not None and thit.mat == hit.mat
                    if front and same:
                        st["beer_applied"] += 1
                        x = max(thit.t, 0.0)
                        LiT = LiT * (np.exp(-m["absorption"] * x) if (np.isfinite(x) and x > 0) else LiT)
                    elif front:
                        st["beer_skipped"] += 1
                    elif same:                               # only `entering` keeps Beer away
                        st["beer_not_entering"] += 1
                Lo = Lo + LiR * R + LiT * (1.0 - R)
        elif kind == "conductor":                            # :252-275
            Rf = fresnel_conductor(m["ior"], m["k"], max(0.0, -dot(d, N)))
            rd = self._glossy(unit(mirror_dir(d, N)), m, rng, st, "rough_conductor")
            st["secondary"] += 1
            Li, _ = self._trace(p + N * self.seps, rd, T(0.0), time, depth + 1, rng, st)
            Lo = Lo + (Rf * m["mirror"]) * Li
        if not np.isfinite(Lo).all():                        # :277-280
            return np.zeros(3, T), hit
        return Lo, hit

    def _glossy(self, rd, m, rng, st, key):
        """:191-197 and :259-265."""
        if m["rough"] == 0:
            return rd
        st[key] += 1
        tan, bit = tangent_frame(rd, self.T)
        a = rng.next_unit(self.T) - 0.5
        b = rng.next_unit(self.T) - 0.5
        return unit(rd + (m["rough"] * a) * bit + (m["rough"] * b) * tan)

    # -------------------------------------------------------------- pixel loop, :285-356
    def render_chunk(self, camera_index, chunk):
        """One 8-row chunk: (rows x W x 3 radiance in the scalar type, ray tally, branch tally)."""
        T = self.T
        c = self.camera(self.scene.cameras[camera_index])
        W, H, eye, u, v, w = c["W"], c["H"], c["eye"], c["u"], c["v"], c["w"]
        r0, r1 = chunk * CHUNK, min(chunk * CHUNK + CHUNK, H)
        out = np.zeros((max(0, r1 - r0), W, 3), T)
        st = dict.fromkeys(BRANCHES + RAYS + ("depth_gt_max", "jitter"), 0)
        spp = c["spp"]
        n = int(np.floor(np.sqrt(np.float64(spp))))          # :300
        dof = c["aperture"] > 0 and c["focus"] > 0
        plane_pt = eye - w * c["nd"]
        for j in range(r0, r1):
            for i in range(W):
                # :294: Swift gives ^ and &+ the same (addition) precedence, left to right
                rng = PCG32((((j << 32) ^ i) + 0x9E3779B97F4A7C15) & MASK64)
                acc = np.zeros(3, T)
                done = 0
                for sy in range(n):
                    for sx in range(n):
                        x1 = rng.next_unit(T)
                        x2 = rng.next_unit(T)
                        ci = T(i) + (T(sx) + x1) / T(n)
                        cj = T(j) + (T(sy) + x2) / T(n)
                        s = (c["q00"] - v * (cj * c["dv"])) + u * (ci * c["du"])
                        d0 = unit(s - eye)
                        d, org = d0, eye
                        if dof:                              # :325-338
                            den = dot(d0, -w)
                            tf = c["focus"] if abs(den) < 1e-6 else c["focus"] / den
                            ur = rng.next_unit(T) - 0.5
                            vr = rng.next_unit(T) - 0.5
                            org = eye + (ur * u + vr * v) * c["aperture"]
                            d = unit((eye + d0 * tf) - org)
                        time = rng.next_unit(T)              # :340, always drawn
                        den = dot(d, w)
                        timg = dot(plane_pt - org, w) / (den if den != 0 else T(5e-324))
                        st["primary"] += 1
                        L, _ = self._trace(org, d, max(timg, T(0.0)), time, 0, rng, st)
                        acc = acc + L
                        done += 1
                        if done >= spp:
                            break
                    if done >= spp:
                        break
                out[j - r0, i] = acc / T(spp)                # :354
        return out, {k: st[k] for k in RAYS}, {k: st[k] for k in BRANCHES}

    def render(self, camera_index=0, chunk_first=0, chunk_step=1):
        """(radiance rows x W x 3 in the scalar type, RGBA8, ray tally, branch tally) of the selected
        chunks packed in chunk order, like OracleScene.render."""
        cam = self.scene.cameras[camera_index]
        H = max(1, int(cam.image_resolution[1]))
        parts = [self.render_chunk(camera_index, k) for k in range(chunk_first, (H + CHUNK - 1) // CHUNK, chunk_step)]
        return gather(parts, max(1, int(cam.image_resolution[0])), self.T)


def gather(parts, width, T=np.float64):
    """Chunk results -> (frame, RGBA8, ray tally, branch tally)."""
    rgb = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, width, 3), T)
    rays = {k: sum(p[1][k] for p in parts) for k in RAYS}
    branches = {k: sum(p[2][k] for p in parts) for k in BRANCHES}
    return rgb, to_rgba8(rgb), rays, branches


def to_rgba8(rgb):
    """RayTracer.swift:186-194: clamp to [0, 255], truncate, alpha 255."""
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = np.trunc(np.clip(rgb.astype(np.float64), 0.0, 255.0)).astype(np.uint8)
    return out
