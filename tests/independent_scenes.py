"""The tiny scenes that the independent tracer (independent_tracer.py) renders; test helper.

Every scene is small enough for an O(rays x primitives) tracer in Python: at most about 100
primitives, frames of 16x12 to 24x20 (at least two 8-row chunks, the last one shorter).  No two
surfaces coincide.  tests/golden/make_independent_golden.py freezes their frames.
"""
import math
import os

import numpy as np

import myraytracer_amd as M
from myraytracer_amd import scenes

NAMES = ("phong", "mirrors", "glass", "blur_quirk", "empty", "all_miss")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "independent")
_frozen = {}


def trs(t=(0.0, 0.0, 0.0), axis=(0.0, 1.0, 0.0), deg=0.0, s=(1.0, 1.0, 1.0)):
    """Column-major localToWorld of scale, then rotation about `axis`, then translation."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    c, sn = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + sn * K + (1 - c) * (K @ K)
    m = np.eye(4)
    m[:3, :3] = R @ np.diag(np.asarray(s, np.float64))
    m[:3, 3] = t
    return tuple(float(x) for x in m.T.reshape(-1))


def box_mesh(mid, material, shading="flat", **kw):
    """Unit cube, six quads, outward counter-clockwise."""
    P = np.array([[-.5, -.5, -.5], [.5, -.5, -.5], [.5, .5, -.5], [-.5, .5, -.5],
                  [-.5, -.5, .5], [.5, -.5, .5], [.5, .5, .5], [-.5, .5, .5]])
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 4, 7, 3), (1, 2, 6, 5), (0, 1, 5, 4), (3, 7, 6, 2)]
    F = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32) + 1
    return M.Mesh(id=mid, material=material, positions=P, indices=F, shading_mode=shading, **kw)


def quad_mesh(mid, material, corners, **kw):
    return M.Mesh(id=mid, material=material, positions=np.asarray(corners, np.float64),
                  indices=np.array([[1, 2, 3], [1, 3, 4]], np.int32), shading_mode="flat", **kw)


def ico_mesh(mid, material, level, shading, **kw):
    V, F = scenes.icosphere(level)
    return M.Mesh(id=mid, material=material, positions=V, indices=F.astype(np.int32), indices_one_based=False,
                  shading_mode=shading, **kw)


def floor(mid, material, y=-1.0, half=6.0):
    return quad_mesh(mid, material, [[-half, y, half], [half, y, half], [half, y, -half], [-half, y, -half]])


def _diffuse(kd, ks=(0.4, 0.4, 0.4), phong=24.0):
    return M.Material(ambient=(0.1, 0.1, 0.1), diffuse=kd, specular=ks, phong=phong)


def phong():
    """Flat and smooth meshes, a mesh with its own transform, three instances (rotated and
    non-uniformly scaled, mirrored, material override), a transformed sphere, a tilted plane with an
    unnormalised normal, a triangle, material ids 0 and 9 of three, two point lights, ambient,
    background above the horizon.  One sample per pixel."""
    cam = M.Camera(position=(0.3, 3.0, 7.0), gaze_point=(0.0, 0.9, 0.0), up=(0.0, 1.0, 0.0), fovy=42.0,
                   image_resolution=(24, 20))
    objs = [box_mesh(1, "1", transform=trs((-2.0, -0.1, 0.5), (0, 1, 0), 30.0, (1.2, 1.2, 1.2))),
            ico_mesh(2, "2", 0, "smooth", transform=trs((0.2, 0.2, 0.0), s=(0.9, 0.9, 0.9))),
            M.MeshInstance(id=3, base_mesh_id=2, transform=trs((2.3, 0.6, -0.5), (1, 1, 0), 40.0, (0.6, 1.1, 0.8))),
            M.MeshInstance(id=4, base_mesh_id=2, transform=trs((-0.6, 1.9, -1.5), (1, 0, 0), 20.0, (-0.8, 0.7, 0.9))),
            M.MeshInstance(id=5, base_mesh_id=1, material="3",
                           transform=trs((1.2, -0.2, 2.0), (0, 1, 0), -20.0, (0.7, 1.0, 0.7))),
            M.Sphere(center=(0.1, 0.0, 0.0), radius=0.5, material="2",
                     transform=trs((-1.8, 1.6, -2.0), (0, 0, 1), 25.0, (1.4, 0.8, 1.0))),
            M.Plane(center=(0.0, -1.0, 0.0), normal=(0.0, 2.0, 0.0), material="0", transform=trs(axis=(0, 0, 1), deg=2.0)),
            M.Triangle(vertices=((-3.5, -0.8, -3.5), (3.5, -0.8, -4.0), (0.3, 3.0, -4.2)), material="9")]
    mats = [_diffuse((0.7, 0.3, 0.2)), _diffuse((0.2, 0.6, 0.3), (0.6, 0.6, 0.6), 40.0),
            _diffuse((0.2, 0.3, 0.7), (0.3, 0.3, 0.3), 8.0)]
    return M.Scene(cameras=[cam], materials=mats, objects=objs,
                   point_lights=[M.PointLight((4.0, 6.0, 5.0), (3500.0, 3500.0, 3500.0)),
                                 M.PointLight((-5.0, 4.0, 2.0), (1500.0, 1200.0, 1000.0))],
                   ambient_light=(20.0, 20.0, 20.0), background_color=(5.0, 10.0, 20.0), max_recursion_depth=2)


def mirrors():
    """Mirror and conductor spheres, a rough-mirror box, a rough-conductor smooth icosphere; depth 3,
    four samples.  Cameras: lookAt with depth of field, nearPlane, lookAt without fovy."""
    cams = [M.Camera(position=(0.0, 1.5, 6.0), gaze_point=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=45.0,
                     image_resolution=(16, 12), num_samples=4, aperture_size=0.15, focus_distance=6.0),
            M.Camera(position=(3.0, 2.0, 5.0), gaze=(-0.5, -0.3, -1.0), up=(0.0, 1.0, 0.0), type="nearPlane",
                     near_plane=(-0.6, 0.6, -0.45, 0.45), near_distance=1.0, image_resolution=(16, 12), num_samples=4),
            M.Camera(position=(-3.0, 1.0, 5.0), gaze_point=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), near_distance=1.0,
                     image_resolution=(16, 12), num_samples=4)]
    mats = [_diffuse((0.6, 0.5, 0.4)),
            M.Material(ambient=(0.05, 0.05, 0.05), diffuse=(0.2, 0.2, 0.2), specular=(0.6, 0.6, 0.6), phong=64.0,
                       mirror=(0.7, 0.7, 0.75), type="mirror"),
            M.Material(ambient=(0.05, 0.05, 0.05), diffuse=(0.2, 0.2, 0.2), specular=(0.5, 0.5, 0.5), phong=30.0,
                       mirror=(0.9, 0.8, 0.6), ior=0.2, absorption_index=3.0, type="conductor"),
            M.Material(ambient=(0.05, 0.05, 0.05), diffuse=(0.2, 0.2, 0.2), specular=(0.5, 0.5, 0.5), phong=40.0,
                       mirror=(0.8, 0.8, 0.8), roughness=0.08, type="mirror"),
            M.Material(ambient=(0.05, 0.05, 0.05), diffuse=(0.1, 0.1, 0.2), specular=(0.4, 0.4, 0.4), phong=20.0,
                       mirror=(0.7, 0.8, 0.9), ior=0.4, absorption_index=2.5, roughness=0.12, type="conductor")]
    objs = [floor(1, "1"),
            M.Sphere(center=(-1.5, 0.0, 0.0), radius=1.0, material="2"),
            M.Sphere(center=(1.2, -0.2, 0.5), radius=0.8, material="3"),
            box_mesh(2, "4", transform=trs((0.0, -0.4, -2.5), (0, 1, 0), 25.0, (1.5, 1.0, 1.0))),
            ico_mesh(3, "5", 0, "smooth", transform=trs((0.2, 1.5, -0.5), s=(0.6, 0.6, 0.6))),
            M.Triangle(vertices=((-5.0, -0.9, -4.5), (5.0, -0.9, -4.5), (0.0, 5.0, -5.0)), material="1")]
    return M.Scene(cameras=cams, materials=mats, objects=objs,
                   point_lights=[M.PointLight((4.0, 6.0, 5.0), (3000.0, 3000.0, 3000.0)),
                                 M.PointLight((-5.0, 3.0, 2.0), (1200.0, 1000.0, 900.0))],
                   ambient_light=(20.0, 20.0, 20.0), background_color=(5.0, 10.0, 20.0), max_recursion_depth=3)


def glass():
    """A clear glass sphere, a closed absorbing glass box (rays leave it through total internal
    reflection), a second box of the same glass behind it (rays leaving the first hit the same
    material while not entering), a mirrored instance of it (negative determinant), an open sheet of that glass (its transmitted rays hit another
    material, so Beer is skipped), a rough dielectric sphere, a floor whose Phong exponent is below
    1, covers within a shadow epsilon behind the first area light and behind a second point light; two area lights and a point light; depth 4, four
    samples."""
    cam = M.Camera(position=(0.0, 1.5, 6.5), gaze_point=(0.0, 0.2, 0.0), up=(0.0, 1.0, 0.0), fovy=45.0,
                   image_resolution=(20, 12), num_samples=4)
    mats = [_diffuse((0.6, 0.5, 0.4), phong=0.6),           # exponent below 1: max(1, .) for point lights only
            M.Material(diffuse=(0.1, 0.1, 0.1), specular=(0.5, 0.5, 0.5), phong=50.0, ior=1.5, type="dielectric"),
            M.Material(diffuse=(0.05, 0.05, 0.05), specular=(0.4, 0.4, 0.4), phong=60.0, ior=1.5,
                       absorption=(0.3, 0.6, 0.9), type="dielectric"),
            M.Material(diffuse=(0.1, 0.1, 0.1), specular=(0.3, 0.3, 0.3), phong=20.0, ior=1.33, roughness=0.1,
                       type="dielectric")]
    objs = [floor(1, "1"),
            M.Sphere(center=(-1.6, 0.0, 0.0), radius=1.0, material="2"),
            box_mesh(2, "3", transform=trs((1.1, -0.2, 0.4), (0, 1, 0), 35.0, (1.4, 1.4, 1.4))),
            box_mesh(4, "3", transform=trs((1.45, -0.6, -1.4), (0, 1, 0), 35.0, (1.2, 0.6, 1.0))),
            # mirrored glass: the determinant flip turns its normals inwards, so `entering` is inverted
            M.MeshInstance(id=7, base_mesh_id=4, transform=trs((-0.3, -0.55, 1.6), (0, 1, 0), 15.0, (-0.7, 0.7, 0.7))),
            quad_mesh(3, "3", [[-0.7, -0.6, 2.6], [0.5, -0.6, 2.8], [0.5, 0.5, 2.8], [-0.7, 0.5, 2.6]]),
            M.Sphere(center=(0.0, 1.7, -1.0), radius=0.6, material="4"),
            # Shadow rays start one shadow epsilon along the ray, so tMax = dist - eps ends at an area
            # light's sample and tMax = dist ends one epsilon behind a point light.  A cover half an
            # epsilon behind the first area light must not shadow it; one a fifth of an epsilon behind
            # the second point light must.
            quad_mesh(5, "1", [[-1.0, 4.0005, 0.0], [1.0, 4.0005, 0.0], [1.0, 4.0005, 2.0], [-1.0, 4.0005, 2.0]]),
            quad_mesh(6, "1", [[-4.5, 5.0002, 3.5], [-3.5, 5.0002, 3.5], [-3.5, 5.0002, 4.5], [-4.5, 5.0002, 4.5]])]
    return M.Scene(cameras=[cam], materials=mats, objects=objs,
                   point_lights=[M.PointLight((4.0, 6.0, 5.0), (2500.0, 2500.0, 2500.0)),
                                 M.PointLight((-4.0, 5.0, 4.0), (800.0, 800.0, 800.0))],
                   area_lights=[M.AreaLight(position=(0.0, 4.0, 1.0), normal=(0.0, -1.0, 0.0),
                                            radiance=(40.0, 38.0, 30.0), size=1.5),
                                M.AreaLight(position=(-3.0, 2.5, 3.0), normal=(0.5, -0.5, -0.5),
                                            radiance=(10.0, 12.0, 20.0), size=0.8)],
                   ambient_light=(20.0, 20.0, 20.0), background_color=(5.0, 10.0, 20.0), max_recursion_depth=4)


def blur_quirk():
    """Mesh and triangle motion blur; numSamples 5 (four traced, divided by five); depth 0 with a
    mirror, whose `depth < maxDepth` is false.  The triangle moves within its own plane and is
    surrounded by nothing, see the tracer's docstring on its box."""
    cam = M.Camera(position=(0.0, 1.2, 6.0), gaze_point=(0.0, 0.1, 0.0), up=(0.0, 1.0, 0.0), fovy=45.0,
                   image_resolution=(16, 12), num_samples=5)
    mats = [_diffuse((0.6, 0.5, 0.4)), _diffuse((0.2, 0.5, 0.7)),
            M.Material(ambient=(0.05, 0.05, 0.05), diffuse=(0.2, 0.2, 0.2), specular=(0.6, 0.6, 0.6), phong=64.0,
                       mirror=(0.7, 0.7, 0.75), type="mirror")]
    objs = [floor(1, "1"),
            box_mesh(2, "2", transform=trs((-1.4, -0.3, 0.0), (0, 1, 0), 20.0), motion_blur=(0.7, 0.25, 0.0)),
            M.Sphere(center=(1.5, 0.0, 0.3), radius=0.9, material="3"),
            M.Triangle(vertices=((-0.8, 0.9, -1.0), (0.9, 1.0, -1.0), (0.1, 2.3, -1.0)), material="2",
                       motion_blur=(0.5, 0.3, 0.0))]
    return M.Scene(cameras=[cam], materials=mats, objects=objs,
                   point_lights=[M.PointLight((3.0, 6.0, 5.0), (3000.0, 3000.0, 3000.0))],
                   ambient_light=(20.0, 20.0, 20.0), background_color=(5.0, 10.0, 20.0), max_recursion_depth=0)


def empty():
    """No objects: no TLAS, every pixel is zero, not the background (Object+Extension.swift:98)."""
    cam = M.Camera(position=(0.0, 0.0, 5.0), gaze_point=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=45.0,
                   image_resolution=(16, 12), num_samples=4)
    return M.Scene(cameras=[cam], materials=[_diffuse((0.5, 0.5, 0.5))], objects=[],
                   point_lights=[M.PointLight((3.0, 6.0, 5.0), (3000.0, 3000.0, 3000.0))],
                   ambient_light=(20.0, 20.0, 20.0), background_color=(5.0, 10.0, 20.0), max_recursion_depth=2)


def all_miss():
    """Objects that no primary ray reaches: behind the camera and off to the side."""
    sc = empty()
    sc.objects = [M.Triangle(vertices=((-1.0, -1.0, 8.0), (1.0, -1.0, 8.0), (0.0, 1.0, 8.0)), material="1"),
                  M.Sphere(center=(30.0, 0.0, 0.0), radius=1.0, material="1")]
    return sc


def scene(name):
    return globals()[name]()


def cases():
    """Every (scene, camera)."""
    return [(name, cam) for name in NAMES for cam in range(len(scene(name).cameras))]


def frozen(name):
    """The committed independent/<name>.npz as a dict (read once)."""
    if name not in _frozen:
        with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
            _frozen[name] = {k: z[k] for k in z.files}
    return _frozen[name]


def frozen_selection(name, cam, first=0, step=1):
    """(rgb, rgba, (primary, shadow, secondary)) of a chunk selection, from the frozen file: chunks
    are independent of one another (the seeds are per pixel, jitterIndex restarts per chunk)."""
    z = frozen(name)
    rgb, rgba, rays = z[f"rgb_{cam}"], z[f"rgba_{cam}"], z[f"rays_{cam}"]
    sel = list(range(first, len(rays), step))
    rows = [r for c in sel for r in range(8 * c, min(8 * c + 8, rgb.shape[0]))]
    return rgb[rows], rgba[rows], tuple(int(x) for x in rays[sel].sum(axis=0))
