"""Python host mirror of the reference's public engine API.

`RayTracerEngine` mirrors `RayTracerEngine` (RT/RayTracer.swift:25-228): it is built
from a scene (init(from:data:) :30-49), answers `inspect` (:52-67) and renders one
camera (`render`, :115-131) or all cameras (`render_all`, :70-102), returning
`RenderResult`s with RGBA8 pixels (:186-195) and `RenderStats` (Models/RenderStats.swift).

Every render goes through libmyrt.so's C ABI (include/rtcore.h) into the HIP kernels;
there is no CPU fallback — if the library or a GPU is missing, construction fails.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _abi as A
from .scene import Scene

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmyrt.so")
_lib = None


class RenderError(RuntimeError):
    """Raised for a negative rtcore status (NSError equivalents, RayTracer.swift:121,141-154)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"[{code}] {message}")
        self.code = code


def load_library() -> C.CDLL:
    """Load the in-tree HIP library.  torch is imported first so the process has ONE HIP
    runtime (libmyrt.so then binds to torch's libamdhip64.so.7 by SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MYRT_LIB") or LIB_PATH      # MYRT_LIB: A/B a tuning variant (tools/build_variants.sh)
    if not os.path.exists(path):
        raise RenderError(A.RT_ERR_NO_RENDERER,
                          f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        import torch  # noqa: F401  (shared HIP runtime)
    except Exception:  # pragma: no cover - torch is part of the image
        pass
    _lib = A.bind(C.CDLL(path))
    return _lib


def _check(rc: int):
    if rc != A.RT_OK:
        msg = load_library().rt_last_error()
        raise RenderError(rc, msg.decode() if msg else "")


@dataclass
class RenderStats:                       # Models/RenderStats.swift:8-24 (+ ray counts)
    meshes: int
    triangles: int
    spheres: int
    planes: int
    rays: int                            # primary + shadow (the reference always reported 0)
    primary_rays: int
    shadow_rays: int
    secondary_rays: int
    milliseconds: float
    kernel_ms: float
    shadow_rays_traced: int = 0          # shadow rays whose any-hit walk ran (<= shadow_rays)
    rewalked: int = 0                    # closest-hit rays re-walked in reference order (equal-t ties)

    @property
    def rays_traced(self) -> int:
        return self.primary_rays + self.shadow_rays_traced


@dataclass
class CameraSpec:                        # Models/RenderConfig.swift:19-25
    index: int
    id: Optional[str]
    image_name: Optional[str]
    width: int
    height: int


@dataclass
class SceneInfo:                         # Models/RenderConfig.swift:27-33
    cameras: List[CameraSpec]
    meshes: int
    triangles: int
    spheres: int
    planes: int


@dataclass
class RenderResult:                      # Models/RenderResult.swift:10-15 (CGImage -> arrays)
    file_name: Optional[str]
    rgba8: np.ndarray                    # (H, W, 4) uint8, row 0 = top
    rgb: np.ndarray                      # (H, W, 3) float64 — Renderer.render's [Vec3]
    camera: CameraSpec
    stats: RenderStats


@dataclass
class RenderProgress:                    # Models/RenderProgress.swift:8-14
    fraction: float
    message: Optional[str] = None


class RayTracerEngine:
    """Device-resident scene + renderer (one full replica per listed GPU)."""

    def __init__(self, scene: Scene, devices: Optional[Sequence[int]] = None, dynamic: bool = False,
                 deformable: bool = False):
        """dynamic: instances and cameras may move between renders (set_transform / set_camera /
        commit; rt_scene_create_ex with RT_SCENE_DYNAMIC).  deformable: mesh vertices may move as
        well (set_positions; RT_SCENE_DEFORMABLE, which implies dynamic)."""
        lib = load_library()
        self.scene = scene
        self._packed = scene.to_desc()
        handle = C.c_void_p()
        devs = list(devices) if devices else [0]
        arr = (C.c_int32 * len(devs))(*devs)
        flags = (A.RT_SCENE_DYNAMIC if dynamic else 0) | (A.RT_SCENE_DEFORMABLE if deformable else 0)
        if flags:
            _check(lib.rt_scene_create_ex(self._packed.ptr, arr, len(devs), flags, C.byref(handle)))
        else:
            _check(lib.rt_scene_create(self._packed.ptr, arr, len(devs), C.byref(handle)))
        self._h = handle
        self.devices = devs
        self.deformable = bool(deformable)
        self.dynamic = bool(dynamic) or self.deformable

    @classmethod
    def from_file(cls, path, format: str = "auto", devices: Optional[Sequence[int]] = None) -> "RayTracerEngine":
        """RayTracerEngine.init(from: url) (RayTracer.swift:30-34): JSON or XML scene file."""
        from . import sceneio
        return cls(sceneio.load(path, format), devices)

    @classmethod
    def from_data(cls, data, format: str = "auto", devices: Optional[Sequence[int]] = None,
                  base_dir: Optional[str] = None) -> "RayTracerEngine":
        """RayTracerEngine.init(data:) (RayTracer.swift:35-36)."""
        from . import sceneio
        return cls(sceneio.loads(data, format, base_dir), devices)

    # -- lifecycle
    def close(self):
        if getattr(self, "_h", None):
            load_library().rt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    # -- render options (rt_scene_set_option; defaults are the production settings)
    def set_option(self, name: str, value: int):
        _check(load_library().rt_scene_set_option(self._h, name.encode(), int(value)))

    def set_unsafe_option(self, name: str, value: int):
        """Test hooks (debug_fail_replica, wide_delta_scale, debug_fail_commit_alloc,
        debug_fail_commit_step, ...) through the non-production rt_scene_set_unsafe_option;
        set_option refuses them."""
        _check(load_library().rt_scene_set_unsafe_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int64()
        _check(load_library().rt_scene_get_option(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    # -- dynamic scenes (RTContext.refitTLAS, RTContext.swift:883-927)
    def instance_of(self, object_index: int) -> int:
        """The instance scene object `object_index` produced (-1: none)."""
        k = C.c_int32(-1)
        _check(load_library().rt_scene_instance_of_object(self._h, int(object_index), C.byref(k)))
        return int(k.value)

    def set_transform(self, object_index: int, m16):
        """Stage a new column-major localToWorld for the instance of scene object `object_index`
        (applied by commit()); self.scene.objects[object_index].transform follows, so
        oracle.OracleScene(self.scene) is the reference scene for the engine's next committed state."""
        m = np.ascontiguousarray(np.asarray(m16, dtype=np.float64).reshape(-1))
        if m.size != 16:
            raise ValueError("a transform is 16 values, column-major")
        k = self.instance_of(object_index) if self.dynamic else 0
        if k < 0:
            raise RenderError(A.RT_ERR_INVALID_ARG, f"object {object_index} produced no instance")
        _check(load_library().rt_scene_set_instance_transform(self._h, k, m.ctypes.data_as(A.c_double_p)))
        self.scene.objects[object_index].transform = tuple(float(x) for x in m)

    def set_camera(self, index: int, camera):
        """Replace camera `index` (takes effect at once); self.scene.cameras[index] follows."""
        from .scene import pack_camera
        cc = pack_camera(camera)
        _check(load_library().rt_scene_set_camera(self._h, int(index), C.byref(cc)))
        self.scene.cameras[index] = camera

    def commit(self, rebuild=False) -> A.rt_commit_stats:
        """Apply the staged transforms (rt_scene_commit): blocks until every replica is updated.
        With `rebuild` the flattened instance tree is then built again on the device for the new
        pose (rt_scene_commit_ex): True takes the Morton builder (RT_COMMIT_REBUILD_FIT),
        "clustered" the clustered one (RT_COMMIT_REBUILD_FIT_CLUSTERED); last_rebuild_stats() and
        last_rebuild_detail() say what happened.
        How it ends (rtcore.h "how a commit ends"): a RenderError with RT_ERR_INVALID_ARG or RT_ERR_OOM
        changed nothing - what was staged is dropped, the last_*_stats() keep the last successful
        commit's, and self.scene (which follows staging) describes a pose the engine never took.
        Without memory for the rebuild the pose is committed and the old tree refit:
        last_rebuild_stats().reason == RT_REBUILD_NO_MEMORY.  A RenderError with RT_ERR_DEVICE means
        the scene is lost: every later render, submit, query, commit, fit_cost and wide_read of this
        engine raises RT_ERR_DEVICE; close() it and build a new one."""
        st = A.rt_commit_stats()
        lib = load_library()
        if isinstance(rebuild, str):
            if rebuild != "clustered":
                raise ValueError('rebuild is False, True or "clustered"')
            _check(lib.rt_scene_commit_ex(self._h, A.RT_COMMIT_REBUILD_FIT_CLUSTERED, C.byref(st)))
        elif rebuild:
            _check(lib.rt_scene_commit_ex(self._h, A.RT_COMMIT_REBUILD_FIT, C.byref(st)))
        else:
            _check(lib.rt_scene_commit(self._h, C.byref(st)))
        return st

    def last_rebuild_stats(self) -> A.rt_rebuild_stats:
        """What the last commit() did for a rebuild (rt_scene_last_rebuild_stats): zeros when it
        asked for none; rebuilt = 0 and a reason (RT_REBUILD_*) when the old tree stayed."""
        st = A.rt_rebuild_stats()
        _check(load_library().rt_scene_last_rebuild_stats(self._h, C.byref(st)))
        return st

    def last_rebuild_detail(self) -> A.rt_rebuild_detail:
        """Which builder made the tree of the last commit() (rt_scene_last_rebuild_detail): zeros
        when it asked for no rebuild; builder 1 Morton, 2 clustered; the clustering's iterations and
        time, whether it fell back to Morton, and the tree cost before and after."""
        st = A.rt_rebuild_detail()
        _check(load_library().rt_scene_last_rebuild_detail(self._h, C.byref(st)))
        return st

    def fit_cost(self) -> float:
        """The cost of the flattened instance tree in use now (rt_scene_fit_cost): summed slot-box
        surface areas over the root's; 0.0 when the scene has no such tree.  Lower is better."""
        c = C.c_double(0.0)
        _check(load_library().rt_scene_fit_cost(self._h, C.byref(c)))
        return float(c.value)

    # -- instance visibility (rtcore.h "instance visibility")
    def set_visible(self, object_index: int, visible: bool):
        """Stage hiding (False) or showing (True) the instance of scene object `object_index`;
        commit() applies it.  Instance and object indices never change."""
        k = self.instance_of(object_index) if self.dynamic else 0
        if k < 0:
            raise RenderError(A.RT_ERR_INVALID_ARG, f"object {object_index} produced no instance")
        _check(load_library().rt_scene_set_instance_visible(self._h, k, 1 if visible else 0))

    def set_visible_many(self, object_indices, visible):
        """set_visible for several objects: `visible` is one flag for all, or one per object.
        Objects whose instances are consecutive go down in one rt_scene_set_instances_visible call."""
        objs = [int(o) for o in object_indices]
        flags = [bool(visible)] * len(objs) if isinstance(visible, (bool, int, np.bool_)) else [bool(v) for v in visible]
        if len(flags) != len(objs):
            raise ValueError("one flag per object")
        inst = [self.instance_of(o) if self.dynamic else 0 for o in objs]
        for o, k in zip(objs, inst):
            if k < 0:
                raise RenderError(A.RT_ERR_INVALID_ARG, f"object {o} produced no instance")
        lib, q = load_library(), 0
        while q < len(inst):
            e = q + 1
            while e < len(inst) and inst[e] == inst[e - 1] + 1:
                e += 1
            buf = (C.c_uint8 * (e - q))(*[1 if f else 0 for f in flags[q:e]])
            _check(lib.rt_scene_set_instances_visible(self._h, inst[q], e - q, buf))
            q = e

    def is_visible(self, object_index: int) -> bool:
        """Whether the instance of scene object `object_index` is visible, as of the last commit()."""
        k = self.instance_of(object_index) if self.dynamic else -1
        if k < 0:
            raise RenderError(A.RT_ERR_INVALID_ARG, f"object {object_index} produced no instance")
        v = C.c_int32(0)
        _check(load_library().rt_scene_instance_visible(self._h, k, C.byref(v)))
        return bool(v.value)

    def last_visibility_stats(self) -> A.rt_visibility_stats:
        """Instance and pair counts after the last commit(), what it showed and hid, whether it rebuilt
        the flattened instance tree on its own and whether that tree holds every visible pair
        (rt_scene_last_visibility_stats)."""
        st = A.rt_visibility_stats()
        _check(load_library().rt_scene_last_visibility_stats(self._h, C.byref(st)))
        return st

    def visible_scene(self) -> Scene:
        """A Scene holding only the objects whose instance is visible as of the last commit(), in
        scene order with their current transforms: the reference scene of the committed state
        (oracle.OracleScene(eng.visible_scene())); see visible_subset."""
        return visible_subset(self.scene, [self.instance_of(i) >= 0 and self.is_visible(i)
                                           for i in range(len(self.scene.objects))])

    # -- ray masks (rtcore.h "ray masks")
    def set_mask(self, object_index: int, mask: int):
        """Give the instance of scene object `object_index` the 32 mask bits `mask`
        (rt_scene_set_instance_masks): applied at once, no commit, on static scenes too.  A masked
        query's ray sees the instance iff the two masks share a bit and the instance is visible."""
        self.set_mask_many([object_index], [mask])

    def set_mask_many(self, object_indices, masks):
        """set_mask for several objects: `masks` is one value for all, or one per object.  Objects
        whose instances are consecutive go down in one rt_scene_set_instance_masks call."""
        objs = [int(o) for o in object_indices]
        vals = [int(masks)] * len(objs) if isinstance(masks, (int, np.integer)) else [int(m) for m in masks]
        if len(vals) != len(objs):
            raise ValueError("one mask per object")
        if any(m < 0 or m > 0xFFFFFFFF for m in vals):
            raise ValueError("a mask is 32 bits")
        inst = [self.instance_of(o) for o in objs]
        for o, k in zip(objs, inst):
            if k < 0:
                raise RenderError(A.RT_ERR_INVALID_ARG, f"object {o} produced no instance")
        lib, q = load_library(), 0
        while q < len(inst):
            e = q + 1
            while e < len(inst) and inst[e] == inst[e - 1] + 1:
                e += 1
            buf = (C.c_uint32 * (e - q))(*vals[q:e])
            _check(lib.rt_scene_set_instance_masks(self._h, inst[q], e - q, buf))
            q = e

    def mask_of(self, object_index: int) -> int:
        """The mask of the instance of scene object `object_index` (0xFFFFFFFF until it was set)."""
        k = self.instance_of(object_index)
        if k < 0:
            raise RenderError(A.RT_ERR_INVALID_ARG, f"object {object_index} produced no instance")
        m = C.c_uint32(0)
        _check(load_library().rt_scene_instance_mask(self._h, k, C.byref(m)))
        return int(m.value)

    def masked_scene(self, mask: int) -> Scene:
        """A Scene holding only the objects a ray with mask `mask` sees: those whose instance is
        visible as of the last commit() and whose mask shares a bit with `mask`, in scene order
        (visible_subset).  oracle.OracleScene(eng.masked_scene(m)) is the reference of a masked query."""
        keep = []
        for i in range(len(self.scene.objects)):
            k = self.instance_of(i)
            keep.append(k >= 0 and (not self.dynamic or self.is_visible(i)) and (self.mask_of(i) & int(mask)) != 0)
        return visible_subset(self.scene, keep)

    # -- deforming meshes (BVHBuilder.refit applied to a BLAS, BVH.swift:254-291)
    def vertex_count(self, object_index: int) -> int:
        """The vertex count of mesh object `object_index` (rt_scene_mesh_vertex_count)."""
        n = C.c_int64(0)
        _check(load_library().rt_scene_mesh_vertex_count(self._h, int(object_index), C.byref(n)))
        return int(n.value)

    def set_positions(self, object_index: int, positions, normals=None, mirror: bool = True):
        """Stage new vertex positions (and, for a mesh created with per-vertex normals, optionally
        new normals) for mesh object `object_index`; commit() applies them.  `positions` / `normals`
        are (N, 3) float64 numpy arrays, or contiguous float64 torch tensors on the scene's device,
        which are passed by pointer and must stay unchanged until commit() returns.  With `mirror`
        self.scene.objects[object_index] follows (a PLY-backed mesh becomes an inline mesh), so
        oracle.OracleScene(self.scene) stays the reference scene of the next committed state.
        The mirror follows when the positions are staged, as set_transform's does: a commit() that
        is refused (RT_ERR_INVALID_ARG) drops what was staged, and self.scene then describes a pose
        the engine never took - stage a valid pose again, or pass mirror=False and keep the mirror
        yourself, where a refusal is possible."""
        def unpack(a):
            if a is None:
                return None, None, False
            if hasattr(a, "data_ptr"):                       # a torch tensor
                if str(a.dtype) != "torch.float64" or not a.is_contiguous() or a.dim() != 2 or a.shape[1] != 3:
                    raise ValueError("a tensor must be a contiguous float64 (N, 3)")
                if a.device.type == "cpu":
                    return unpack(a.numpy())
                return a, np.asarray(a.detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3) if mirror else None, True
            h = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            if h.ndim != 2 or h.shape[1] != 3:
                raise ValueError("positions / normals are (N, 3) arrays")
            return h, h, False

        p, p_host, p_dev = unpack(positions)
        q, q_host, q_dev = unpack(normals)
        if p is None:
            raise ValueError("positions is None")
        if q is not None and q_dev != p_dev:
            raise ValueError("positions and normals must both be host arrays or both device tensors")
        count = int(p.shape[0]) if p.ndim == 2 else int(p.numel() // 3)
        if q is not None and (int(q.shape[0]) if q.ndim == 2 else int(q.numel() // 3)) != count:
            raise ValueError("normals must have one row per position")
        ptr = (lambda x: None if x is None else C.c_void_p(x.data_ptr() if p_dev else x.ctypes.data))
        _check(load_library().rt_scene_set_mesh_positions(self._h, int(object_index), ptr(p), count, ptr(q),
                                                          A.RT_POSITIONS_DEVICE if p_dev else 0))
        if not mirror:
            return
        o = self.scene.objects[object_index]
        if o.ply_path is not None:                           # the PLY's arrays, as the build read them
            m = ply_load(o.ply_path)
            o.indices = np.ascontiguousarray(m["indices"], dtype=np.int32).reshape(-1, 3)
            o.indices_one_based = False
            o.normals = m["normals"]
            o.ply_path = None
        o.positions = p_host.copy()
        if q_host is not None:
            o.normals = q_host.copy()

    def last_deform_stats(self) -> A.rt_deform_stats:
        """What the last commit() did for deformations (rt_scene_last_deform_stats)."""
        st = A.rt_deform_stats()
        _check(load_library().rt_scene_last_deform_stats(self._h, C.byref(st)))
        return st

    def instance_bounds(self, instance: int):
        """Instance.worldBounds of an instance: (lo[3], hi[3]) float64 arrays."""
        lo, hi = np.empty(3), np.empty(3)
        _check(load_library().rt_scene_instance_bounds(self._h, int(instance), lo.ctypes.data_as(A.c_double_p),
                                                       hi.ctypes.data_as(A.c_double_p)))
        return lo, hi

    # -- introspection (RayTracer.swift:52-67)
    def info(self) -> A.rt_scene_info:
        out = A.rt_scene_info()
        _check(load_library().rt_scene_info_get(self._h, C.byref(out)))
        return out

    def camera_spec(self, index: int) -> CameraSpec:
        c = self.scene.cameras[index]
        return CameraSpec(index, c.id, c.image_name, int(c.image_resolution[0]), int(c.image_resolution[1]))

    def inspect(self) -> SceneInfo:
        i = self.info()
        return SceneInfo([self.camera_spec(k) for k in range(len(self.scene.cameras))],
                         int(i.meshes), int(i.triangles), int(i.spheres), int(i.planes))

    # -- rendering
    def alloc_frame(self, camera_index: int = 0, chunk_first: int = 0, chunk_step: int = 1, rgba: bool = True):
        """Page-locked (rgb, rgba) output arrays for a chunk selection (rt_host_alloc): passed to
        render_rows as out/out_rgba, finished rows are DMA'd into them with no host copy."""
        cam = self.scene.cameras[camera_index]
        W, H = max(1, int(cam.image_resolution[0])), max(1, int(cam.image_resolution[1]))
        rows = load_library().rt_rows_for_chunks(H, chunk_first, chunk_step)
        rgb = pinned_array((rows, W, 3), np.float64)
        return rgb, (pinned_array((rows, W, 4), np.uint8) if rgba else None)

    def render_rows(self, camera_index: int = 0, chunk_first: int = 0, chunk_step: int = 1,
                    want_rgba: bool = True, progress: Optional[Callable[[RenderProgress], bool]] = None,
                    out: Optional[np.ndarray] = None, out_rgba: Optional[np.ndarray] = None):
        """Render the selected 8-row chunks; returns (rgb[rows,W,3] f64, rgba[rows,W,4] u8, RenderStats).
        `out` / `out_rgba`: optional reusable C-contiguous (rows, W, 3) float64 / (rows, W, 4) uint8
        arrays for the results (page-locked ones from alloc_frame take the direct-DMA path)."""
        lib = load_library()
        if not (0 <= camera_index < len(self.scene.cameras)):
            raise RenderError(A.RT_ERR_INVALID_CAMERA, "Invalid camera index")
        cam = self.scene.cameras[camera_index]
        W, H = max(1, int(cam.image_resolution[0])), max(1, int(cam.image_resolution[1]))
        rows = lib.rt_rows_for_chunks(H, chunk_first, chunk_step)
        if out is not None and out.shape == (rows, W, 3) and out.dtype == np.float64 and out.flags.c_contiguous:
            rgb = out
        else:
            rgb = np.empty((rows, W, 3), dtype=np.float64)
        if not want_rgba:
            rgba = None
        elif out_rgba is not None and out_rgba.shape == (rows, W, 4) and out_rgba.dtype == np.uint8 \
                and out_rgba.flags.c_contiguous:
            rgba = out_rgba
        else:
            rgba = np.empty((rows, W, 4), dtype=np.uint8)
        stats = self.render_into(camera_index, chunk_first, chunk_step, rgb, rgba, progress=progress)
        return rgb, rgba, stats

    def render_into(self, camera_index: int = 0, chunk_first: int = 0, chunk_step: int = 1,
                    rgb: Optional[np.ndarray] = None, rgba: Optional[np.ndarray] = None,
                    frame_layout: bool = False,
                    progress: Optional[Callable[[RenderProgress], bool]] = None) -> RenderStats:
        """rt_render_ex into caller-owned arrays (either may be None).  Shapes: the selected
        rows packed, (rows, W, 3|4); with frame_layout the whole frame (H, W, 3|4), the
        selected chunks' rows written at their image rows (RT_RENDER_FRAME_LAYOUT)."""
        lib = load_library()
        if not (0 <= camera_index < len(self.scene.cameras)):
            raise RenderError(A.RT_ERR_INVALID_CAMERA, "Invalid camera index")
        cam = self.scene.cameras[camera_index]
        W, H = max(1, int(cam.image_resolution[0])), max(1, int(cam.image_resolution[1]))
        rows = H if frame_layout else lib.rt_rows_for_chunks(H, chunk_first, chunk_step)
        for a, ch, dt in ((rgb, 3, np.float64), (rgba, 4, np.uint8)):
            if a is not None and (a.shape != (rows, W, ch) or a.dtype != dt or not a.flags.c_contiguous):
                raise ValueError(f"output array must be C-contiguous {dt.__name__}{(rows, W, ch)}, got "
                                 f"{a.dtype}{a.shape}")
        st = A.rt_stats()

        def _cb(user, done, total):
            if progress is None:
                return 1
            return 1 if progress(RenderProgress(done / max(total, 1), f"Row {done}/{total}")) else 0

        cb = A.RT_PROGRESS_FN(_cb) if progress is not None else A.RT_PROGRESS_FN()
        _check(lib.rt_render_ex(self._h, camera_index, chunk_first, chunk_step,
                                rgb.ctypes.data_as(A.c_double_p) if rgb is not None else None,
                                rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if rgba is not None else None,
                                A.RT_RENDER_FRAME_LAYOUT if frame_layout else 0, C.byref(st), cb, None))
        return _stats(st)

    def submit_into(self, camera_index: int = 0, chunk_first: int = 0, chunk_step: int = 1,
                    rgb: Optional[np.ndarray] = None, rgba: Optional[np.ndarray] = None,
                    frame_layout: bool = False, kernel_time: bool = False) -> int:
        """rt_render_submit: enqueue a render into page-locked arrays (pinned_array /
        register_host) and return its ticket at once; the arrays must stay alive until
        wait(ticket).  At most A.RT_MAX_IN_FLIGHT renders may be pending (RenderError -32).
        kernel_time: time the kernels with HIP events (RenderStats.kernel_ms, else 0)."""
        lib = load_library()
        if not (0 <= camera_index < len(self.scene.cameras)):
            raise RenderError(A.RT_ERR_INVALID_CAMERA, "Invalid camera index")
        cam = self.scene.cameras[camera_index]
        W, H = max(1, int(cam.image_resolution[0])), max(1, int(cam.image_resolution[1]))
        rows = H if frame_layout else lib.rt_rows_for_chunks(H, chunk_first, chunk_step)
        for a, ch, dt in ((rgb, 3, np.float64), (rgba, 4, np.uint8)):
            if a is not None and (a.shape != (rows, W, ch) or a.dtype != dt or not a.flags.c_contiguous):
                raise ValueError(f"output array must be C-contiguous {dt.__name__}{(rows, W, ch)}, got "
                                 f"{a.dtype}{a.shape}")
        t = C.c_int64(-1)
        _check(lib.rt_render_submit(self._h, camera_index, chunk_first, chunk_step,
                                    rgb.ctypes.data_as(A.c_double_p) if rgb is not None else None,
                                    rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if rgba is not None else None,
                                    (A.RT_RENDER_FRAME_LAYOUT if frame_layout else 0) |
                                    (A.RT_RENDER_KERNEL_TIME if kernel_time else 0), C.byref(t)))
        return int(t.value)

    def wait(self, ticket: int) -> RenderStats:
        """rt_render_wait: block until the submitted render is complete in its arrays."""
        st = A.rt_stats()
        _check(load_library().rt_render_wait(self._h, ticket, C.byref(st)))
        return _stats(st)

    def frame_pipeline(self, camera_index: int, chunk_first: int, chunk_step: int, rgbas, frame_layout: bool = True):
        """Frames rendered with len(rgbas) renders in flight (rt_render_submit / rt_render_wait),
        frame k into rgbas[k % len(rgbas)], arguments marshalled once.  Returns (submit, wait):
        submit(k) enqueues frame k and returns its ticket; wait(ticket) returns the raw rt_stats."""
        for a in rgbas:                                      # validates every buffer once
            self.wait(self.submit_into(camera_index, chunk_first, chunk_step, None, a, frame_layout))
        lib = load_library()
        h = self._h
        fs, fw = lib.rt_render_submit, lib.rt_render_wait
        ptrs = [a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in rgbas]
        flags = A.RT_RENDER_FRAME_LAYOUT if frame_layout else 0
        t = C.c_int64(-1)
        pt = C.byref(t)
        st = A.rt_stats()
        pst = C.byref(st)
        keep = list(rgbas)

        def submit(k: int) -> int:
            rc = fs(h, camera_index, chunk_first, chunk_step, None, ptrs[k % len(ptrs)], flags, pt)
            if rc != A.RT_OK:
                _check(rc)
            assert keep
            return t.value

        def wait(ticket: int) -> A.rt_stats:
            rc = fw(h, ticket, pst)
            if rc != A.RT_OK:
                _check(rc)
            return st
        return submit, wait

    def frame_renderer(self, camera_index: int = 0, chunk_first: int = 0, chunk_step: int = 1,
                       rgb: Optional[np.ndarray] = None, rgba: Optional[np.ndarray] = None,
                       frame_layout: bool = False) -> Callable[[], A.rt_stats]:
        """render_into with the arguments checked and marshalled once: returns a callable that
        renders one frame into the same arrays (one rt_render_ex call, no progress callback)
        and returns the raw rt_stats.  For frame loops whose per-call Python cost should not
        count as render time (bench.py)."""
        self.render_into(camera_index, chunk_first, chunk_step, rgb, rgba, frame_layout)   # validates
        lib = load_library()
        fn = lib.rt_render_ex
        h = self._h
        prgb = rgb.ctypes.data_as(A.c_double_p) if rgb is not None else None
        prgba = rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if rgba is not None else None
        flags = A.RT_RENDER_FRAME_LAYOUT if frame_layout else 0
        st = A.rt_stats()
        pst = C.byref(st)
        cb = A.RT_PROGRESS_FN()
        keep = (rgb, rgba)

        def one() -> A.rt_stats:
            rc = fn(h, camera_index, chunk_first, chunk_step, prgb, prgba, flags, pst, cb, None)
            if rc != A.RT_OK:
                _check(rc)
            assert keep is not None
            return st
        return one

    def render(self, camera_index: int = 0, progress: Optional[Callable[[RenderProgress], bool]] = None) -> RenderResult:
        """RayTracerEngine.render(format:cameraIndex:progress:) (RayTracer.swift:115-131)."""
        rgb, rgba, stats = self.render_rows(camera_index, 0, 1, True, progress)
        spec = self.camera_spec(camera_index)
        return RenderResult(self.scene.cameras[camera_index].image_name, rgba, rgb, spec, stats)

    def save_png(self, path: str, camera_index: int = 0,
                 progress: Optional[Callable[[RenderProgress], bool]] = None) -> RenderResult:
        """renderCGImage + ImageHelper.savePNG (RayTracer.swift:105-112, Helpers/Image.swift:14-42)."""
        from . import sceneio
        res = self.render(camera_index, progress)
        sceneio.save_png(res.rgba8, path)
        return res

    def render_all(self, progress: Optional[Callable[[RenderProgress], bool]] = None) -> List[RenderResult]:
        """renderAll (RayTracer.swift:70-102)."""
        return [self.render(k, progress) for k in range(len(self.scene.cameras))]

    # -- device-resident path (bench / multi-GPU ranks)
    def render_device(self, out_rgb_ptr: int, camera_index: int = 0, chunk_first: int = 0, chunk_step: int = 1,
                      slot: int = 0, stream: int = 0, out_rgba_ptr: int = 0):
        """Enqueue a render into device buffers on `stream` (no host sync)."""
        _check(load_library().rt_render_device(self._h, slot, camera_index, chunk_first, chunk_step,
                                               C.c_void_p(out_rgb_ptr), C.c_void_p(out_rgba_ptr or None),
                                               C.c_void_p(stream or None)))

    def collect_stats(self, slot: int = 0) -> A.rt_stats:
        st = A.rt_stats()
        _check(load_library().rt_stats_collect(self._h, slot, C.byref(st)))
        return st

    def work_counters(self, out_rgb_ptr: int, camera_index: int = 0, chunk_first: int = 0, chunk_step: int = 1,
                      slot: int = 0, stream: int = 0) -> A.rt_work_counters:
        wc = A.rt_work_counters()
        _check(load_library().rt_render_device_counted(self._h, slot, camera_index, chunk_first, chunk_step,
                                                       C.c_void_p(out_rgb_ptr), C.c_void_p(stream or None),
                                                       C.byref(wc)))
        return wc

    def trace_rays(self, origins, dirs, tmin=None, time=None, slot: int = 0):
        """Closest hits of explicit rays through the render kernels' traversal
        (rt_debug_trace_rays, a thin caller of the ray-query path: query_closest on host arrays):
        returns t (+inf = miss), world point, world normal, material."""
        o, d, n, tl, tm = _ray_arrays(origins, dirs, tmin, time)
        t = np.empty(n); p = np.empty((n, 3)); nn = np.empty((n, 3)); mat = np.empty(n, np.int32)
        _check(load_library().rt_debug_trace_rays(
            self._h, slot, n, o.ctypes.data_as(A.c_double_p), d.ctypes.data_as(A.c_double_p),
            tl.ctypes.data_as(A.c_double_p), tm.ctypes.data_as(A.c_double_p), t.ctypes.data_as(A.c_double_p),
            p.ctypes.data_as(A.c_double_p), nn.ctypes.data_as(A.c_double_p), mat.ctypes.data_as(A.c_int32_p)))
        return t, p, nn, mat

    def occluded_rays(self, origins, dirs, tmax, time=None, slot: int = 0):
        """Any-hit of explicit segments (rt_debug_occluded_rays, a thin caller of the ray-query
        path: query_occluded on host arrays): bool per ray."""
        o, d, n, tl, tm = _ray_arrays(origins, dirs, tmax, time)
        out = np.empty(n, np.uint8)
        _check(load_library().rt_debug_occluded_rays(
            self._h, slot, n, o.ctypes.data_as(A.c_double_p), d.ctypes.data_as(A.c_double_p),
            tl.ctypes.data_as(A.c_double_p), tm.ctypes.data_as(A.c_double_p), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.astype(bool)

    # -- ray queries (rt_query_closest / rt_query_occluded)
    def query_closest(self, origins, dirs, tmin=None, time=None, *, slot: int = 0, want=("t", "uv", "ids"),
                      bounds=None, mask=None) -> "RayHits":
        """Closest hits of caller-given rays through the scene's production walks (rt_query_closest).
        `origins` / `dirs` are (N, 3) float64: numpy arrays in give numpy arrays out; contiguous
        float64 torch tensors on the slot's device are used in place, the work is enqueued on
        torch.cuda.current_stream() and torch tensors come back (with `bounds` given nothing
        synchronises).  `tmin` / `time` are per-ray arrays of the same kind, or None (0).
        `want` names the RayHits fields to fill: t, uv, ids, point, normal, flags.
        `bounds` = (origin_reach, origin_coord, dir_norm) declares the batch's maxima (rays beyond
        them come back flagged RT_HIT_OUT_OF_BOUNDS, untraced); None lets the device find them.
        `mask`: None is the unmasked query (instance masks are ignored); an int gives every ray
        that mask; a uint32 numpy array - with device rays a torch int32 / uint32 tensor on their
        device, whose bits are the masks - gives ray i mask[i] (rt_query_closest_masked, set_mask)."""
        unknown = set(want) - set(RayHits.FIELDS)
        if unknown:
            raise ValueError(f"unknown RayHits fields {sorted(unknown)}")
        # `keep` holds the arrays the batch points into (converted copies among them) until the call returns
        rays, n, on_dev, keep, alloc = _query_rays(origins, dirs, tmin, time)
        hits = RayHits()
        hb = A.rt_hit_batch()
        for name, (cols, dt) in RayHits.FIELDS.items():
            if name in want:
                a = alloc((n, cols) if cols > 1 else (n,), dt)
                setattr(hits, name, a)
                setattr(hb, name, _ptr(a))
        if mask is None:
            _check(load_library().rt_query_closest(self._h, int(slot), n, C.byref(rays), C.byref(hb), _bounds(bounds),
                                                   A.RT_QUERY_DEVICE if on_dev else 0, _stream(on_dev)))
        else:
            rm, keep_mask = _ray_masks(mask, n, on_dev, origins)
            _check(load_library().rt_query_closest_masked(self._h, int(slot), n, C.byref(rays), C.byref(hb),
                                                          _bounds(bounds), A.RT_QUERY_DEVICE if on_dev else 0,
                                                          _stream(on_dev), C.byref(rm)))
        return hits

    def query_occluded(self, origins, dirs, tmax=None, time=None, *, slot: int = 0, bounds=None, mask=None):
        """Any hit of caller-given segments (rt_query_occluded): per ray 0 = free, 1 = blocked, 2 = not
        traced (beyond the declared `bounds`, or non-finite), as a uint8 numpy array or torch tensor;
        arguments as query_closest (`tmax` None = +inf; `mask`: rt_query_occluded_masked)."""
        rays, n, on_dev, keep, alloc = _query_rays(origins, dirs, tmax, time)    # keep: as in query_closest
        out = alloc((n,), np.uint8)
        if mask is None:
            _check(load_library().rt_query_occluded(self._h, int(slot), n, C.byref(rays), C.c_void_p(_ptr(out)),
                                                    _bounds(bounds), A.RT_QUERY_DEVICE if on_dev else 0, _stream(on_dev)))
        else:
            rm, keep_mask = _ray_masks(mask, n, on_dev, origins)
            _check(load_library().rt_query_occluded_masked(self._h, int(slot), n, C.byref(rays), C.c_void_p(_ptr(out)),
                                                           _bounds(bounds), A.RT_QUERY_DEVICE if on_dev else 0,
                                                           _stream(on_dev), C.byref(rm)))
        return out

    def last_query_stats(self, slot: int = 0) -> A.rt_query_counts:
        """Counts of the last query on `slot` (rt_query_stats); valid once its stream has drained."""
        st = A.rt_query_counts()
        _check(load_library().rt_query_stats(self._h, int(slot), C.byref(st)))
        return st

    # -- first-hit buffers (rt_render_gbuffer)
    def first_hits(self, camera_index: int = 0, chunk_first: int = 0, chunk_step: int = 1, *,
                   want=("rays", "t", "ids"), centre: bool = False, frame_layout: bool = False, slot: int = 0,
                   out=None) -> "FirstHits":
        """Per pixel of the selected 8-row chunks, the first primary ray the render casts through it
        and what that ray hits (rt_render_gbuffer): a FirstHits whose `origins`, `dirs`, `tmin`, `time`
        are shaped (rows, W[, 3]) and whose `hits` is a RayHits shaped (rows, W[, cols]), exactly what
        query_closest returns for those rays.  `want` names what to fill: "rays" (all four ray arrays)
        or any of origins, dirs, tmin, time, and the RayHits fields t, uv, ids, point, normal, flags;
        the rest is None.  `centre`: the deterministic ray through each pixel's centre (no lens, time 0)
        instead of the render's jittered one.  Rows are packed in chunk order (rows_for_chunks rows), or
        with `frame_layout` every array is a whole H x W frame whose unselected rows are not written.
        numpy arrays come back by default.  `out` = a dict, keyed as `want`, of contiguous float64 /
        int32 / uint8 torch tensors on the slot's device: they are written in place, enqueued on
        torch.cuda.current_stream() with no synchronisation, and `want` is ignored."""
        return self._first_hits(None, camera_index, chunk_first, chunk_step, want, centre, frame_layout, slot, out)

    def first_hits_masked(self, mask: int, camera_index: int = 0, chunk_first: int = 0, chunk_step: int = 1, *,
                          want=("rays", "t", "ids"), centre: bool = False, frame_layout: bool = False, slot: int = 0,
                          out=None) -> "FirstHits":
        """first_hits with one ray mask for the whole call (rt_render_gbuffer_masked): a camera layer,
        picking against selectable objects.  The record is query_closest(exported rays, mask=mask)'s."""
        if not 0 <= int(mask) <= 0xFFFFFFFF:
            raise ValueError("a mask is 32 bits")
        return self._first_hits(int(mask), camera_index, chunk_first, chunk_step, want, centre, frame_layout, slot, out)

    def _first_hits(self, mask, camera_index, chunk_first, chunk_step, want, centre, frame_layout, slot, out):
        cam = self.scene.cameras[camera_index] if 0 <= camera_index < len(self.scene.cameras) else None
        W, H = (max(1, int(cam.image_resolution[0])), max(1, int(cam.image_resolution[1]))) if cam else (0, 0)
        rows = H if frame_layout else rows_for_chunks(H, chunk_first, chunk_step)
        fields = dict(FirstHits.RAYS, **RayHits.FIELDS)
        names = list(out) if out is not None else [f for w in want for f in (FirstHits.RAYS if w == "rays" else (w,))]
        unknown = set(names) - set(fields)
        if unknown:
            raise ValueError(f"unknown FirstHits fields {sorted(unknown)}")
        on_dev = out is not None
        res, gb = FirstHits(hits=RayHits(), rows=rows, width=W), A.rt_gbuffer()
        for name in names:
            cols, dt = fields[name]
            shape = (rows, W, cols) if cols > 1 else (rows, W)
            if on_dev:
                import torch
                a = out[name]
                tdt = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}[dt]
                if not isinstance(a, torch.Tensor) or not a.is_cuda or a.dtype != tdt or not a.is_contiguous() or \
                        a.numel() != rows * W * cols:
                    raise ValueError(f"{name}: a contiguous {tdt} tensor of {shape} on the slot's device")
            else:
                a = np.empty(shape, dt)
            ray = name in FirstHits.RAYS
            setattr(res if ray else res.hits, name, a)
            setattr(gb if ray else gb.hits, FirstHits.ABI.get(name, name), _ptr(a))
        flags = (A.RT_GBUFFER_DEVICE if on_dev else 0) | (A.RT_GBUFFER_PIXEL_CENTRE if centre else 0) | \
                (A.RT_GBUFFER_FRAME_LAYOUT if frame_layout else 0)
        if mask is None:
            _check(load_library().rt_render_gbuffer(self._h, int(slot), int(camera_index), int(chunk_first),
                                                    int(chunk_step), C.byref(gb), flags, _stream(on_dev)))
        else:
            _check(load_library().rt_render_gbuffer_masked(self._h, int(slot), int(camera_index), int(chunk_first),
                                                           int(chunk_step), C.byref(gb), flags, _stream(on_dev), mask))
        return res

    def bvh_hash(self, instance: int) -> int:
        return int(load_library().rt_debug_bvh_hash(self._h, instance))

    def wide_read(self, slot: int = 0) -> dict:
        """The four-wide trees of replica `slot`, copied back from the device (rt_debug_wide_read);
        the dict of wide_build()."""
        lib = load_library()
        return _wide_dump(lambda io: lib.rt_debug_wide_read(self._h, int(slot), C.byref(io)))


def visible_subset(scene: Scene, keep) -> Scene:
    """A shallow copy of `scene` holding only the objects whose `keep` flag is set, in scene order.
    A MeshInstance kept while its base mesh is not is written as a Mesh of its own, with the base's
    triangles, shading and triangle motion blur and the instance's id, matrix and material (a Mesh
    has no instance motion: a MeshInstance's motion_blur is not carried over)."""
    import copy
    from .scene import Mesh, MeshInstance
    keep = [bool(k) for k in keep]
    if len(keep) != len(scene.objects):
        raise ValueError("one flag per object")
    kept_mesh = {o.id for o, k in zip(scene.objects, keep) if k and isinstance(o, Mesh)}
    base = {o.id: o for o in scene.objects if isinstance(o, Mesh)}
    objs = []
    for o, k in zip(scene.objects, keep):
        if not k:
            continue
        if isinstance(o, MeshInstance) and o.base_mesh_id not in kept_mesh and o.base_mesh_id in base:
            b = base[o.base_mesh_id]
            m = copy.copy(b)
            m.id = o.id
            m.material = o.material if o.material not in (None, "") else b.material
            m.transform = o.transform
            objs.append(m)
        else:
            objs.append(o)
    out = copy.copy(scene)
    out.objects = objs
    return out


_WIDE_SCALARS = ("wnodes", "wide_copy", "tris", "pairs", "instances", "tw_tlas_nodes", "fit_nodes", "marker_base",
                 "tlas_leaf_base", "wide_root", "fit_root", "identity", "fit_blocked", "wide_coord", "fit_coord")


def _wide_dump(call) -> dict:
    """Two calls of an rt_wide_dump hook: the counts, then the buffers sized from them.  Returns
    the scalars under their rtcore.h names and the arrays: nodes (wnodes, 32) uint32 raw words of
    the 128-byte records, lbox (tris, 6), fpairs (pairs, 2), l2w (instances, 16), tbox
    (instances, 6), wroot, bcoord, inst_bounds (instances, 6), tri_prim, tri_last."""
    io = A.rt_wide_dump()
    _check(call(io))
    nn, nt, npair, ni = int(io.wnodes), int(io.tris), int(io.pairs), int(io.instances)
    arr = {"nodes": np.zeros((nn, 32), np.uint32), "lbox": np.zeros((nt, 6)), "fpairs": np.zeros((npair, 2), np.int32),
           "l2w": np.zeros((ni, 16)), "tbox": np.zeros((ni, 6)), "wroot": np.zeros(ni, np.int32),
           "bcoord": np.zeros(ni), "inst_bounds": np.zeros((ni, 6)), "tri_prim": np.zeros(nt, np.int32),
           "tri_last": np.zeros(nt, np.uint8)}
    io.cap_wnodes, io.cap_tris, io.cap_pairs, io.cap_instances = nn, nt, npair, ni
    for name, a in arr.items():
        if a.size:
            setattr(io, name, a.ctypes.data_as(dict(A.rt_wide_dump._fields_)[name]))
    _check(call(io))
    assert (int(io.wnodes), int(io.tris), int(io.pairs), int(io.instances)) == (nn, nt, npair, ni)
    out = {k: getattr(io, k) for k in _WIDE_SCALARS}
    out.update(arr)
    return out


def wide_build(scene: Scene, dynamic: bool = False) -> dict:
    """The four-wide trees of a host-only build (rt_debug_wide_build; no device is touched)."""
    lib = load_library()
    pk = scene.to_desc()
    return _wide_dump(lambda io: lib.rt_debug_wide_build(pk.ptr, A.RT_SCENE_DYNAMIC if dynamic else 0, C.byref(io)))


def _stats(st: A.rt_stats) -> RenderStats:
    return RenderStats(int(st.meshes), int(st.triangles), int(st.spheres), int(st.planes),
                       int(st.primary_rays + st.shadow_rays), int(st.primary_rays), int(st.shadow_rays),
                       int(st.secondary_rays), float(st.milliseconds), float(st.kernel_ms),
                       int(st.shadow_rays_traced), int(st.rewalked))


def register_host(arr: np.ndarray):
    """Page-lock an existing host array (rt_host_register; e.g. a framebuffer in shared memory
    that several processes fill).  Call unregister_host(arr) before the memory goes away."""
    _check(load_library().rt_host_register(C.c_void_p(arr.ctypes.data), arr.nbytes))


def unregister_host(arr: np.ndarray):
    _check(load_library().rt_host_unregister(C.c_void_p(arr.ctypes.data)))


@dataclass
class RayHits:
    """What query_closest returns: the fields named in `want`, the others None.  t: +inf on a miss;
    uv: Moeller-Trumbore u, v; ids: (object, face within that object, instance, material), -1 on a
    miss; point / normal: world hit point and geometric normal; flags: RT_HIT_* bits."""
    t: object = None
    uv: object = None
    ids: object = None
    point: object = None
    normal: object = None
    flags: object = None
    FIELDS = {"t": (1, np.float64), "uv": (2, np.float64), "ids": (4, np.int32), "point": (3, np.float64),
              "normal": (3, np.float64), "flags": (1, np.uint8)}


@dataclass
class FirstHits:
    """What first_hits returns: per pixel the first primary ray of the render (origins, dirs (rows, W,
    3); tmin, time (rows, W)) and its record (`hits`, a RayHits of the same leading shape); the
    fields that were not asked for are None."""
    origins: object = None
    dirs: object = None
    tmin: object = None
    time: object = None
    hits: "RayHits" = None
    rows: int = 0
    width: int = 0
    RAYS = {"origins": (3, np.float64), "dirs": (3, np.float64), "tmin": (1, np.float64), "time": (1, np.float64)}
    ABI = {"origins": "origin", "dirs": "dir"}            # rt_gbuffer's member names


def _ptr(a):
    return None if a is None else int(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def _bounds(b):
    return None if b is None else C.byref(A.rt_query_bounds(float(b[0]), float(b[1]), float(b[2])))


def _stream(on_dev: bool):
    if not on_dev:
        return None
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream or None)


def _query_rays(origins, dirs, tlim, time):
    """rt_ray_batch over the caller's arrays: (batch, n, device?, the arrays it points into, an
    allocator of outputs of the same kind)."""
    on_dev = hasattr(origins, "data_ptr") and origins.device.type != "cpu"
    rays = A.rt_ray_batch()
    if on_dev:
        import torch
        n = int(origins.shape[0])
        for name, a, cols in (("origins", origins, 3), ("dirs", dirs, 3), ("tlimit", tlim, 1), ("time", time, 1)):
            if a is None and cols == 1:
                continue
            if not isinstance(a, torch.Tensor) or a.device != origins.device or a.dtype != torch.float64 or \
                    not a.is_contiguous() or a.numel() != n * cols:
                raise ValueError(f"{name}: a contiguous float64 tensor of {n} x {cols} on {origins.device}")
        keep = (origins, dirs, tlim, time)
        dt = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}

        def alloc(shape, dtype):
            return torch.empty(shape, dtype=dt[dtype], device=origins.device)
    else:
        as_np = (lambda a: a.numpy() if hasattr(a, "data_ptr") else a)
        o = np.ascontiguousarray(as_np(origins), dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(as_np(dirs), dtype=np.float64).reshape(-1, 3)
        n = o.shape[0]
        if d.shape[0] != n:
            raise ValueError("origins and dirs differ in length")
        per_ray = (lambda a: None if a is None else
                   np.ascontiguousarray(np.broadcast_to(as_np(a), (n,)), dtype=np.float64))
        keep = (o, d, per_ray(tlim), per_ray(time))

        def alloc(shape, dtype):
            return np.empty(shape, dtype)
    rays.origin, rays.dir, rays.tlimit, rays.time = (_ptr(a) for a in keep)
    return rays, n, on_dev, keep, alloc


def _ray_masks(mask, n: int, on_dev: bool, origins):
    """rt_ray_masks for a query of n rays: (the struct, the array it points into)."""
    rm = A.rt_ray_masks()
    if isinstance(mask, (int, np.integer)):
        if not 0 <= int(mask) <= 0xFFFFFFFF:
            raise ValueError("a mask is 32 bits")
        rm.per_ray, rm.all = None, int(mask)
        return rm, None
    if on_dev:
        import torch
        ok = (torch.int32, getattr(torch, "uint32", torch.int32))
        if not isinstance(mask, torch.Tensor) or mask.device != origins.device or mask.dtype not in ok or \
                not mask.is_contiguous() or mask.numel() != n:
            raise ValueError(f"mask: an int, or a contiguous int32 / uint32 tensor of {n} on {origins.device}")
        keep = mask
    else:
        keep = np.ascontiguousarray(mask.numpy() if hasattr(mask, "data_ptr") else mask)
        if keep.dtype == np.int32:
            keep = keep.view(np.uint32)
        if keep.dtype != np.uint32 or keep.size != n:
            raise ValueError(f"mask: an int, or a uint32 array of {n}")
    rm.per_ray, rm.all = _ptr(keep), 0
    return rm, keep


def query_tables(scene: Scene, flags: int = 0) -> dict:
    """The face table of a host-only build (rt_debug_query_tables; no device is touched): face and
    tri_object per triangle record, verts (tris, 9) = v0, e1, e2, inst_object per instance."""
    lib = load_library()
    pk = scene.to_desc()
    io = A.rt_query_tables()
    _check(lib.rt_debug_query_tables(pk.ptr, flags, C.byref(io)))
    nt, ni = int(io.tris), int(io.instances)
    out = {"face": np.zeros(nt, np.int32), "tri_object": np.zeros(nt, np.int32), "verts": np.zeros((nt, 9)),
           "inst_object": np.zeros(ni, np.int32)}
    for name, a in out.items():
        setattr(io, name, a.ctypes.data_as(dict(A.rt_query_tables._fields_)[name]))
    _check(lib.rt_debug_query_tables(pk.ptr, flags, C.byref(io)))
    return out


def _ray_arrays(origins, dirs, tlim, time):
    o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    n = o.shape[0]
    if d.shape[0] != n:
        raise ValueError("origins and dirs differ in length")
    tl = np.zeros(n) if tlim is None else np.ascontiguousarray(np.broadcast_to(tlim, (n,)), dtype=np.float64)
    tm = np.zeros(n) if time is None else np.ascontiguousarray(np.broadcast_to(time, (n,)), dtype=np.float64)
    return o, d, n, tl, tm


def pinned_array(shape, dtype) -> np.ndarray:
    """numpy array over page-locked host memory (rt_host_alloc); freed with the array."""
    import weakref
    lib = load_library()
    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dt.itemsize
    if nbytes == 0:
        return np.empty(shape, dt)
    p = C.c_void_p()
    _check(lib.rt_host_alloc(nbytes, C.byref(p)))
    buf = (C.c_uint8 * nbytes).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dt).reshape(shape)
    weakref.finalize(buf, lib.rt_host_free, C.c_void_p(p.value))
    return arr


def rows_for_chunks(height: int, chunk_first: int, chunk_step: int) -> int:
    """Pure-Python restatement of rt_rows_for_chunks (used by host-side sharding logic)."""
    height = max(1, height)
    n = (height + 7) // 8
    return sum(min(8, height - 8 * c) for c in range(chunk_first, n, chunk_step)) if chunk_step >= 1 else 0


def ply_load(path: str):
    """PLYLoader.load (PLYReader.swift:54-210) through the product's C ABI.
    Returns dict(positions (V,3) f64, normals (V,3) f64 | None, texcoords (V,2) f32 | None, indices (T,3) i32)."""
    lib = load_library()
    m = A.rt_ply_mesh()
    _check(lib.rt_ply_load(path.encode(), C.byref(m)))
    try:
        pos = np.ctypeslib.as_array(m.positions, shape=(m.num_positions * 3,)).reshape(-1, 3).copy() \
            if m.num_positions else np.zeros((0, 3))
        nrm = np.ctypeslib.as_array(m.normals, shape=(m.num_normals * 3,)).reshape(-1, 3).copy() \
            if m.num_normals else None
        uv = np.ctypeslib.as_array(m.texcoords, shape=(m.num_texcoords * 2,)).reshape(-1, 2).copy() \
            if m.num_texcoords else None
        idx = np.ctypeslib.as_array(m.indices, shape=(m.num_indices,)).copy() if m.num_indices else \
            np.zeros((0,), np.int32)
    finally:
        lib.rt_ply_free(C.byref(m))
    return {"positions": pos, "normals": nrm, "texcoords": uv, "indices": idx.reshape(-1, 3) if idx.size % 3 == 0 else idx}
