"""Ray masks, the interface: rtcore.h declares rt_scene_set_instance_masks, rt_scene_instance_mask,
rt_ray_masks, rt_query_closest_masked, rt_query_occluded_masked and rt_render_gbuffer_masked; the ctypes
mirror and the library agree; RT_ABI_VERSION stays 5 (the entry points are appended and detected by
symbol) and the lists earlier ABI tests pin stay; the Python engine and rt_engine.hpp carry the methods;
RayTracerEngine.masked_scene selects the objects a masked ray sees.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import myraytracer_amd as M
from myraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtcore.h")
FUNCS = ("rt_scene_set_instance_masks", "rt_scene_instance_mask", "rt_query_closest_masked",
         "rt_query_occluded_masked", "rt_render_gbuffer_masked")
FIELDS = ["per_ray", "all", "pad"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _args(src, name):
    """The parameter list of function `name` in the header, comments and newlines removed."""
    return re.sub(r"\s+", " ", re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1)).strip()


def test_header_declares_the_interface():
    src = _code()
    assert re.search(r"typedef struct rt_ray_masks\s*\{", src)
    for f in FUNCS:
        assert re.search(rf"\bint32_t\s+{f}\s*\(", src), f
    assert re.search(r"rt_scene_set_instance_masks\s*\(\s*rt_scene\s*\*[^,]*,\s*int32_t[^,]*,\s*int32_t[^,]*,"
                     r"\s*const uint32_t\s*\*", src)
    assert re.search(r"rt_scene_instance_mask\s*\(\s*const rt_scene\s*\*[^,]*,\s*int32_t[^,]*,\s*uint32_t\s*\*", src)
    # the masked entry points take their unmasked counterpart's arguments, then the masks
    for plain, masked, last in (("rt_query_closest", "rt_query_closest_masked", r"const rt_ray_masks\s*\*\s*\w+"),
                                ("rt_query_occluded", "rt_query_occluded_masked", r"const rt_ray_masks\s*\*\s*\w+"),
                                ("rt_render_gbuffer", "rt_render_gbuffer_masked", r"uint32_t\s+\w+")):
        a, b = _args(src, plain), _args(src, masked)
        assert b.startswith(a + ", "), (plain, a, b)
        assert re.fullmatch(last, b[len(a) + 2:]), (masked, b)
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", src).group(1)) == 5
    # what the header, DESIGN.md and INTEGRATION.md used to rule out is now said to exist; masks in
    # renders stay out of scope and the header says so
    for path in (HEADER, os.path.join(ROOT, "DESIGN.md"), os.path.join(ROOT, "INTEGRATION.md")):
        text = re.sub(r"[\s*]+", " ", open(path).read())
        assert "per-ray or per-render masks" not in text, path
    head = re.sub(r"[\s*]+", " ", open(HEADER).read())
    assert "ray masks" in head and "masks in renders" in head


def test_mirror_matches_the_header(tmp_path):
    assert A.RT_ABI_VERSION == 5
    assert A.MASK_SYMBOLS == list(FUNCS) and set(FUNCS) <= set(A.EXPORTED_SYMBOLS)
    assert A.QUERY_SYMBOLS == ["rt_query_closest", "rt_query_occluded", "rt_query_stats", "rt_debug_query_tables"]
    assert A.GBUFFER_SYMBOLS == ["rt_render_gbuffer"]
    assert len(set(A.EXPORTED_SYMBOLS)) == len(A.EXPORTED_SYMBOLS)
    assert [f for f, _ in A.rt_ray_masks._fields_] == FIELDS
    prog = tmp_path / "sizes.c"
    body = ('printf("%zu\\n", sizeof(rt_ray_masks));printf("%zu\\n", sizeof(rt_query_counts));'
            'printf("%zu\\n", sizeof(rt_gbuffer));' +
            "".join(f'printf("%zu\\n", offsetof(rt_ray_masks, {f}));' for f in FIELDS))
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(A.rt_ray_masks) == 16
    assert got[1] == C.sizeof(A.rt_query_counts) == 72              # keeps its layout
    assert got[2] == C.sizeof(A.rt_gbuffer)
    for k, f in enumerate(FIELDS):
        assert got[3 + k] == getattr(A.rt_ray_masks, f).offset, f


def test_library_exports_and_refuses_without_a_scene():
    lib = M.load_library()
    assert lib.rt_version().endswith(b"(abi 5, gfx950, fp64)")
    for f in FUNCS:
        assert hasattr(lib, f), f
    for f in FUNCS:                                                    # bind() gave each its prototype
        assert getattr(lib, f).restype is C.c_int32 and getattr(lib, f).argtypes, f
    P = C.POINTER
    assert lib.rt_scene_set_instance_masks.argtypes == [C.c_void_p, C.c_int32, C.c_int32, P(C.c_uint32)]
    assert lib.rt_scene_instance_mask.argtypes == [C.c_void_p, C.c_int32, P(C.c_uint32)]
    assert lib.rt_query_closest_masked.argtypes == lib.rt_query_closest.argtypes + [P(A.rt_ray_masks)]
    assert lib.rt_query_occluded_masked.argtypes == lib.rt_query_occluded.argtypes + [P(A.rt_ray_masks)]
    assert lib.rt_render_gbuffer_masked.argtypes == lib.rt_render_gbuffer.argtypes + [C.c_uint32]
    masks = (C.c_uint32 * 2)(1, 2)
    m = C.c_uint32(7)
    rm = A.rt_ray_masks(None, 3, 0)
    rays, hits, gb = A.rt_ray_batch(), A.rt_hit_batch(), A.rt_gbuffer()
    out = (C.c_uint8 * 1)(9)
    assert lib.rt_scene_set_instance_masks(None, 0, 2, masks) == A.RT_ERR_NO_SCENE
    assert b"scene" in lib.rt_last_error().lower()
    assert lib.rt_scene_instance_mask(None, 0, C.byref(m)) == A.RT_ERR_NO_SCENE and m.value == 7
    assert lib.rt_query_closest_masked(None, 0, 1, C.byref(rays), C.byref(hits), None, 0, None,
                                       C.byref(rm)) == A.RT_ERR_NO_SCENE
    assert lib.rt_query_occluded_masked(None, 0, 1, C.byref(rays), out, None, 0, None, C.byref(rm)) == A.RT_ERR_NO_SCENE
    assert lib.rt_query_occluded_masked(None, 0, 1, C.byref(rays), out, None, 0, None, None) == A.RT_ERR_NO_SCENE
    assert out[0] == 9
    assert lib.rt_render_gbuffer_masked(None, 0, 0, 0, 1, C.byref(gb), 0, None, 1) == A.RT_ERR_NO_SCENE


def test_the_python_engine_carries_the_interface():
    E = M.RayTracerEngine
    for name in ("set_mask", "set_mask_many", "mask_of", "masked_scene", "first_hits_masked"):
        assert callable(getattr(E, name)), name
    assert list(inspect.signature(E.set_mask).parameters) == ["self", "object_index", "mask"]
    assert list(inspect.signature(E.set_mask_many).parameters) == ["self", "object_indices", "masks"]
    assert list(inspect.signature(E.mask_of).parameters) == ["self", "object_index"]
    assert list(inspect.signature(E.masked_scene).parameters) == ["self", "mask"]
    for q in (E.query_closest, E.query_occluded):                      # `mask` is keyword-only, None by default
        p = inspect.signature(q).parameters["mask"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    # first_hits_masked is first_hits with the mask in front; first_hits keeps its own list
    plain = inspect.signature(E.first_hits).parameters
    masked = inspect.signature(E.first_hits_masked).parameters
    assert list(masked) == ["self", "mask"] + list(plain)[1:]
    for name in list(plain)[1:]:
        assert (masked[name].kind, masked[name].default) == (plain[name].kind, plain[name].default), name


class _Stub(M.RayTracerEngine):
    """masked_scene over a scene, visibility flags and masks held here: no device, no library."""

    def __init__(self, scene, inst, visible, masks, dynamic=True):
        self.scene, self.dynamic, self._h = scene, dynamic, None
        self._inst, self._vis, self._masks = inst, visible, masks

    def instance_of(self, i):
        return self._inst[i]

    def is_visible(self, i):
        return self._vis[i]

    def mask_of(self, i):
        return self._masks[i]


def test_masked_scene_selects_the_visible_objects_that_share_a_bit():
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    base = M.Mesh(id=1, material="2", positions=pos, indices=np.array([[0, 1, 2]], np.int32), indices_one_based=False)
    inst = M.MeshInstance(id=5, base_mesh_id=1, transform=M.translation(1.0, 2.0, 3.0))
    sph, pln = M.Sphere((0.0, 0.0, 0.0), 1.0), M.Plane(center=(0.0, -1.0, 0.0), normal=(0.0, 1.0, 0.0))
    sc = M.Scene(cameras=[], materials=[], objects=[base, inst, sph, pln])
    eng = _Stub(sc, inst=[1, 0, 2, 3], visible=[True, True, False, True], masks=[0b0001, 0b0110, 0xFFFFFFFF, 0x80000000])
    ids = lambda s: [o.id if isinstance(o, (M.Mesh, M.MeshInstance)) else type(o).__name__ for o in s.objects]   # noqa: E731
    assert ids(eng.masked_scene(0xFFFFFFFF)) == [1, 5, "Plane"]          # the hidden sphere never shows
    assert ids(eng.masked_scene(0b0001)) == [1]
    assert ids(eng.masked_scene(0x80000000)) == ["Plane"]
    assert ids(eng.masked_scene(0)) == [] and ids(eng.masked_scene(0b1000)) == []
    alone = eng.masked_scene(0b0100).objects                             # the instance without its base: a Mesh of its own
    assert len(alone) == 1 and isinstance(alone[0], M.Mesh) and alone[0].id == 5
    assert tuple(alone[0].transform) == tuple(inst.transform) and alone[0].positions is pos
    assert eng.masked_scene(0b0011).objects == [base, inst] and len(sc.objects) == 4
    # a static scene has no visibility to ask for; an object without an instance is never kept
    static = _Stub(sc, inst=[1, 0, -1, 3], visible=[False] * 4, masks=[1, 1, 1, 2], dynamic=False)
    assert ids(static.masked_scene(1)) == [1, 5] and ids(static.masked_scene(3)) == [1, 5, "Plane"]


def test_the_cpp_host_carries_the_interface(tmp_path):
    hpp = open(os.path.join(ROOT, "include", "rt_engine.hpp")).read()
    assert re.search(r"void\s+setMask\(int32_t objectIndex, uint32_t mask\)", hpp)
    assert re.search(r"uint32_t\s+maskOf\(int32_t objectIndex\)\s+const", hpp)
    assert re.search(r"FirstHits\s+firstHitsMasked\(uint32_t mask,", hpp)
    assert re.search(r"RayHits\s+queryClosest\(uint32_t mask,", hpp)
    assert re.search(r"RayHits\s+queryClosest\(const std::vector<uint32_t>& masks,", hpp)
    assert re.search(r"std::vector<uint8_t>\s+queryOccluded\(uint32_t mask,", hpp)
    assert re.search(r"std::vector<uint8_t>\s+queryOccluded\(const std::vector<uint32_t>& masks,", hpp)
    # the masked and the unmasked overloads compile and resolve side by side
    src = tmp_path / "use.cpp"
    src.write_text('#include "rt_engine.hpp"\n'
                   "void use(myrt::RayTracerEngine& e, const std::vector<double>& o, const std::vector<double>& d,\n"
                   "         const std::vector<uint32_t>& m) {\n"
                   "    e.setMask(0, 3u); (void)e.maskOf(0);\n"
                   "    (void)e.queryClosest(o, d); (void)e.queryClosest(1u, o, d); (void)e.queryClosest(m, o, d);\n"
                   "    (void)e.queryOccluded(o, d); (void)e.queryOccluded(1u, o, d); (void)e.queryOccluded(m, o, d);\n"
                   "    (void)e.firstHits(); (void)e.firstHitsMasked(2u);\n"
                   "}\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
