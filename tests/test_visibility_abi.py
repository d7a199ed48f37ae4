"""Instance visibility, the interface: rtcore.h declares rt_scene_set_instance_visible,
rt_scene_set_instances_visible, rt_scene_instance_visible, rt_visibility_stats and
rt_scene_last_visibility_stats; the ctypes mirror and the library agree; RT_ABI_VERSION stays 5 (the
entry points are appended and detected by symbol) and the lists earlier ABI tests pin stay.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import myraytracer_amd as M
from myraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtcore.h")
FUNCS = ("rt_scene_set_instance_visible", "rt_scene_set_instances_visible", "rt_scene_instance_visible",
         "rt_scene_last_visibility_stats")
FIELDS = ["instances", "visible", "shown", "hidden", "pairs", "pairs_visible", "pairs_in_tree", "forced_rebuild",
          "fit_complete"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_interface():
    src = _code()
    assert re.search(r"typedef struct rt_visibility_stats\s*\{", src)
    for f in FUNCS:
        assert re.search(rf"\bint32_t\s+{f}\s*\(", src), f
    assert re.search(r"rt_scene_set_instance_visible\s*\(\s*rt_scene\s*\*[^,]*,\s*int32_t[^,]*,\s*int32_t[^,)]*\)", src)
    assert re.search(r"rt_scene_set_instances_visible\s*\(\s*rt_scene\s*\*[^,]*,\s*int32_t[^,]*,\s*int32_t[^,]*,"
                     r"\s*const uint8_t\s*\*", src)
    assert re.search(r"rt_scene_instance_visible\s*\(\s*const rt_scene\s*\*[^,]*,\s*int32_t[^,]*,\s*int32_t\s*\*", src)
    assert re.search(r"rt_scene_last_visibility_stats\s*\(\s*const rt_scene\s*\*[^,]*,\s*rt_visibility_stats\s*\*", src)
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", src).group(1)) == 5
    # the blanket sentence is gone from the header and from DESIGN.md: both now say what is possible
    text = open(HEADER).read() + open(os.path.join(ROOT, "DESIGN.md")).read()
    assert not re.search(r"can\s+(still\s+)?not\s+be\s+added\s+or\s+removed", re.sub(r"[\s*]+", " ", text))


def test_mirror_matches_the_header(tmp_path):
    assert A.RT_ABI_VERSION == 5
    assert A.VISIBILITY_SYMBOLS == list(FUNCS) and set(FUNCS) <= set(A.EXPORTED_SYMBOLS)
    assert A.REBUILD_SYMBOLS == ["rt_scene_commit_ex", "rt_scene_last_rebuild_stats"]
    assert A.REBUILD_DETAIL_SYMBOLS == ["rt_scene_last_rebuild_detail", "rt_scene_fit_cost"]
    assert [f for f, _ in A.rt_visibility_stats._fields_] == FIELDS
    prog = tmp_path / "sizes.c"
    body = 'printf("%zu\\n", sizeof(rt_visibility_stats));printf("%zu\\n", sizeof(rt_commit_stats));' + "".join(
        f'printf("%zu\\n", offsetof(rt_visibility_stats, {f}));' for f in FIELDS)
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(A.rt_visibility_stats) == 64
    assert got[1] == C.sizeof(A.rt_commit_stats) == 32              # keeps its layout
    for k, f in enumerate(FIELDS):
        assert got[2 + k] == getattr(A.rt_visibility_stats, f).offset, f


def test_library_exports_and_refuses_without_a_scene():
    lib = M.load_library()
    assert lib.rt_version().endswith(b"(abi 5, gfx950, fp64)")
    for f in FUNCS:
        assert hasattr(lib, f), f
    v = C.c_int32(7)
    flags = (C.c_uint8 * 2)(1, 0)
    st = A.rt_visibility_stats()
    assert lib.rt_scene_set_instance_visible(None, 0, 0) == A.RT_ERR_NO_SCENE
    assert b"scene" in lib.rt_last_error().lower()
    assert lib.rt_scene_set_instances_visible(None, 0, 2, flags) == A.RT_ERR_NO_SCENE
    assert lib.rt_scene_instance_visible(None, 0, C.byref(v)) == A.RT_ERR_NO_SCENE and v.value == 7
    assert lib.rt_scene_last_visibility_stats(None, C.byref(st)) == A.RT_ERR_NO_SCENE


def test_the_python_engine_carries_the_interface():
    E = M.RayTracerEngine
    for name in ("set_visible", "set_visible_many", "is_visible", "last_visibility_stats", "visible_scene"):
        assert callable(getattr(E, name)), name
    assert list(inspect.signature(E.set_visible).parameters) == ["self", "object_index", "visible"]
    assert list(inspect.signature(E.is_visible).parameters) == ["self", "object_index"]
    sig = inspect.signature(E.commit)                                 # commit's signature stays
    assert list(sig.parameters) == ["self", "rebuild"] and sig.parameters["rebuild"].default is False


def test_visible_subset_keeps_an_instance_whose_base_is_hidden():
    """A MeshInstance kept while its base mesh is hidden becomes a Mesh of its own with the same
    triangles and matrix; kept together with its base it stays a MeshInstance."""
    import numpy as np
    from myraytracer_amd import engine
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    base = M.Mesh(id=1, material="2", positions=pos, indices=np.array([[0, 1, 2]], np.int32), indices_one_based=False)
    inst = M.MeshInstance(id=5, base_mesh_id=1, transform=M.translation(1.0, 2.0, 3.0))
    sc = M.Scene(cameras=[], materials=[], objects=[base, inst, M.Sphere((0.0, 0.0, 0.0), 1.0)])
    both = engine.visible_subset(sc, [True, True, False])
    assert both.objects == [base, inst] and len(sc.objects) == 3
    alone = engine.visible_subset(sc, [False, True, True]).objects
    assert isinstance(alone[0], M.Mesh) and alone[0].id == 5 and alone[0].material == "2"
    assert alone[0].positions is pos and tuple(alone[0].transform) == tuple(inst.transform)
    assert isinstance(alone[1], M.Sphere) and engine.visible_subset(sc, [False] * 3).objects == []


def test_the_cpp_host_carries_the_interface():
    hpp = open(os.path.join(ROOT, "include", "rt_engine.hpp")).read()
    assert re.search(r"void\s+setVisible\(int32_t objectIndex, bool visible\)", hpp)
    assert re.search(r"bool\s+isVisible\(int32_t objectIndex\)\s+const", hpp)
    assert re.search(r"rt_visibility_stats\s+lastVisibilityStats\(\)\s+const", hpp)
