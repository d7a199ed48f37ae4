"""Deforming meshes, the interface: rtcore.h declares the three entry points, both flags and
rt_deform_stats; the ctypes mirror and the library agree; RT_ABI_VERSION stays 5 (the entry points
are appended under it and detected by symbol).  No GPU."""
import ctypes as C
import os
import re
import subprocess

import myraytracer_amd as M
from myraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtcore.h")
FUNCS = ("rt_scene_mesh_vertex_count", "rt_scene_set_mesh_positions", "rt_scene_last_deform_stats")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_interface():
    src = _code()
    for f in FUNCS:
        assert re.search(rf"\bint32_t\s+{f}\s*\(", src), f
    assert re.search(r"#define\s+RT_SCENE_DEFORMABLE\s+2u", src)
    assert re.search(r"#define\s+RT_POSITIONS_DEVICE\s+1u", src)
    assert re.search(r"typedef struct rt_deform_stats\s*\{", src)
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", src).group(1)) == 5


def test_mirror_matches_the_header(tmp_path):
    assert A.RT_ABI_VERSION == 5
    assert (A.RT_SCENE_DEFORMABLE, A.RT_POSITIONS_DEVICE, A.RT_SCENE_DYNAMIC) == (2, 1, 1)
    assert set(FUNCS) <= set(A.EXPORTED_SYMBOLS)
    names = [f for f, _ in A.rt_deform_stats._fields_]
    assert names == ["meshes_deformed", "triangles", "instances_rebounded", "validate_ms", "deform_ms", "blas_refit_ms"]
    prog = tmp_path / "sizes.c"
    body = 'printf("%zu\\n", sizeof(rt_deform_stats));' + "".join(
        f'printf("%zu\\n", offsetof(rt_deform_stats, {f}));' for f in names)
    body += 'printf("%u %u\\n", RT_SCENE_DEFORMABLE, RT_POSITIONS_DEVICE);'
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(prog)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert int(got[0]) == C.sizeof(A.rt_deform_stats) == 48
    for k, f in enumerate(names):
        assert int(got[1 + k]) == getattr(A.rt_deform_stats, f).offset
    assert got[-2:] == ["2", "1"]


def test_library_exports_and_refuses_without_a_scene():
    lib = M.load_library()
    assert lib.rt_version().endswith(b"(abi 5, gfx950, fp64)")
    n = C.c_int64(-1)
    assert lib.rt_scene_mesh_vertex_count(None, 0, C.byref(n)) == A.RT_ERR_NO_SCENE
    assert lib.rt_scene_set_mesh_positions(None, 0, None, 0, None, 0) == A.RT_ERR_NO_SCENE
    st = A.rt_deform_stats()
    assert lib.rt_scene_last_deform_stats(None, C.byref(st)) == A.RT_ERR_NO_SCENE


def test_host_build_with_the_flag_keeps_the_fp64_layouts():
    """rt_debug_wide_build accepts RT_SCENE_DEFORMABLE (a host-only build: the retained vertex ids,
    level lists and adjacency are made) and gives the trees of a dynamic build of the same scene."""
    import numpy as np
    import deform_scenes as DS
    lib = M.load_library()
    sc = DS.base_scene("smooth", sizes=(1, 3, 65))
    pk = sc.to_desc()
    a = M.engine._wide_dump(lambda io: lib.rt_debug_wide_build(pk.ptr, A.RT_SCENE_DEFORMABLE, C.byref(io)))
    b = M.engine._wide_dump(lambda io: lib.rt_debug_wide_build(pk.ptr, A.RT_SCENE_DYNAMIC, C.byref(io)))
    assert a["wide_root"] >= 0 and a["identity"] == 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    io = A.rt_wide_dump()
    assert lib.rt_debug_wide_build(pk.ptr, 4, C.byref(io)) == A.RT_ERR_INVALID_ARG
