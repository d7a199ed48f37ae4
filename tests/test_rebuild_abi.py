"""Rebuilding the flattened instance tree, the interface: rtcore.h declares rt_scene_commit_ex,
rt_scene_last_rebuild_stats, RT_COMMIT_REBUILD_FIT, the RT_REBUILD_* reasons and rt_rebuild_stats;
the ctypes mirror and the library agree; RT_ABI_VERSION stays 5 (the entry points are appended under
it and detected by symbol).  No GPU."""
import ctypes as C
import os
import re
import subprocess

import myraytracer_amd as M
from myraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtcore.h")
FUNCS = ("rt_scene_commit_ex", "rt_scene_last_rebuild_stats")
FIELDS = ["rebuilt", "reason", "pairs", "nodes_before", "nodes_after", "depth_before", "depth_after", "sort_ms",
          "build_ms", "total_ms"]
REASONS = ["RT_REBUILD_NONE", "RT_REBUILD_NO_TREE", "RT_REBUILD_BLOCKED", "RT_REBUILD_TOO_DEEP", "RT_REBUILD_TOO_LARGE",
           "RT_REBUILD_NO_MEMORY"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_interface():
    src = _code()
    for f in FUNCS:
        assert re.search(rf"\bint32_t\s+{f}\s*\(", src), f
    assert re.search(r"#define\s+RT_COMMIT_REBUILD_FIT\s+1u", src)
    assert re.search(r"typedef struct rt_rebuild_stats\s*\{", src)
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", src).group(1)) == 5


def test_mirror_matches_the_header(tmp_path):
    assert A.RT_ABI_VERSION == 5 and A.RT_COMMIT_REBUILD_FIT == 1
    assert set(FUNCS) <= set(A.EXPORTED_SYMBOLS) and list(FUNCS) == A.REBUILD_SYMBOLS
    assert [f for f, _ in A.rt_rebuild_stats._fields_] == FIELDS
    prog = tmp_path / "sizes.c"
    body = 'printf("%zu\\n", sizeof(rt_rebuild_stats));' + "".join(
        f'printf("%zu\\n", offsetof(rt_rebuild_stats, {f}));' for f in FIELDS)
    body += 'printf("%u\\n", RT_COMMIT_REBUILD_FIT);' + "".join(f'printf("%d\\n", {r});' for r in REASONS)
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(prog)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert int(got[0]) == C.sizeof(A.rt_rebuild_stats) == 72
    for k, f in enumerate(FIELDS):
        assert int(got[1 + k]) == getattr(A.rt_rebuild_stats, f).offset
    assert int(got[1 + len(FIELDS)]) == A.RT_COMMIT_REBUILD_FIT
    assert [int(x) for x in got[2 + len(FIELDS):]] == [getattr(A, r) for r in REASONS] == list(range(6))


def test_library_exports_and_refuses_without_a_scene():
    lib = M.load_library()
    assert lib.rt_version().endswith(b"(abi 5, gfx950, fp64)")
    cs = A.rt_commit_stats()
    assert lib.rt_scene_commit_ex(None, A.RT_COMMIT_REBUILD_FIT, C.byref(cs)) == A.RT_ERR_NO_SCENE
    assert lib.rt_scene_commit_ex(None, 0, None) == A.RT_ERR_NO_SCENE
    st = A.rt_rebuild_stats()
    assert lib.rt_scene_last_rebuild_stats(None, C.byref(st)) == A.RT_ERR_NO_SCENE
    assert b"scene" in lib.rt_last_error().lower()


def test_the_python_engine_carries_the_interface():
    import inspect
    sig = inspect.signature(M.RayTracerEngine.commit)
    assert sig.parameters["rebuild"].default is False
    assert callable(M.RayTracerEngine.last_rebuild_stats)


def test_the_cpp_host_carries_the_interface():
    hpp = open(os.path.join(ROOT, "include", "rt_engine.hpp")).read()
    assert re.search(r"rt_commit_stats\s+commit\(bool rebuild = false\)", hpp)
    assert re.search(r"rt_rebuild_stats\s+lastRebuildStats\(\)\s+const", hpp)
