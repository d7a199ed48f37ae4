"""The clustered builder of the flattened instance tree, the interface: rtcore.h declares
RT_COMMIT_REBUILD_FIT_CLUSTERED, rt_rebuild_detail, rt_scene_last_rebuild_detail and
rt_scene_fit_cost; the ctypes mirror and the library agree; what test_rebuild_abi.py pins stays
(RT_ABI_VERSION 5, REBUILD_SYMBOLS, rt_rebuild_stats, commit's default).  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import myraytracer_amd as M
from myraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtcore.h")
FUNCS = ("rt_scene_last_rebuild_detail", "rt_scene_fit_cost")
FIELDS = ["builder", "iterations", "fell_back", "pad", "cluster_ms", "cost_before", "cost_after"]


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_interface():
    src = _code()
    assert re.search(r"#define\s+RT_COMMIT_REBUILD_FIT_CLUSTERED\s+8u", src)
    assert re.search(r"#define\s+RT_COMMIT_REBUILD_FIT\s+1u", src)
    assert re.search(r"typedef struct rt_rebuild_detail\s*\{", src)
    for f in FUNCS + ("rt_scene_commit_ex",):
        assert re.search(rf"\bint32_t\s+{f}\s*\(", src), f
    assert re.search(r"rt_scene_last_rebuild_detail\s*\(\s*const rt_scene\s*\*[^,]*,\s*rt_rebuild_detail\s*\*", src)
    assert re.search(r"rt_scene_fit_cost\s*\(\s*rt_scene\s*\*[^,]*,\s*double\s*\*", src)
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", src).group(1)) == 5


def test_mirror_matches_the_header(tmp_path):
    assert A.RT_ABI_VERSION == 5 and A.RT_COMMIT_REBUILD_FIT == 1 and A.RT_COMMIT_REBUILD_FIT_CLUSTERED == 8
    assert A.REBUILD_SYMBOLS == ["rt_scene_commit_ex", "rt_scene_last_rebuild_stats"]
    assert A.REBUILD_DETAIL_SYMBOLS == list(FUNCS) and set(FUNCS) <= set(A.EXPORTED_SYMBOLS)
    assert [f for f, _ in A.rt_rebuild_detail._fields_] == FIELDS
    prog = tmp_path / "sizes.c"
    body = 'printf("%zu\\n", sizeof(rt_rebuild_detail));printf("%zu\\n", sizeof(rt_rebuild_stats));' + "".join(
        f'printf("%zu\\n", offsetof(rt_rebuild_detail, {f}));' for f in FIELDS)
    body += 'printf("%u\\n", RT_COMMIT_REBUILD_FIT_CLUSTERED);'
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(A.rt_rebuild_detail) == 40
    assert got[1] == C.sizeof(A.rt_rebuild_stats) == 72
    for k, f in enumerate(FIELDS):
        assert got[2 + k] == getattr(A.rt_rebuild_detail, f).offset, f
    assert got[2 + len(FIELDS)] == A.RT_COMMIT_REBUILD_FIT_CLUSTERED


def test_library_exports_and_refuses_without_a_scene():
    lib = M.load_library()
    assert lib.rt_version().endswith(b"(abi 5, gfx950, fp64)")
    for f in FUNCS:
        assert hasattr(lib, f), f
    dt = A.rt_rebuild_detail()
    assert lib.rt_scene_last_rebuild_detail(None, C.byref(dt)) == A.RT_ERR_NO_SCENE
    cost = C.c_double(-1.0)
    assert lib.rt_scene_fit_cost(None, C.byref(cost)) == A.RT_ERR_NO_SCENE
    assert b"scene" in lib.rt_last_error().lower()
    cs = A.rt_commit_stats()
    for flags in (A.RT_COMMIT_REBUILD_FIT_CLUSTERED, A.RT_COMMIT_REBUILD_FIT | A.RT_COMMIT_REBUILD_FIT_CLUSTERED):
        assert lib.rt_scene_commit_ex(None, flags, C.byref(cs)) == A.RT_ERR_NO_SCENE


def test_the_python_engine_carries_the_interface():
    sig = inspect.signature(M.RayTracerEngine.commit)
    assert sig.parameters["rebuild"].default is False
    assert callable(M.RayTracerEngine.last_rebuild_detail) and callable(M.RayTracerEngine.fit_cost)
    assert callable(M.RayTracerEngine.last_rebuild_stats)

    class _Lib:                                            # records the flags commit() hands to the library
        def __init__(self):
            self.calls = []

        def rt_scene_commit_ex(self, h, flags, st):
            self.calls.append(("ex", flags))
            return 0

        def rt_scene_commit(self, h, st):
            self.calls.append(("plain", 0))
            return 0

    from myraytracer_amd import engine
    fake, real = _Lib(), engine.load_library
    eng = M.RayTracerEngine.__new__(M.RayTracerEngine)
    eng._h = None
    engine.load_library = lambda: fake
    try:
        eng.commit()
        eng.commit(rebuild=True)
        eng.commit(rebuild="clustered")
        with pytest.raises(ValueError):
            eng.commit(rebuild="sah")
    finally:
        engine.load_library = real
    assert fake.calls == [("plain", 0), ("ex", A.RT_COMMIT_REBUILD_FIT), ("ex", A.RT_COMMIT_REBUILD_FIT_CLUSTERED)]


def test_the_cpp_host_carries_the_interface():
    hpp = open(os.path.join(ROOT, "include", "rt_engine.hpp")).read()
    assert re.search(r"rt_commit_stats\s+commit\(bool rebuild = false\)", hpp)
    assert re.search(r"rt_commit_stats\s+commitEx\(uint32_t flags\)", hpp)
    assert re.search(r"rt_rebuild_detail\s+lastRebuildDetail\(\)\s+const", hpp)
    assert re.search(r"double\s+fitCost\(\)", hpp)
