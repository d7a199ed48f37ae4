"""First-hit buffers, the interface: rtcore.h declares rt_render_gbuffer, rt_gbuffer and the flags;
the ctypes mirror has the header's layout; the library exports the symbol and refuses a NULL scene;
rt_engine.hpp's firstHits compiles.  RT_ABI_VERSION stays 5 (the entry point is appended under it
and detected by symbol).  No GPU."""
import ctypes as C
import os
import re
import subprocess

import myraytracer_amd as M
from myraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtcore.h")
FLAGS = (("RT_GBUFFER_DEVICE", 1), ("RT_GBUFFER_PIXEL_CENTRE", 2), ("RT_GBUFFER_FRAME_LAYOUT", 4))


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_interface():
    src = _code()
    assert re.search(r"\bint32_t\s+rt_render_gbuffer\s*\(\s*rt_scene\*\s*\w+,\s*int32_t\s+\w+,\s*int32_t\s+\w+,\s*"
                     r"int32_t\s+\w+,\s*int32_t\s+\w+,\s*const\s+rt_gbuffer\*\s*\w+,\s*uint32_t\s+\w+,\s*void\*\s*\w+\)", src)
    assert re.search(r"typedef struct rt_gbuffer\s*\{", src)
    for name, val in FLAGS:
        assert re.search(rf"#define\s+{name}\s+{val}u", src), name
        assert getattr(A, name) == val
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", src).group(1)) == 5 == A.RT_ABI_VERSION


def test_mirror_matches_the_header(tmp_path):
    assert A.GBUFFER_SYMBOLS == ["rt_render_gbuffer"] and set(A.GBUFFER_SYMBOLS) <= set(A.EXPORTED_SYMBOLS)
    fields = [f for f, _ in A.rt_gbuffer._fields_]
    assert fields == ["origin", "dir", "tmin", "time", "hits"]
    body = 'printf("rt_gbuffer %zu\\n", sizeof(rt_gbuffer));'
    body += "".join(f'printf("{f} %zu\\n", offsetof(rt_gbuffer, {f}));' for f in fields)
    prog = tmp_path / "sizes.c"
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(prog)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["rt_gbuffer"]) == C.sizeof(A.rt_gbuffer)
    for f in fields:
        assert int(got[f]) == getattr(A.rt_gbuffer, f).offset, f
    assert A.rt_gbuffer.hits.size == C.sizeof(A.rt_hit_batch)


def test_library_exports_and_refuses_without_a_scene():
    lib = M.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", M.engine.LIB_PATH], capture_output=True, text=True).stdout
    assert hasattr(lib, "rt_render_gbuffer") and re.search(r"\bT rt_render_gbuffer\b", out)
    gb = A.rt_gbuffer()
    assert lib.rt_render_gbuffer(None, 0, 0, 0, 1, C.byref(gb), 0, None) == A.RT_ERR_NO_SCENE
    assert b"scene" in lib.rt_last_error().lower()
    assert lib.rt_render_gbuffer(None, 0, 0, 0, 1, None, A.RT_GBUFFER_DEVICE, None) == A.RT_ERR_NO_SCENE


def test_the_python_host_names_the_method():
    import inspect
    sig = inspect.signature(M.RayTracerEngine.first_hits)
    assert list(sig.parameters)[1:] == ["camera_index", "chunk_first", "chunk_step", "want", "centre", "frame_layout",
                                        "slot", "out"]
    assert sig.parameters["want"].default == ("rays", "t", "ids")
    assert sig.parameters["want"].kind is inspect.Parameter.KEYWORD_ONLY
    assert set(M.engine.FirstHits.RAYS) == {"origins", "dirs", "tmin", "time"}


def test_the_cpp_host_names_the_method(tmp_path):
    src = tmp_path / "g.cpp"
    src.write_text('#include "rt_engine.hpp"\n'
                   "myrt::RayTracerEngine::FirstHits (myrt::RayTracerEngine::*a)(int32_t, int32_t, int32_t, uint32_t, "
                   "uint32_t, int32_t) = &myrt::RayTracerEngine::firstHits;\n"
                   "size_t use(myrt::RayTracerEngine& e) {\n"
                   "    myrt::RayTracerEngine::FirstHits f = e.firstHits();\n"
                   "    myrt::RayTracerEngine::FirstHits g = e.firstHits(0, 1, 2, myrt::RayTracerEngine::WantRays | "
                   "myrt::RayTracerEngine::WantNormal, RT_GBUFFER_PIXEL_CENTRE);\n"
                   "    const myrt::RayTracerEngine::RayHits& h = f.hits;\n"
                   "    return f.origins.size() + f.dirs.size() + f.tmin.size() + f.time.size() + h.ids.size() + "
                   "g.hits.normal.size() + (size_t)f.rows * (size_t)f.width;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", "-o",
                    str(tmp_path / "g.o"), str(src)], check=True)
