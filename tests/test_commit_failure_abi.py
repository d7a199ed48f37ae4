"""How a commit ends, the interface: the two test hooks debug_fail_commit_alloc and
debug_fail_commit_step are unsafe options (rt_scene_set_option refuses them, rt_scene_set_unsafe_option
takes them), both entry points answer RT_ERR_NO_SCENE without a scene, no ABI symbol was added and the
header, the C++ host and the Python engine state the contract.  No GPU: with a scene the refusal and the
acceptance are shown by tests/test_gpu_commit_failures.py."""
import os
import re

import myraytracer_amd as M
from myraytracer_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("debug_fail_commit_alloc", "debug_fail_commit_step")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_hooks_are_unsafe_options_that_default_to_off():
    src = _read("myraytracer_amd", "csrc", "render.hip")
    for name, hi in zip(HOOKS, ("1 << 20", "10")):
        m = re.search(r'\{"%s",\s*(-?\d+),\s*(-?\d+),\s*([^,]+),\s*(true|false)?\}' % name, src)
        assert m, name
        assert (m.group(1), m.group(2), m.group(3).strip(), m.group(4)) == ("0", "0", hi, "true"), m.groups()
    # read by the commit alone
    for opt in ("kOptDebugFailCommitAlloc", "kOptDebugFailCommitStep"):
        assert len(re.findall(r"\b%s\b" % opt, src)) == 1                           # the enum
        assert re.search(r"\b%s\b" % opt, _read("myraytracer_amd", "csrc", "commit.h"))
        for other in ("query.h", "refit.h", "rebuild.h", "deform.h", "render_full.h", "wide.h", "device.h"):
            assert not re.search(r"\b%s\b" % opt, _read("myraytracer_amd", "csrc", other)), (opt, other)


def test_both_entry_points_refuse_without_a_scene():
    lib = M.load_library()
    for name in HOOKS:
        assert lib.rt_scene_set_option(None, name.encode(), 1) == A.RT_ERR_NO_SCENE
        assert lib.rt_scene_set_unsafe_option(None, name.encode(), 1) == A.RT_ERR_NO_SCENE
        assert b"scene" in lib.rt_last_error().lower()


def test_no_symbol_was_added_and_the_contract_is_written_down():
    assert A.RT_ABI_VERSION == 5 and lib_version_is_5()
    hdr = re.sub(r"\s*\n\s*\*\s*", " ", _read("include", "rtcore.h"))
    assert "How a commit ends" in hdr
    for phrase in ("RT_ERR_OOM for every host or device allocation", "keep reporting the last SUCCESSFUL commit",
                   "reason = RT_REBUILD_NO_MEMORY", "The scene lost", "rt_scene_destroy and the rt_scene_last_* getters still work"):
        assert phrase in hdr, phrase
    for name in HOOKS:
        assert name in hdr
        assert name in _read("INTEGRATION.md")
    design = _read("DESIGN.md")
    assert "debug_fail_commit_alloc" in design and "scene is lost" in design
    assert "RT_ERR_DEVICE" in _read("include", "rt_engine.hpp").split("rt_commit_stats commit(bool rebuild")[0].rsplit("/*", 1)[1]
    assert "lost" in M.RayTracerEngine.commit.__doc__


def lib_version_is_5():
    return M.load_library().rt_version().endswith(b"(abi 5, gfx950, fp64)")
