"""ju_set_scene_lookahead without a GPU (docs/scene_detect.md "Passes"): the entry point and the kernel's test hook are
declared, exported and bound; NULL runtimes and the hook's bad arguments are refused before any device call; the stat keys
and the setting are documented where a caller looks for them."""

import ctypes as C
import os
import re

from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_setter_is_declared_exported_and_bound(hip_library, product_library):
    header, test_header = read("include", "joshupscale_amd.h"), read("include", "joshupscale_amd_test.h")
    assert re.search(r"JU_API\s+int\s+ju_set_scene_lookahead\s*\(\s*ju_runtime\s*\*\s*\w*\s*,\s*int\s+on\s*\)", header)
    assert "ju_set_scene_lookahead" in R.PRODUCT_SYMBOLS and "ju_set_scene_lookahead" not in R.HOOK_SYMBOLS
    assert hasattr(product_library, "ju_set_scene_lookahead") and hasattr(hip_library, "ju_set_scene_lookahead")
    assert callable(R.Runtime.set_scene_lookahead)
    # the kernel's hook: the test flavour only
    assert re.search(r"JU_API\s+int\s+ju_debug_scene_pass\s*\(", test_header) and "ju_debug_scene_pass" not in header
    assert "ju_debug_scene_pass" in R.HOOK_SYMBOLS and "ju_debug_scene_pass" not in R.PRODUCT_SYMBOLS
    assert hasattr(hip_library, "ju_debug_scene_pass") and not hasattr(product_library, "ju_debug_scene_pass")


def test_a_null_runtime_is_refused_without_a_gpu(hip_library, product_library):
    for lib in (hip_library, product_library):
        for on in (0, 1, 2):
            assert lib.ju_set_scene_lookahead(None, on) == 1                     # JU_ERR_INVALID_ARGUMENT
            assert "runtime is NULL" in lib.ju_last_error().decode()
        value = C.c_double(7)
        for key in (b"scene_lookahead", b"scene_pass_frames"):
            assert lib.ju_get_stat(None, key, C.byref(value)) == 1 and value.value == 7


def test_the_hook_refuses_bad_arguments_without_a_gpu(hip_library):
    recs = (R.JuSceneInfo * 9)()
    reset_at, cut_at = (C.c_uint32 * 9)(), (C.c_int32 * 9)()
    ptrs, strides = (C.c_void_p * 9)(), (C.c_ssize_t * 9)()

    def call(count, frames=ptrs, has_prev=3, records=recs):
        rc = hip_library.ju_debug_scene_pass(count, frames, strides, 48, 30, None, None, None, has_prev, 0, 22000, 1, records,
                                             reset_at, cut_at)
        return rc, hip_library.ju_last_error().decode() if rc else ""

    for count in (0, -1, 9):
        assert call(count) == (1, "std::invalid_argument: ju_debug_scene_pass: count must be 1 .. 8")
    assert call(2, frames=None) == (1, "std::invalid_argument: ju_debug_scene_pass: NULL array")
    assert call(2, records=None) == (1, "std::invalid_argument: ju_debug_scene_pass: NULL array")
    for has_prev in (2, 4, -1):
        assert call(2, has_prev=has_prev) == (1, "std::invalid_argument: ju_debug_scene_pass: has_prev must be 0, 1 or 3")


def test_the_setting_and_its_stat_keys_are_documented():
    header, doc = read("include", "joshupscale_amd.h"), read("docs", "scene_detect.md")
    for text in (header, doc, R.Runtime.stat.__doc__):
        assert '"scene_lookahead"' in text and '"scene_pass_frames"' in text
    for text in (header, doc, read("INTEGRATION.md")):
        assert "ju_set_scene_lookahead" in text and "Not provided: a pass split at a cut" not in text
    assert "ju_process_group" in doc.split("Not provided")[-1]       # group passes for a detecting runtime: named as missing
    assert "scene_lookahead" in read("README.md")
