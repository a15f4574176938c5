"""ju_set_stage_lookahead without a GPU (docs/source_stage.md and docs/output_stage.md, "Passes"): the entry point and the
items kernel's test hook are declared, exported and bound; a NULL runtime and the hook's bad arguments are refused before
any device call; the stat keys and the setting are documented where a caller looks for them, and no document says any
longer that passes are not provided for scaled frames."""

import ctypes as C
import os
import re

from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_setter_is_declared_exported_and_bound(hip_library, product_library):
    header, test_header = read("include", "joshupscale_amd.h"), read("include", "joshupscale_amd_test.h")
    assert re.search(r"JU_API\s+int\s+ju_set_stage_lookahead\s*\(\s*ju_runtime\s*\*\s*\w*\s*,\s*int\s+on\s*\)", header)
    assert "ju_set_stage_lookahead" in R.PRODUCT_SYMBOLS and "ju_set_stage_lookahead" not in R.HOOK_SYMBOLS
    assert hasattr(product_library, "ju_set_stage_lookahead") and hasattr(hip_library, "ju_set_stage_lookahead")
    assert callable(R.Runtime.set_stage_lookahead)
    # the kernel's hook: the test flavour only
    assert re.search(r"JU_API\s+int\s+ju_debug_scale_items\s*\(", test_header) and "ju_debug_scale_items" not in header
    assert "ju_debug_scale_items" in R.HOOK_SYMBOLS and "ju_debug_scale_items" not in R.PRODUCT_SYMBOLS
    assert hasattr(hip_library, "ju_debug_scale_items") and not hasattr(product_library, "ju_debug_scale_items")


def test_a_null_runtime_is_refused_without_a_gpu(hip_library, product_library):
    for lib in (hip_library, product_library):
        for on in (0, 1, 2):
            assert lib.ju_set_stage_lookahead(None, on) == 1                     # JU_ERR_INVALID_ARGUMENT
            assert "runtime is NULL" in lib.ju_last_error().decode()
        value = C.c_double(7)
        for key in (b"stage_lookahead", b"lookahead_staged_frames"):
            assert lib.ju_get_stat(None, key, C.byref(value)) == 1 and value.value == 7


def test_the_hook_refuses_bad_arguments_without_a_gpu(hip_library):
    ptrs, strides = (C.c_void_p * 9)(), (C.c_ssize_t * 9)()

    def call(count, dst=ptrs, src=ptrs, dst_w=24, src_w=46):
        rc = hip_library.ju_debug_scale_items(count, 0, dst, strides, dst_w, 16, src, strides, src_w, 30)
        return rc, hip_library.ju_last_error().decode() if rc else ""

    for count in (0, -1, 9):
        assert call(count) == (1, "std::invalid_argument: ju_debug_scale_items: count must be 1 .. 8")
    assert call(2, dst=None) == (1, "std::invalid_argument: ju_debug_scale_items: NULL array")
    assert call(2, src=None) == (1, "std::invalid_argument: ju_debug_scale_items: NULL array")
    assert call(2, dst_w=0) == (1, "std::invalid_argument: ju_debug_scale_items: a size outside 1 .. 32768")
    assert call(2, src_w=(1 << 15) + 1) == (1, "std::invalid_argument: ju_debug_scale_items: a size outside 1 .. 32768")
    assert call(2) == (1, "std::invalid_argument: ju_debug_scale_items: NULL buffer")


def test_the_setting_and_its_stat_keys_are_documented():
    header = read("include", "joshupscale_amd.h")
    source_doc, output_doc = read("docs", "source_stage.md"), read("docs", "output_stage.md")
    for text in (header, source_doc, output_doc, R.Runtime.stat.__doc__):
        assert '"stage_lookahead"' in text or "`stage_lookahead`" in text
        assert '"lookahead_staged_frames"' in text or "`lookahead_staged_frames`" in text
    for text in (header, source_doc, output_doc, read("INTEGRATION.md"), read("README.md")):
        assert "ju_set_stage_lookahead" in text
    for doc in (source_doc, output_doc):
        assert re.search(r"^## Passes", doc, re.M)
        assert "MB" in doc.split("## Passes")[1]                  # what the slots cost


def test_no_document_says_that_passes_are_not_provided_for_scaled_frames():
    header = read("include", "joshupscale_amd.h")
    for text in (header, read("docs", "source_stage.md"), read("docs", "output_stage.md")):
        flat = " ".join(text.replace("*", " ").split())
        assert "scaled or masked frames inside look-ahead" not in flat
    # group passes stay named as missing
    flat = " ".join(header.replace("*", " ").split())
    assert "Not provided: scaled or masked frames inside group passes" in flat
