"""ju_set_stage_group without a GPU (docs/source_stage.md and docs/output_stage.md, "Group passes"): the entry point and
the two kernels' test hooks are declared, exported and bound; a NULL runtime and the hooks' bad arguments are refused before
any device call; the setting, its stat keys and what the slots cost are documented where a caller looks for them, and no
document says any longer that group passes are not provided for scaled or masked members."""

import ctypes as C
import os
import re

from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("ju_debug_scale_members", "ju_debug_yuv_items_sized")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_setter_is_declared_exported_and_bound(hip_library, product_library):
    header, test_header = read("include", "joshupscale_amd.h"), read("include", "joshupscale_amd_test.h")
    assert re.search(r"JU_API\s+int\s+ju_set_stage_group\s*\(\s*ju_runtime\s*\*\s*\w*\s*,\s*int\s+on\s*\)", header)
    assert "ju_set_stage_group" in R.PRODUCT_SYMBOLS and "ju_set_stage_group" not in R.HOOK_SYMBOLS
    assert hasattr(product_library, "ju_set_stage_group") and hasattr(hip_library, "ju_set_stage_group")
    assert callable(R.Runtime.set_stage_group)
    assert R._PRODUCT_SIGS["ju_set_stage_group"] == R._PRODUCT_SIGS["ju_set_scene_group"]    # (rt, int) -> int
    # the kernels' hooks: the test flavour only
    for hook in HOOKS:
        assert re.search(r"JU_API\s+int\s+" + hook + r"\s*\(", test_header) and hook not in header
        assert hook in R.HOOK_SYMBOLS and hook not in R.PRODUCT_SYMBOLS
        assert hasattr(hip_library, hook) and not hasattr(product_library, hook)
    # the C++ plugin surface stays as it is
    assert "stage_group" not in read("include", "JoshUpscale", "core.h")


def test_a_null_runtime_is_refused_without_a_gpu(hip_library, product_library):
    for lib in (hip_library, product_library):
        for on in (0, 1, 2):
            assert lib.ju_set_stage_group(None, on) == 1                         # JU_ERR_INVALID_ARGUMENT
            assert "runtime is NULL" in lib.ju_last_error().decode()
        value = C.c_double(7)
        for key in (b"stage_group", b"group_staged_frames"):
            assert lib.ju_get_stat(None, key, C.byref(value)) == 1 and value.value == 7


def test_the_refusal_text_is_the_one_the_header_gives():
    """(the value check itself needs a runtime, and a runtime a device: tests/test_gpu_stage_group.py holds the call to this
    text; here the text in the sources and the header is held to one wording)"""
    text = "ju_set_stage_group: on must be 0 or 1, got "
    assert text in read("joshupscale_amd", "csrc", "engine_passes.cpp")
    assert text + "N" in " ".join(read("include", "joshupscale_amd.h").replace("*", " ").split())


def test_the_members_hook_refuses_bad_arguments_without_a_gpu(hip_library):
    fake = (C.c_void_p * 9)(*([0x1000] * 9))                     # (never read: every case is refused before a device call)
    null, strides, filts = (C.c_void_p * 9)(), (C.c_ssize_t * 9)(), (C.c_int * 9)()
    sizes = (C.c_size_t * 9)(*([46] * 9))

    def call(count, dst=fake, src=fake, filters=filts, dst_w=24, w=sizes):
        rc = hip_library.ju_debug_scale_members(count, filters, dst, strides, dst_w, 16, src, strides, w, sizes)
        return rc, hip_library.ju_last_error().decode() if rc else ""

    for count in (0, -1, 9):
        assert call(count) == (1, "std::invalid_argument: ju_debug_scale_members: count must be 1 .. 8")
    for kw in (dict(dst=None), dict(src=None), dict(filters=None), dict(w=None)):
        assert call(2, **kw) == (1, "std::invalid_argument: ju_debug_scale_members: NULL array")
    assert call(2, dst_w=0) == (1, "std::invalid_argument: ju_debug_scale_members: a size outside 1 .. 32768")
    assert call(2, w=(C.c_size_t * 9)(46, (1 << 15) + 1)) == (1, "std::invalid_argument: ju_debug_scale_members: a size outside 1 .. 32768")
    assert call(2, dst=null) == (1, "std::invalid_argument: ju_debug_scale_members: NULL buffer")
    # member 1: Catmull-Rom beyond its factor of 8, beside a triangle member inside its 16; then an unknown filter
    rc, msg = call(2, filters=(C.c_int * 9)(0, 2), w=(C.c_size_t * 9)(216, 216))
    assert rc == 1 and "216 -> 24 is beyond a factor of 8" in msg, msg
    rc, msg = call(2, filters=(C.c_int * 9)(0, 1))
    assert rc == 1 and "unknown filter 1" in msg, msg


def test_the_sized_decode_hook_refuses_bad_arguments_without_a_gpu(hip_library):
    n = 2
    fmts, css = (C.c_int * n)(R.FMT_NV12, R.FMT_YUY2), (C.c_int * n)(0, 0)
    fake, strides = (C.c_void_p * n)(0x1000, 0x1000), (C.c_ssize_t * n)(512, 512)
    planes, pstrides = (C.c_void_p * (3 * n))(*([0x1000] * 6)), (C.c_ssize_t * (3 * n))(*([512] * 6))

    def call(count=n, formats=fmts, widths=(48, 50), heights=(30, 34), images=fake):
        rc = hip_library.ju_debug_yuv_items_sized(count, formats, css, (C.c_size_t * n)(*widths) if widths else None,
                                                  (C.c_size_t * n)(*heights), images, strides, planes, pstrides)
        return rc, hip_library.ju_last_error().decode() if rc else ""

    for count in (0, -1, 9):
        assert call(count=count) == (1, "std::invalid_argument: ju_debug_yuv_items_sized: 1 .. 8 items")
    assert call(widths=None) == (1, "std::invalid_argument: ju_debug_yuv_items_sized: null argument")
    assert call(formats=(C.c_int * n)(R.FMT_NV12, 99)) == (1, "std::invalid_argument: ju_debug_yuv_items_sized: not a YUV format")
    # each item's own size is held to its own format's parity: an odd height for the 4:2:0 item, an odd width for the 4:2:2 one
    for kw in (dict(heights=(31, 34)), dict(widths=(48, 51)), dict(widths=(48, 0))):
        rc, msg = call(**kw)
        assert rc == 1 and "sizes 1 .. 32768, an even width for 4:2:0 and 4:2:2, an even height for 4:2:0" in msg, msg
    assert call(images=(C.c_void_p * n)(0x1000, None)) == (1, "std::invalid_argument: ju_debug_yuv_items_sized: null buffer")


def test_the_setting_and_its_stat_keys_are_documented():
    header = read("include", "joshupscale_amd.h")
    source_doc, output_doc = read("docs", "source_stage.md"), read("docs", "output_stage.md")
    for text in (header, source_doc, output_doc, R.Runtime.stat.__doc__):
        assert '"stage_group"' in text or "`stage_group`" in text
        assert '"group_staged_frames"' in text or "`group_staged_frames`" in text
    for text in (header, source_doc, output_doc, read("INTEGRATION.md"), read("README.md")):
        assert "ju_set_stage_group" in text
    for doc in (source_doc, output_doc):
        assert re.search(r"^## Group passes", doc, re.M)
        assert "MB" in doc.split("## Group passes")[1]            # what the slots cost
    assert "scale_bgrx_members_kernel" in source_doc


def test_no_document_says_that_group_passes_are_not_provided_for_staged_members():
    header = read("include", "joshupscale_amd.h")
    limit = "scaled or masked frames inside group passes"
    for text in (header, read("docs", "source_stage.md"), read("docs", "output_stage.md"), read("INTEGRATION.md"), read("README.md")):
        flat = " ".join(text.replace("*", " ").split())
        # the old, unconditional limit is gone: where the words remain, they speak of a runtime that has not asked to ride
        # and name the setting that provides it in the same sentence
        for tail in flat.split(limit)[1:]:
            assert tail.startswith(" of a runtime that has not asked to ride") and "ju_set_stage_group" in tail.split(";")[0]
        assert "always runs on its own" not in flat
        assert "members under a source size, an output size or a mask inside group passes" not in flat
    # and the engine's own comment no longer says "whatever" without the exception
    assert "no stage: a scaled or masked member stays" not in read("joshupscale_amd", "csrc", "engine_passes.cpp")
