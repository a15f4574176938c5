"""ju_process_frames without a GPU: the declaration, the export, the refusals that need no runtime, and the Python
binding's own check (which comes before any native call)."""

import ctypes as C
import os
import re

import pytest

from helpers import ROOT
from joshupscale_amd import runtime as R

JU_ERR_INVALID_ARGUMENT = 1


def test_header_declares_process_frames():
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    m = re.search(r"JU_API\s+int\s+ju_process_frames\s*\(([^)]*)\)", text)
    assert m, "ju_process_frames is not declared"
    args = " ".join(m.group(1).split())
    assert args == "ju_runtime *runtime, const ju_frame *inputs, const ju_frame *outputs, int count", args
    assert "ju_process_frames" in R.PRODUCT_SYMBOLS
    assert "no YUV frames in ju_process_batch look-ahead passes" not in " ".join(text.split())


def test_both_library_flavours_export_process_frames(product_library, hip_library):
    assert hasattr(product_library, "ju_process_frames")
    assert hasattr(hip_library, "ju_process_frames")
    # the hook that runs the pass's decode kernel alone: test flavour only
    assert "ju_debug_yuv_items" in R.HOOK_SYMBOLS
    assert hasattr(hip_library, "ju_debug_yuv_items") and not hasattr(product_library, "ju_debug_yuv_items")
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    assert re.search(r"JU_API\s+int\s+ju_debug_yuv_items\s*\(", test_header)


def test_null_arrays_and_negative_counts_are_refused_without_a_gpu(product_library):
    lib = product_library
    frames = (R.JuFrame * 2)()
    # count == 0: nothing to do, whatever else is passed
    assert lib.ju_process_frames(None, None, None, 0) == 0
    assert lib.ju_process_frames(None, frames, frames, 0) == 0
    assert lib.ju_process_frames(None, None, frames, 2) == JU_ERR_INVALID_ARGUMENT
    assert b"ju_process_frames" in lib.ju_last_error()
    assert lib.ju_process_frames(None, frames, None, 2) == JU_ERR_INVALID_ARGUMENT
    assert b"ju_process_frames" in lib.ju_last_error()
    assert lib.ju_process_frames(None, frames, frames, -1) == JU_ERR_INVALID_ARGUMENT
    assert b"ju_process_frames" in lib.ju_last_error()
    assert lib.ju_process_frames(None, None, None, -3) == JU_ERR_INVALID_ARGUMENT
    # a NULL runtime with frames to process: refused too, nothing to launch
    assert lib.ju_process_frames(None, frames, frames, 2) == JU_ERR_INVALID_ARGUMENT


def test_python_binding_refuses_unequal_lists_before_any_native_call(monkeypatch):
    def native(*a, **k):
        raise AssertionError("a native call was made")

    class Lib:
        def __getattr__(self, name):
            raise AssertionError("the library was touched: " + name)

    monkeypatch.setattr(R, "_check", native)
    rt = R.Runtime.__new__(R.Runtime)
    rt._lib, rt._h = Lib(), C.c_void_p()
    f = R.JuFrame()
    with pytest.raises(ValueError):
        rt.process_frames([f, f], [f])
    with pytest.raises(ValueError):
        rt.process_frames([], [f])
    with pytest.raises(ValueError):
        rt.process_frames(iter([f]), iter([f, f, f]))


# ---- the one table of the formats (csrc/kernels.h): which values exist, which of them are deep -----------------------
LISTED = {R.FMT_I420, R.FMT_NV12, R.FMT_P010, R.FMT_I010, R.FMT_YUY2, R.FMT_UYVY, R.FMT_I422, R.FMT_P210, R.FMT_I210,
          R.FMT_I444, R.FMT_I410, R.FMT_BGR24, R.FMT_RGB24, R.FMT_RGBX, R.FMT_BGRX64, R.FMT_RGBP8, R.FMT_RGBP10,
          R.FMT_RGBP16, R.FMT_RGBPH, R.FMT_RGBPS, R.FMT_BGR96F}
DEEP = {R.FMT_P010, R.FMT_I010, R.FMT_P210, R.FMT_I210, R.FMT_I410, R.FMT_BGRX64, R.FMT_RGBP10, R.FMT_RGBP16,
        R.FMT_RGBPH, R.FMT_RGBPS, R.FMT_BGR96F}
VALUES = range(0, max(LISTED) + 2)                               # 0 (BGRX) .. one past the table's last


def test_the_items_hook_refuses_exactly_the_values_that_are_not_in_the_table(hip_library):
    """NULL buffers: a listed format gets as far as the buffers ("null"), an unlisted one is refused before them."""
    lib = hip_library
    one, zero = (C.c_int * 1), (C.c_ssize_t * 1)(0)
    for v in VALUES:
        rc = lib.ju_debug_yuv_items(1, one(v), one(0), 4, 4, (C.c_void_p * 1)(), zero, (C.c_void_p * 3)(),
                                    (C.c_ssize_t * 3)())
        err = lib.ju_last_error()
        assert rc == JU_ERR_INVALID_ARGUMENT, v
        if v in LISTED:
            assert b"null" in err and b"not a" not in err, (v, err)
        else:
            assert b"not a" in err and b"format" in err and b"null" not in err, (v, err)


def test_each_single_kernel_hook_refuses_op_2_for_exactly_the_formats_that_are_not_deep(hip_library):
    """Op 2 (encode from the f16 state) with NULL buffers: a deep format the hook admits gets as far as the buffers; a
    format it admits that is not deep is refused for the op, any other value as not the hook's kind of format.
    ju_debug_yuv admits I420 and NV12 alone, neither deep: it has no op 2 at all."""
    lib = hip_library
    planes, strides = (C.c_void_p * 3)(), (C.c_ssize_t * 3)()
    families = {"ju_debug_yuv": {R.FMT_I420, R.FMT_NV12}, "ju_debug_yuv10": {R.FMT_P010, R.FMT_I010},
                "ju_debug_yuv_sampled": {R.FMT_YUY2, R.FMT_UYVY, R.FMT_I422, R.FMT_P210, R.FMT_I210, R.FMT_I444,
                                         R.FMT_I410},
                "ju_debug_rgb": {f for f in LISTED if f >= R.FMT_BGR24}}
    assert set().union(*families.values()) == LISTED
    for name, family in families.items():
        for v in VALUES:
            cs = () if name == "ju_debug_rgb" else (0,)
            rc = getattr(lib, name)(2, v, *cs, 4, 4, None, 0, planes, strides)
            err = lib.ju_last_error()
            assert rc == JU_ERR_INVALID_ARGUMENT, (name, v)
            assert (b"null" in err) == (v in family and v in DEEP), (name, v, err)
            if name == "ju_debug_yuv":
                assert b"direction" in err, (v, err)
            elif v not in family:
                assert b"not a" in err and b"format" in err, (name, v, err)
            elif v not in DEEP:
                assert b"op 2" in err, (name, v, err)
