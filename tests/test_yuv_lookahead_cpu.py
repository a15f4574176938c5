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
