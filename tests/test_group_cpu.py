"""ju_process_group without a GPU: the declaration, the export, the refusals that need no runtime, and the Python
binding's own checks (which come before any native call)."""

import ctypes as C
import os
import re

import pytest

from helpers import ROOT
from joshupscale_amd import runtime as R

JU_ERR_INVALID_ARGUMENT = 1


def test_header_declares_process_group():
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    m = re.search(r"JU_API\s+int\s+ju_process_group\s*\(([^)]*)\)", text)
    assert m, "ju_process_group is not declared"
    args = " ".join(m.group(1).split())
    assert args == ("ju_runtime *const *runtimes, const ju_image *inputs, const ju_image *outputs, int count"), args
    assert "ju_process_group" in R.PRODUCT_SYMBOLS


def test_product_library_exports_process_group(product_library, hip_library):
    assert hasattr(product_library, "ju_process_group")
    assert hasattr(hip_library, "ju_process_group")


def test_null_arguments_and_negative_counts_are_refused_without_a_gpu(product_library):
    lib = product_library
    img = (R.JuImage * 2)()
    hs = (C.c_void_p * 2)()
    assert lib.ju_process_group(None, img, img, 2) == JU_ERR_INVALID_ARGUMENT
    assert b"ju_process_group" in lib.ju_last_error()
    assert lib.ju_process_group(hs, None, img, 2) == JU_ERR_INVALID_ARGUMENT
    assert lib.ju_process_group(hs, img, None, 2) == JU_ERR_INVALID_ARGUMENT
    assert lib.ju_process_group(hs, img, img, -1) == JU_ERR_INVALID_ARGUMENT
    assert lib.ju_process_group(None, None, None, -3) == JU_ERR_INVALID_ARGUMENT
    # NULL runtimes inside the array: refused, nothing to launch
    assert lib.ju_process_group(hs, img, img, 2) == JU_ERR_INVALID_ARGUMENT
    # count == 0: nothing to do
    assert lib.ju_process_group(None, None, None, 0) == 0


def test_python_binding_refuses_bad_lists_before_any_native_call(monkeypatch):
    def native(*a, **k):
        raise AssertionError("a native call was made")

    monkeypatch.setattr(R, "_check", native)
    monkeypatch.setattr(R, "load_library", native)
    img = R.JuImage()
    with pytest.raises(ValueError):
        R.process_group([object(), object()], [img], [img, img])
    with pytest.raises(ValueError):
        R.process_group([object()], [img], [])
    with pytest.raises(TypeError):
        R.process_group([object(), object()], [img, img], [img, img])
    with pytest.raises(TypeError):
        R.process_group([None], [img], [img])
    R.process_group([], [], [])  # (nothing to do, nothing called)
