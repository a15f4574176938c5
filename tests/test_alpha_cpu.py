"""The alpha channel's definition (tests/alpha_reference.py) held to its own properties, the limits' message held
between the C++ layer and its Python twin, and the declared surface (CPU; docs/alpha.md)."""

import os
import re

import numpy as np
import pytest

import alpha_reference as A
import output_reference as OUT
import scale_filter_reference as F
from helpers import ROOT
from joshupscale_amd import runtime as R

# (source, destination) sizes as (H, W): the shapes of tests/test_gpu_alpha.py
SHAPES = [((30, 48), (120, 192)), ((16, 24), (16, 24)), ((17, 23), (16, 24)), ((16, 24), (7, 50)), ((64, 1024), (4, 64)),
          ((64, 512), (8, 64)), ((4, 6), (64, 96)), ((16, 24), (64, 96))]


def filters_of(src, dst):
    """(64, 1024) -> (4, 64) is 16 : 1: the triangle only."""
    return [f for f in F.FILTERS if src[0] <= F.down_max(f) * dst[0] and src[1] <= F.down_max(f) * dst[1]]


def random_codes(kind, hw, seed):
    return np.random.default_rng(seed).integers(0, A.TOP[kind] + 1, hw, dtype=np.int64)


def test_the_plane_and_the_codes_round_trip_in_all_three_widths():
    for kind in ("byte", "word", "bits"):
        codes = np.arange(A.TOP[kind] + 1, dtype=np.int64)[None, :]
        plane = A.plane(kind, codes)
        assert plane.min() == 0 and plane.max() == 65535          # 257 * 255 = 21845 * 3 = 65535
        assert (A.code(kind, plane) == codes).all()
    assert (A.plane("none", None, 3, 5) == 65535).all() and A.plane("none", None, 3, 5).shape == (3, 5)
    # the codes round to nearest: the midpoints between two codes go up
    assert A.code("byte", np.array([128, 129, 65535 - 129])).tolist() == [0, 1, 254]
    assert A.code("bits", np.array([10922, 10923, 54612, 54613])).tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("kind", ["byte", "word", "bits"])
def test_equal_sizes_give_the_alpha_back_code_for_code(kind):
    for hw in [(16, 24), (17, 23), (30, 48)]:
        codes = random_codes(kind, hw, 7)
        for filt in (F.TRIANGLE, F.CATMULL_ROM):
            assert (A.alpha(A.SOURCE, kind, codes, hw, kind, hw, filt) == codes).all()


def test_opaque_in_gives_opaque_out_and_equals_opaque_mode():
    for src, dst in SHAPES:
        for filt in filters_of(src, dst):
            for kind in ("byte", "word", "bits"):
                top = np.full(src, A.TOP[kind], np.int64)
                want = A.alpha(A.OPAQUE, kind, None, src, kind, dst)
                assert (want == A.TOP[kind]).all() and want.shape == dst
                assert (A.alpha(A.SOURCE, kind, top, src, kind, dst, filt) == want).all()
                # an input without a slot is opaque
                assert (A.alpha(A.SOURCE, "none", None, src, kind, dst, filt) == want).all()
    assert A.alpha(A.SOURCE, "byte", np.zeros((4, 4), np.int64), (4, 4), "none", (16, 16)) is None
    assert (A.alpha(A.ZERO, "byte", None, (4, 4), "word", (16, 16)) == 0).all()


def test_the_sums_stay_inside_the_kernels_words_at_every_shape():
    for src, dst in SHAPES:
        for filt in filters_of(src, dst):
            for plane in (A.checkerboard(*src), np.full(src, 65535, np.int64),
                          A.plane("word", random_codes("word", src, 11))):
                v, acc = A.sums(plane, *dst, filt)
                if filt == F.TRIANGLE:
                    assert 0 <= v.min() and v.max() <= 65535 * 4096 < 1 << 28
                    assert 0 <= acc.min() and acc.max() < 1 << 40
                else:
                    assert np.abs(v).max() <= 65535 * F.ABS_SUM_MAX < 1 << 29   # one signed LDS word
                    assert np.abs(acc).max() < 1 << 42                          # the signed 64-bit horizontal sum


def test_the_triangle_is_output_references_scale16_on_one_channel():
    for src, dst in [((30, 48), (120, 192)), ((17, 23), (16, 24)), ((64, 1024), (4, 64))]:
        plane = A.plane("word", random_codes("word", src, 3))
        want = OUT.scale16(np.repeat(plane[..., None], 3, axis=2), *dst)[..., 0]
        assert (A.scale(plane, *dst, F.TRIANGLE) == want).all()
        for filt in F.CUBIC:
            if filt in filters_of(src, dst):
                assert (A.scale(plane, *dst, filt) == F.scale16(np.repeat(plane[..., None], 3, axis=2), *dst, filt)[..., 0]).all()


def test_the_checkerboard_leaves_the_range_at_both_ends_under_catmull_rom():
    """What makes the GPU case exercise the clamp: without it the shifted sums of 16x24 -> 64x96 are below 0 and above
    65535."""
    board = A.checkerboard(16, 24)
    _, acc = A.sums(board, 64, 96, F.CATMULL_ROM)
    assert (acc >> 24).min() < 0 and (acc >> 24).max() > 65535
    out = A.scale(board, 64, 96, F.CATMULL_ROM)
    assert out.min() == 0 and out.max() == 65535


def c_problem(lib, mode, filt, in_size, out_size):
    rc = lib.ju_debug_alpha_problem(mode, filt, in_size[0], in_size[1], out_size[0], out_size[1])
    return rc, (lib.ju_last_error().decode() if rc else "")


def test_the_limits_and_their_message_match_between_c_and_python(hip_library):
    lib = hip_library
    ok = [(A.ZERO, 0, (48, 30), (192, 120)), (A.OPAQUE, 3, (48, 30), (192, 120)), (A.SOURCE, 0, (48, 30), (192, 120)),
          (A.SOURCE, 2, (96, 60), (144, 90)), (A.SOURCE, 0, (768, 480), (48, 30)), (A.SOURCE, 3, (384, 240), (48, 30)),
          (A.SOURCE, 0, (2, 2), (32, 32)), (A.SOURCE, 0, (16384, 1024), (1024, 16384)),
          # the sizes do not count where alpha is not scaled
          (A.ZERO, 0, (768, 480), (12, 8)), (A.OPAQUE, 2, (768, 480), (12, 8))]
    for mode, filt, ins, outs in ok:
        assert R.alpha_problem(mode, filt, *ins, *outs) == "" and not A.problem(mode, filt, *ins, *outs)
        assert c_problem(lib, mode, filt, ins, outs) == (0, "")
    bad = [(A.SOURCE, 0, (768, 480), (12, 8)),         # 16 : 1 in and 1 : 16 out: 64 : 1
           (A.SOURCE, 0, (769, 30), (48, 120)), (A.SOURCE, 2, (385, 30), (48, 120)), (A.SOURCE, 3, (48, 241), (48, 30)),
           (A.SOURCE, 0, (48, 30), (769, 120)), (A.SOURCE, 0, (1, 30), (16, 120)), (A.SOURCE, 0, (16385, 30), (16384, 120)),
           (A.SOURCE, 0, (48, 30), (48, 1))]
    for mode, filt, ins, outs in bad:
        text = R.alpha_problem(mode, filt, *ins, *outs)
        assert A.problem(mode, filt, *ins, *outs)
        assert "alpha" in text and f"{ins[0]}x{ins[1]}" in text and f"{outs[0]}x{outs[1]}" in text
        assert f"at most {F.down_max(filt)} times the output" in text
        assert c_problem(lib, mode, filt, ins, outs) == (1, "std::invalid_argument: ju_set_alpha: " + text)
    for mode in (-1, 3, 99):
        text = R.alpha_problem(mode, 0, 48, 30, 192, 120)
        assert "JU_ALPHA_OPAQUE = 1" in text and A.problem(mode, 0, 48, 30, 192, 120)
        assert c_problem(lib, mode, 0, (48, 30), (192, 120)) == (1, "std::invalid_argument: ju_set_alpha: " + text)
    # the filter is checked in every mode, with the scalers' own text
    for mode in (A.ZERO, A.OPAQUE, A.SOURCE):
        for filt in (1, 4, -1):
            text = R.alpha_problem(mode, filt, 48, 30, 192, 120)
            assert text == R.scale_filter_problem(filt) and A.problem(mode, filt, 48, 30, 192, 120)
            assert c_problem(lib, mode, filt, (48, 30), (192, 120)) == (1, "std::invalid_argument: ju_set_alpha: " + text)


def test_the_declared_surface(hip_library, product_library):
    def declared(header):
        text = open(os.path.join(ROOT, "include", header)).read()
        return set(re.findall(r"JU_API\s+[\w\s\*]+?\b(ju_\w+)\s*\(", text))
    for name in ("ju_set_alpha", "ju_get_alpha"):
        assert name in declared("joshupscale_amd.h") and name in R.PRODUCT_SYMBOLS and name not in R.HOOK_SYMBOLS
        assert hasattr(product_library, name) and hasattr(hip_library, name)
    for name in ("ju_debug_alpha_scale", "ju_debug_alpha_fill", "ju_debug_alpha_problem"):
        assert name in declared("joshupscale_amd_test.h") and name not in declared("joshupscale_amd.h")
        assert name in R.HOOK_SYMBOLS and name not in R.PRODUCT_SYMBOLS
        assert hasattr(hip_library, name) and not hasattr(product_library, name)
    header = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    assert "JU_ALPHA_ZERO = 0, JU_ALPHA_OPAQUE = 1, JU_ALPHA_SOURCE = 2" in header
    assert (R.ALPHA_ZERO, R.ALPHA_OPAQUE, R.ALPHA_SOURCE) == (A.ZERO, A.OPAQUE, A.SOURCE) == (0, 1, 2)
    assert "without alpha" not in header
    for cls in (R.Runtime, R.Session):
        assert callable(cls.set_alpha) and callable(cls.get_alpha)
    # the C++ plugin surface does not change
    core = open(os.path.join(ROOT, "include", "JoshUpscale", "core.h")).read()
    assert "alpha" not in core.lower()
    # no device: the hooks refuse before any device call, and the setters refuse a NULL runtime
    assert hip_library.ju_set_alpha(None, 0, 0) == 1 and b"runtime is NULL" in hip_library.ju_last_error()
    assert hip_library.ju_get_alpha(None, None, None) == 1
    assert hip_library.ju_debug_alpha_fill(0, None, 16, 0, 4) == 1 and b"1 .. 32768" in hip_library.ju_last_error()
    assert hip_library.ju_debug_alpha_scale(0, 0, 1, None, 16, 4, 4, None, 16, 4, 4) == 1
    assert b"unknown filter 1" in hip_library.ju_last_error()
