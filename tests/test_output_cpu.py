"""The output stage without a GPU: the numpy definition of the 16-bit scaler (tests/output_reference.py;
docs/output_stage.md) against its own bounds and invariants, a float64 evaluation of the same filter and the 8-bit
scaler; the new entry points; the limits' message in C and in Python."""

import os
import re

import numpy as np
import pytest

import output_reference as O
import source_reference as S
from joshupscale_amd import runtime as R
from test_source_cpu import noise, smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (model output, output size) as (H, W): the small model's output to the sizes of the GPU tests, 1080p to 720p
SIZES = [((120, 192), (90, 144)), ((120, 192), (180, 288)), ((120, 192), (64, 100)), ((120, 192), (240, 384)),
         ((1080, 1920), (720, 1280))]


def p_of(frame):
    """A 16-bit test frame of an 8-bit one with all 16 bits in use: 257 u8 plus a pattern below 257 (never above 65535)."""
    h, w = frame.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    low = ((x * 7 + y * 13) % 257)[..., None]
    return np.minimum(frame[..., :3].astype(np.int64) * 257 + low, 65535)


def test_the_sums_stay_below_2_28_and_2_40_at_the_ratio_limit():
    """All-65535 input, 16 : 1 on both axes (33-tap rows): the vertical sum is 65535 * 4096, the whole sum
    65535 * 2^24 + 2^23; scale16 asserts both bounds itself."""
    assert 65535 * 4096 < 1 << 28 and 65535 * 4096 * 4096 + (1 << 23) < 1 << 40
    p = np.full((64, 96, 3), 65535, np.int64)
    vertical, whole = O.scale16_sums(p, 4, 6)
    assert vertical == 65535 * 4096 < 1 << 28
    assert whole == 65535 * 4096 * 4096 + (1 << 23) < 1 << 40 and whole >= 1 << 32      # (more than 32 bits: why 64 are needed)
    assert int(S.axis_table(64, 4)[1].max()) >= 32
    out = O.scale16(p, 4, 6)
    assert (out[..., :3] == 65535).all() and (out[..., 3] == 0).all() and out.dtype == np.uint16


def test_equal_sizes_are_the_identity():
    for (h, w) in [(16, 24), (120, 192), (2, 2), (7, 301)]:
        p = np.random.default_rng(h).integers(0, 65536, (h, w, 4))
        out = O.scale16(p, h, w)
        assert np.array_equal(out[..., :3], p[..., :3]) and (out[..., 3] == 0).all()


@pytest.mark.parametrize("src,dst", SIZES)
def test_constant_frames_stay_constant(src, dst):
    """Every row of taps sums to 4096: c * 2^24 + 2^23 >> 24 = c."""
    for c in (0, 1, 255, 32768, 65534, 65535):
        out = O.scale16(np.full(src + (3,), c, np.int64), *dst)
        assert (out[..., :3] == c).all() and (out[..., 3] == 0).all(), c


@pytest.mark.parametrize("src,dst", SIZES[:4] + [((120, 192), (120, 192)), ((64, 96), (4, 6)), ((4, 6), (64, 96))])
def test_the_integer_scaler_against_the_same_filter_in_float64(src, dst):
    """|scale16 - float64 value| <= 0.5 + 65535 ((Ty - 1) + (Tx - 1)) / 4096, T the most taps of an axis' rows: the bound
    argument of docs/source_stage.md (test_source_cpu.py) with 16-bit samples in place of 8-bit ones."""
    for frame in (smooth(*src), noise(*src)):
        p = p_of(frame)
        got = O.scale16(p, *dst)[..., :3].astype(np.float64)
        want = S.scale_float(p, *dst)
        ty, tx = int(S.axis_table(src[0], dst[0])[1].max()), int(S.axis_table(src[1], dst[1])[1].max())
        bound = 0.5 + 65535.0 * ((ty - 1) + (tx - 1)) / 4096.0
        worst = float(np.abs(got - want).max())
        print(f"{src} -> {dst}: |int - float64| max {worst:.4f}, bound {bound:.4f} (taps {ty}, {tx})")
        assert worst <= bound + 1e-6


# scale16(257 u8) >> 8 against scale(u8).  With A = sum qy qx u8 and x = A / 2^24 (0 .. 255) the first is
# floor(x + x / 256 + 1 / 512) and the second floor(x + 1 / 2); both lie in {floor(x), floor(x) + 1}: they differ by at most
# 1.  Measured on the smooth and the noise clip at the four sizes below: 1 at every size (0 at the identity).
MEASURED_16_AGAINST_8 = 1


@pytest.mark.parametrize("src,dst", SIZES[:4] + [((120, 192), (120, 192))])
def test_the_16_bit_path_of_an_8_bit_frame_lies_within_one_of_the_8_bit_path(src, dst):
    for name, frame in (("smooth", smooth(*src)), ("noise", noise(*src))):
        deep = O.scale16(frame.astype(np.int64) * 257, *dst)[..., :3].astype(np.int64) >> 8
        plain = O.scale8(frame, *dst)[..., :3].astype(np.int64)
        worst = int(np.abs(deep - plain).max())
        print(f"{src} -> {dst} {name}: max |scale16(257 u8) >> 8 - scale(u8)| = {worst}")
        assert worst <= MEASURED_16_AGAINST_8
        if src == dst:
            assert worst == 0


def test_the_samples_of_a_16_bit_frame():
    p = np.array([0, 1, 63, 64, 257, 32767, 32768, 65534, 65535], np.int64)
    assert np.array_equal(O.samples_from_p("w16", p), p.astype(np.uint16))
    assert np.array_equal(O.samples_from_p("w10", p), (p >> 6).astype(np.uint16)) and O.samples_from_p("w10", p)[-1] == 1023
    unit = O.samples_from_p("s", p)
    assert unit.dtype == np.float32 and unit[0] == 0.0 and unit[-1] == 1.0
    assert np.abs(unit.astype(np.float64) - p / 65535.0).max() <= 2.0 ** -25          # (half an ulp below 1)
    half = O.samples_from_p("h", p)
    assert half.dtype == np.float16 and half[0] == 0.0 and half[-1] == 1.0
    f255 = O.samples_from_p("f255", p)
    assert f255.dtype == np.float32 and f255[-1] == 255.0 and f255[4] == 1.0
    # P = 257 u8 gives the samples of the 8-bit frame's encode, for the word kinds and the 0 .. 255 floats
    u8 = np.arange(256, dtype=np.uint8)
    for kind in ("w16", "w10", "f255"):
        assert np.array_equal(O.samples_from_p(kind, u8.astype(np.int64) * 257), O.G.samples_from_u8(kind, u8)), kind
    with pytest.raises(ValueError):
        O.encode16(R.FMT_NV12, 0, np.zeros((2, 2, 3), np.int64))


def test_which_path_a_format_takes():
    for fmt in O.DEEP:
        assert O.takes_16_bit_path(fmt, True, False)
        assert not O.takes_16_bit_path(fmt, False, False) and not O.takes_16_bit_path(fmt, True, True)
    for fmt in (R.FMT_BGRX, R.FMT_NV12, R.FMT_I420, R.FMT_YUY2, R.FMT_RGB24, R.FMT_RGBP8):
        assert not O.takes_16_bit_path(fmt, True, False)
    assert len(O.DEEP) == 11


def test_new_entry_points_are_declared_and_exported(hip_library, product_library):
    header = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    for name in ("ju_set_output_size", "ju_get_output_size"):
        assert re.search(r"JU_API\s+int\s+" + name + r"\s*\(", header)
        assert name in R.PRODUCT_SYMBOLS and name not in R.HOOK_SYMBOLS
        assert hasattr(product_library, name) and hasattr(hip_library, name)
    assert re.search(r"JU_API\s+int\s+ju_debug_output\s*\(", test_header) and "ju_debug_output" not in header
    assert "ju_debug_output" in R.HOOK_SYMBOLS and "ju_debug_output" not in R.PRODUCT_SYMBOLS
    assert hasattr(hip_library, "ju_debug_output") and not hasattr(product_library, "ju_debug_output")
    for name in ("set_output_size", "get_output_size"):
        assert callable(getattr(R.Runtime, name)) and callable(getattr(R.Session, name))
    assert "a scaler on the output side" not in header


def c_limit_message(lib, ow, oh, mw, mh, filt=0):
    rc = lib.ju_debug_output(2, None, ow, oh, None, mw, mh, filt, 0, None, None)
    return rc, lib.ju_last_error().decode() if rc else ""


def test_the_limits_and_their_message_match_between_c_and_python(hip_library):
    assert (O.AXIS_MIN, O.AXIS_MAX, O.RATIO_MAX) == (R.OUTPUT_AXIS_MIN, R.OUTPUT_AXIS_MAX, R.OUTPUT_RATIO_MAX)
    model = (192, 120)
    good = [(192, 120), (144, 90), (288, 180), (3072, 1920), (12, 8), (100, 64), (3071, 9)]
    bad = [(3073, 120), (192, 1921), (11, 120), (192, 7), (1, 120), (192, 1), (0, 120), (192, 0), (10 ** 6, 120)]
    for (ow, oh) in good:
        assert R.output_size_problem(ow, oh, *model) == ""
        assert c_limit_message(hip_library, ow, oh, *model) == (0, "")
    for (ow, oh) in bad:
        text = R.output_size_problem(ow, oh, *model)
        assert text.startswith(f"output size {ow}x{oh}: ") and "192x120" in text
        rc, message = c_limit_message(hip_library, ow, oh, *model)
        assert rc == 1                                                        # JU_ERR_INVALID_ARGUMENT
        assert message == "std::invalid_argument: ju_set_output_size: " + text
    # the filter
    text = R.output_size_problem(144, 90, *model, filter=1)
    assert "filter" in text
    assert c_limit_message(hip_library, 144, 90, *model, filt=1) == (1, "std::invalid_argument: ju_set_output_size: " + text)
    # a big model: the axis cap binds before the ratio does; a small one: the ratio binds both ways, the floor of 2 too
    assert R.output_size_problem(16384, 16384, 8192, 8192) == "" and R.output_size_problem(16385, 16384, 8192, 8192) != ""
    assert c_limit_message(hip_library, 16384, 16384, 8192, 8192)[0] == 0
    assert c_limit_message(hip_library, 16385, 16384, 8192, 8192)[0] == 1
    assert R.output_size_problem(2, 2, 33, 2) != "" and c_limit_message(hip_library, 2, 2, 33, 2)[0] == 1
    assert R.output_size_problem(2, 2, 32, 2) == "" and c_limit_message(hip_library, 2, 2, 32, 2)[0] == 0
