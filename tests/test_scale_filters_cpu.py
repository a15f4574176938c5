"""The scalers' filters without a GPU (docs/source_stage.md "Filters"): the numpy definition of the two cubic filters
(tests/scale_filter_reference.py) against its own invariants and widths, the C++ table builder word for word
(ju_debug_scale op 4), a float64 evaluation of the same kernels under a derived bound, Pillow's BICUBIC; the limits'
message in C and in Python; the header and the bindings."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import output_reference as O
import scale_filter_reference as F
import source_reference as S
from joshupscale_amd import runtime as R
from test_output_cpu import p_of
from test_source_cpu import noise, smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AXES = [(1080, 2160), (1080, 720), (1080, 270), (272, 270), (480, 3840), (30, 16), (17, 16), (8, 16), (16, 128), (128, 16),
        (2, 32), (7, 5), (5, 7), (64, 9), (3, 2), (2, 3), (100, 37), (8192, 1024), (1000, 999), (16384, 2048)]
CUBIC = pytest.mark.parametrize("filt", F.CUBIC, ids=lambda f: F.NAMES[f])
TOPS = pytest.mark.parametrize("top", [255, 65535])


def scale_of(top):
    return F.scale8 if top == 255 else F.scale16


def samples(top, h, w, seed=11):
    """Full-range noise: uint8 BGRX for the 8-bit path, int64 P for the 16-bit one."""
    rng = np.random.default_rng(seed)
    if top == 255:
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return rng.integers(0, 65536, (h, w, 4), dtype=np.int64)


# ---- tables ----------------------------------------------------------------------------------------------------------------
@CUBIC
@pytest.mark.parametrize("n,m", AXES)
def test_every_row_sums_to_4096_within_33_taps_and_the_absolute_sum(n, m, filt):
    start, count, taps = F.axis_table(n, m, filt)                 # (asserts S > 0 and sum |q| <= 6144 per row itself)
    assert (taps.sum(1) == 4096).all()
    assert 1 <= count.min() and count.max() <= F.MAX_TAPS
    assert int(np.abs(taps).sum(1).max()) <= F.ABS_SUM_MAX
    assert (start >= 0).all() and (start + count <= n).all()
    # what the signed kernels' tile span relies on: a row that lost a zero tap at one end starts or ends one index out of
    # order at the most (the triangle's rows are in order)
    assert int((np.maximum.accumulate(start) - start).max()) <= 1
    assert int((np.maximum.accumulate(start + count) - (start + count)).max()) <= 1
    big = 2 * max(n, m)
    for d in range(m):
        assert (taps[d, count[d]:] == 0).all()
        # one contiguous run: every tap of it lies inside the support, its two ends are not zero, and the raw weights of
        # the run sum above zero
        s = np.arange(start[d], start[d] + count[d], dtype=np.int64)
        u = np.abs((2 * s + 1) * m - (2 * d + 1) * n)
        assert (u < 2 * big).all()
        w = F.raw_weight(filt, u, big)
        assert w[0] != 0 and w[-1] != 0 and int(w.sum()) > 0
        for outside in (start[d] - 1, start[d] + count[d]):       # ... and no index next to it carries weight
            if 0 <= outside < n:
                uo = abs((2 * outside + 1) * m - (2 * d + 1) * n)
                assert uo >= 2 * big or int(F.raw_weight(filt, np.array([uo]), big)[0]) == 0


def test_the_measured_absolute_sums():
    """A <= 5192 (Catmull-Rom) and <= 4668 (Mitchell) over the list: well under the 6144 the kernels' widths rest on."""
    worst = {f: max(F.abs_sum(F.axis_table(n, m, f)) for n, m in AXES) for f in F.CUBIC}
    print(worst)
    assert worst[F.CATMULL_ROM] <= 5192 and worst[F.MITCHELL] <= 4668
    assert all(4096 < a <= F.ABS_SUM_MAX for a in worst.values())            # (some tap IS negative)
    assert max(int(F.axis_table(n, m, f)[1].max()) for n, m in AXES for f in F.CUBIC) <= 32


def c_table(lib, n, m, filt):
    start, count = np.zeros(m, np.int32), np.zeros(m, np.int32)
    taps = np.zeros((m, F.MAX_TAPS), np.int16)
    rc = lib.ju_debug_scale(4, filt, None, 0, m, 0, None, 0, n, 0, start.ctypes.data, count.ctypes.data, taps.ctypes.data)
    assert rc == 0, lib.ju_last_error()
    return start, count, taps


@pytest.mark.parametrize("filt", F.FILTERS, ids=lambda f: F.NAMES[f])
def test_the_cpp_builder_equals_the_numpy_tables_word_for_word(hip_library, filt):
    for n, m in AXES:
        if n > F.down_max(filt) * m or m > F.RATIO_MAX * n:
            continue
        start, count, taps = c_table(hip_library, n, m, filt)
        want = F.axis_table(n, m, filt) if filt else S.axis_table(n, m)
        assert np.array_equal(start, want[0]) and np.array_equal(count, want[1]), (n, m)
        assert np.array_equal(taps, want[2]), (n, m)
    # beyond the filter's factor the builder refuses
    n, m = (129, 16) if filt else (257, 16)
    start, count, taps = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, F.MAX_TAPS), np.int16)
    rc = hip_library.ju_debug_scale(4, filt, None, 0, m, 0, None, 0, n, 0, start.ctypes.data, count.ctypes.data, taps.ctypes.data)
    assert rc == 1 and b"beyond a factor of " + str(F.down_max(filt)).encode() in hip_library.ju_last_error()


def test_every_axis_of_the_list_is_built_by_cpp_for_a_cubic_filter():
    assert all(n <= F.CUBIC_DOWN_MAX * m and m <= F.RATIO_MAX * n for n, m in AXES)


# ---- properties ------------------------------------------------------------------------------------------------------------
@TOPS
def test_catmull_rom_at_equal_sizes_is_the_identity_and_mitchell_is_not(top):
    for (h, w) in [(16, 24), (2, 2), (7, 301)]:
        x = samples(top, h, w)
        out = scale_of(top)(x, h, w, F.CATMULL_ROM)
        assert np.array_equal(out[..., :3], x[..., :3]) and (out[..., 3] == 0).all()
        assert int(F.axis_table(h, h, F.CATMULL_ROM)[1].max()) == 1
    x = samples(top, 16, 24)
    out = scale_of(top)(x, 16, 24, F.MITCHELL)
    assert not np.array_equal(out[..., :3], x[..., :3]) and int(F.axis_table(16, 16, F.MITCHELL)[1].max()) == 3


@TOPS
@CUBIC
def test_constant_frames_stay_constant(filt, top):
    for c in (0, 1, top // 2, top - 1, top):
        x = np.full((9, 11, 4), c, np.uint8 if top == 255 else np.int64)
        out = scale_of(top)(x, 23, 7, filt)
        assert (out[..., :3] == c).all() and (out[..., 3] == 0).all(), c


@TOPS
@CUBIC
def test_the_widths_hold_on_full_range_noise(filt, top):
    """scale8 / scale16 assert |vertical sum| < 2^21 / 2^29 and |whole sum| < 2^34 / 2^42 themselves; the 8-bit whole sum
    does need more than 32 bits."""
    most = 0
    for (src, dst) in [((30, 46), (16, 24)), ((8, 12), (16, 24)), ((64, 96), (8, 12)), ((17, 23), (16, 24)), ((40, 60), (80, 120))]:
        x = samples(top, *src)
        scale_of(top)(x, *dst, filt)
        v, acc = F.sums(x, *dst, filt)
        most = max(most, int(np.abs(acc).max()))
        assert int(np.abs(v).max()) <= top * F.ABS_SUM_MAX and int(np.abs(acc).max()) <= top * F.ABS_SUM_MAX ** 2 + (1 << 23)
    assert top * F.ABS_SUM_MAX < 1 << (21 if top == 255 else 29)
    assert top * F.ABS_SUM_MAX ** 2 + (1 << 23) < 1 << (34 if top == 255 else 42)
    if top == 255:
        assert most >= 1 << 32, most                              # (why the horizontal pass is 64 bits wide)


@TOPS
@CUBIC
def test_a_step_edge_overshoots_both_ways_and_is_clamped(filt, top):
    x = F.step_edges(12, 18, top, np.uint8 if top == 255 else np.int64)
    _, acc = F.sums(x, 24, 36, filt)
    raw = acc >> 24
    assert int(raw.min()) < 0 and int(raw.max()) > top            # (the clamp is exercised, at both ends)
    out = scale_of(top)(x, 24, 36, filt)
    assert int(out.min()) == 0 and int(out[..., :3].max()) == top
    assert np.array_equal(out[..., :3], np.clip(raw, 0, top))


# ---- against float64 -------------------------------------------------------------------------------------------------------
@TOPS
@CUBIC
@pytest.mark.parametrize("src,dst", [((120, 192), (90, 144)), ((120, 192), (180, 288)), ((120, 192), (64, 100)),
                                     ((30, 46), (16, 24)), ((17, 23), (16, 24)), ((8, 12), (16, 24)), ((64, 96), (8, 12)),
                                     ((16, 24), (16, 24))])
def test_the_integer_scaler_against_the_same_filter_in_float64(src, dst, filt, top):
    """|integer result - clamped float64 value| <= 0.5 + top (A_x / 4096 (Ty - 1) + B_y (Tx - 1)) / 4096
    (scale_filter_reference.float_bound; docs/source_stage.md "Filters")."""
    bound = F.float_bound(src, dst, filt, top)
    for frame in (smooth(*src), noise(*src)):
        x = frame if top == 255 else p_of(frame)
        got = scale_of(top)(x, *dst, filt)[..., :3].astype(np.float64)
        want = F.scale_float(x, *dst, filt, top)
        worst = float(np.abs(got - want).max())
        print(f"{F.NAMES[filt]} {src} -> {dst} top {top}: |int - float64| max {worst:.4f}, bound {bound:.4f}")
        assert worst <= bound + 1e-6


# ---- against Pillow --------------------------------------------------------------------------------------------------------
def mid_noise(h, w):
    return np.random.default_rng(23).integers(64, 192, (h, w, 4), dtype=np.uint8)


@pytest.mark.parametrize("src,dst", [((120, 192), (90, 144)), ((120, 192), (180, 288)), ((120, 192), (64, 100)),
                                     ((120, 192), (240, 384)), ((272, 480), (270, 480)), ((30, 46), (16, 24)),
                                     ((17, 23), (16, 24)), ((8, 12), (16, 24))])
def test_catmull_rom_against_pillows_bicubic_resize(src, dst):
    """Pillow's BICUBIC is the same kernel (a = -0.5) with its own coefficient precision and the intermediate image
    clipped to 8 bits, so equality is not expected.  Measured with Pillow 12.2.0: 1 LSB at the most on every case below;
    asserted: that plus 1 LSB, as for the triangle.  (Full-range noise is left out on purpose: the 8-bit clip between
    Pillow's passes then differs by up to 21.)"""
    Image = pytest.importorskip("PIL.Image")
    for name, x in (("smooth", smooth(*src)), ("noise 64..191", mid_noise(*src))):
        got = F.scale8(x, *dst, F.CATMULL_ROM)[..., :3].astype(np.int64)
        rgb = np.ascontiguousarray(x[..., 2::-1])
        pil = np.asarray(Image.fromarray(rgb).resize((dst[1], dst[0]), Image.BICUBIC))[..., ::-1].astype(np.int64)
        worst = int(np.abs(got - pil).max())
        print(f"{src} -> {dst} {name}: max |ours - Pillow| = {worst}")
        assert worst <= 2


# ---- limits and messages ---------------------------------------------------------------------------------------------------
def c_limit(lib, op, filt, a, b):
    """op 2: source size a for a model input b; op 3: output size a for a model output b; (w, h) each."""
    if op == 2:
        rc = lib.ju_debug_scale(2, filt, None, 0, b[0], b[1], None, 0, a[0], a[1], None, None, None)
    else:
        rc = lib.ju_debug_scale(3, filt, None, 0, a[0], a[1], None, 0, b[0], b[1], None, None, None)
    return rc, lib.ju_last_error().decode() if rc else ""


def test_the_limits_and_their_message_match_between_c_and_python(hip_library):
    lib = hip_library
    inp, outp = (48, 30), (192, 120)
    for filt in F.CUBIC:
        # the source: 8 : 1 and 1 : 16 pass, 9 : 1 does not and names the 8
        for size in [(8 * 48, 8 * 30), (3, 2), (48, 30), (72, 48)]:
            assert R.source_size_problem(*size, *inp, filter=filt) == "" and c_limit(lib, 2, filt, size, inp) == (0, "")
        for size in [(9 * 48, 30), (48, 9 * 30), (8 * 48 + 1, 30), (2, 2), (1, 30), (8193, 30)]:
            text = R.source_size_problem(*size, *inp, filter=filt)
            assert text.startswith(f"source size {size[0]}x{size[1]}: ") and "at most 8 times" in text and "48x30" in text
            assert c_limit(lib, 2, filt, size, inp) == (1, "std::invalid_argument: ju_set_source_size: " + text)
        # the output: 1 : 8 down and 16 : 1 up pass, 1 : 9 does not
        for size in [(24, 15), (16 * 192, 16 * 120), (192, 120), (144, 90)]:
            assert R.output_size_problem(*size, *outp, filt) == "" and c_limit(lib, 3, filt, size, outp) == (0, "")
        for size in [(21, 120), (192, 13), (23, 15), (16 * 192 + 1, 120), (1, 120)]:
            text = R.output_size_problem(*size, *outp, filt)
            assert text.startswith(f"output size {size[0]}x{size[1]}: ") and "at least an 8th" in text and "192x120" in text
            assert c_limit(lib, 3, filt, size, outp) == (1, "std::invalid_argument: ju_set_output_size: " + text)
    # filters 1 and 4 (and others) are refused whatever the size, in both layers, with one text that lists the filters
    for filt in (1, 4, -1, 99):
        text = R.source_size_problem(72, 48, *inp, filter=filt)
        assert "filter" in text and "JU_SCALE_CATMULL_ROM = 2" in text and "JU_SCALE_MITCHELL = 3" in text
        assert text == R.output_size_problem(144, 90, *outp, filt) == R.scale_filter_problem(filt)
        assert c_limit(lib, 2, filt, (72, 48), inp) == (1, "std::invalid_argument: ju_set_source_size: " + text)
        assert c_limit(lib, 3, filt, (144, 90), outp) == (1, "std::invalid_argument: ju_set_output_size: " + text)
    # the triangle keeps its factor of 16 both ways and its words
    assert R.source_size_problem(16 * 48, 16 * 30, *inp) == "" == R.source_size_problem(16 * 48, 16 * 30, *inp, filter=0)
    assert c_limit(lib, 2, 0, (16 * 48, 16 * 30), inp) == (0, "") and c_limit(lib, 3, 0, (12, 8), outp) == (0, "")
    text = R.source_size_problem(16 * 48 + 1, 30, *inp)
    assert "within a factor of 16 of" in text and c_limit(lib, 2, 0, (16 * 48 + 1, 30), inp)[1].endswith(text)
    text = R.output_size_problem(11, 120, *outp)
    assert "within a factor of 16 of" in text and c_limit(lib, 3, 0, (11, 120), outp)[1].endswith(text)
    # the numpy definition refuses what the setters refuse
    with pytest.raises(AssertionError):
        F.axis_table.__wrapped__(129, 16, F.CATMULL_ROM)


# ---- header and bindings ---------------------------------------------------------------------------------------------------
def test_the_enum_the_bindings_and_the_hook(hip_library, product_library):
    header = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    for name, value in (("TRIANGLE", 0), ("CATMULL_ROM", 2), ("MITCHELL", 3)):
        assert re.search(r"JU_SCALE_" + name + r"\s*=\s*" + str(value) + r"\b", header)
        assert getattr(R, "SCALE_" + name) == value == getattr(F, name)
    assert not re.search(r"JU_SCALE_\w+\s*=\s*1\b", header) and "reserved" in header
    assert (R.SOURCE_RATIO_MAX, R.OUTPUT_RATIO_MAX, R.CUBIC_DOWN_MAX) == (F.RATIO_MAX, O.RATIO_MAX, F.CUBIC_DOWN_MAX)
    assert re.search(r"JU_API\s+int\s+ju_debug_scale\s*\(", test_header) and "ju_debug_scale" not in header
    assert "ju_debug_scale" in R.HOOK_SYMBOLS and "ju_debug_scale" not in R.PRODUCT_SYMBOLS
    assert hasattr(hip_library, "ju_debug_scale") and not hasattr(product_library, "ju_debug_scale")
    for stat in ("source_filter", "output_filter"):
        assert f'"{stat}"' in header and f'"{stat}"' in R.Runtime.stat.__doc__
    import inspect
    assert list(inspect.signature(R.source_size_problem).parameters)[-1] == "filter"
    assert inspect.signature(R.source_size_problem).parameters["filter"].default == R.SCALE_TRIANGLE
    for cls in (R.Runtime, R.Session):
        for name in ("set_source_size", "set_output_size"):
            assert inspect.signature(getattr(cls, name)).parameters["filter"].default == R.SCALE_TRIANGLE
