"""The definition of the chroma sitings and of BT.2020 (tests/chroma_siting_reference.py), held to what it must be
without the code under test: with the left siting and the matrices 0 .. 3 it is the existing definitions byte for byte;
its resampling reproduces planes that are linear in each siting's own sample positions exactly; flat frames do not
depend on the siting; the BT.2020 integers follow from K_r and K_b; the header's values are runtime.py's."""

import os
import re
from fractions import Fraction

import numpy as np
import pytest

import chroma_siting_reference as CS
import packed10_reference as P
import yuv10_reference as T
import yuv_reference as Y
import yuv_sampled_reference as YS
from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = sorted(CS.SAMPLING)
name_of = CS.FORMAT_NAMES.get
# the half-pixel offsets (x, y) of chroma sample (0, 0) from luma sample (0, 0), in HALF luma pixels
OFFSET2 = {CS.CHROMA_LEFT: (0, 1), CS.CHROMA_CENTER: (1, 1), CS.CHROMA_TOPLEFT: (0, 0)}


def random_samples(fmt, h, w, rng):
    deep = fmt in CS.DEEP
    top, dt = (1024, np.uint16) if deep else (256, np.uint8)
    ch, cw = YS.chroma_shape(CS.SAMPLING[fmt], h, w)
    return [rng.integers(0, top, s).astype(dt) for s in ((h, w), (ch, cw), (ch, cw))]


def old_decode(fmt, cs, planes, w):
    return P.decode_planes(fmt, cs, planes, width=w) if fmt in P.YUV else YS.decode_planes(fmt, cs, planes)


def old_encode(fmt, cs, **source):
    if fmt in P.YUV:
        return P.encode_planes(fmt, cs, **source)
    if "frame16" in source:                                     # (the u16 source of the planar deep formats: P itself)
        p = np.asarray(source["frame16"])[..., :3].astype(np.int64)
        return YS.to_words(fmt, *YS.encode10(p, cs, YS.SAMPLING[fmt]))
    return YS.encode_planes(fmt, cs, **source)


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


# ---- the default is unchanged -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=name_of)
def test_left_siting_equals_the_existing_definitions(fmt):
    rng = np.random.default_rng(100 + fmt)
    for (h, w) in [(46, 30), (2, 2), (6, 34), (4, 18)]:
        for cs in range(4):
            held = CS.to_words(fmt, *random_samples(fmt, h, w, rng))
            assert np.array_equal(CS.decode_planes(fmt, cs | CS.CHROMA_LEFT, held, width=w), old_decode(fmt, cs, held, w))
            frame = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            assert same(CS.encode_planes(fmt, cs, frame=frame), old_encode(fmt, cs, frame=frame))
            if fmt not in CS.DEEP:
                continue
            state = (rng.integers(-40000, 40000, (h, w, 4)) / 65536.0).astype(np.float16)   # (beyond +-0.5: saturates)
            assert same(CS.encode_planes(fmt, cs, state=state), old_encode(fmt, cs, state=state))
            frame16 = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
            assert same(CS.encode_planes(fmt, cs, frame16=frame16), old_encode(fmt, cs, frame16=frame16))


def test_left_siting_equals_the_4_2_0_definitions_called_directly():
    rng = np.random.default_rng(7)
    h, w = 46, 30
    for cs in range(4):
        y, u, v = random_samples(YS.FMT_I420, h, w, rng)
        assert np.array_equal(CS.decode(y, u, v, cs, 420), Y.decode(y, u, v, cs))
        frame = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        assert same(CS.encode(frame, cs, 420), Y.encode(frame, cs))
        y, u, v = random_samples(YS.FMT_P010, h, w, rng)
        assert np.array_equal(CS.decode(y, u, v, cs, 420, deep=True), T.decode10(y, u, v, cs))
        p = rng.integers(0, 65536, (h, w, 3))
        assert same(CS.encode10(p, cs, 420), T.encode10(p, cs))
        assert CS.decode_coefficients(cs) == Y.decode_coefficients(cs)
        assert CS.decode_coefficients(cs, deep=True) == T.decode10_coefficients(cs)
        assert CS.encode_coefficients(cs) == Y.encode_coefficients(cs)
        assert CS.encode10_coefficients(cs) == T.encode10_coefficients(cs)


def test_top_left_is_left_on_4_2_2_and_4_4_4_ignores_the_siting():
    rng = np.random.default_rng(9)
    h, w = 5, 34
    for fmt in FORMATS:
        if CS.SAMPLING[fmt] == 420:
            continue
        held = CS.to_words(fmt, *random_samples(fmt, h, w, rng))
        frame = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        left = CS.decode_planes(fmt, 5, held, width=w), CS.encode_planes(fmt, 5, frame=frame)
        alike = (CS.CHROMA_TOPLEFT,) if CS.SAMPLING[fmt] == 422 else (CS.CHROMA_TOPLEFT, CS.CHROMA_CENTER)
        for siting in alike:
            assert np.array_equal(CS.decode_planes(fmt, 5 | siting, held, width=w), left[0])
            assert same(CS.encode_planes(fmt, 5 | siting, frame=frame), left[1])
        if CS.SAMPLING[fmt] == 422:
            assert not np.array_equal(CS.decode_planes(fmt, 5 | CS.CHROMA_CENTER, held, width=w), left[0])


# ---- geometry, stated without the resampling code -----------------------------------------------------------------------
def chroma_positions2(sampling, siting, ch, cw):
    """(X2, Y2) of every chroma sample, in half luma pixels; 4:2:2 has its own row: Y2 = 2 y."""
    ox, oy = OFFSET2[siting]
    j, i = np.indices((ch, cw))
    return 4 * i + ox, (4 * j + oy if sampling == 420 else 2 * j)


def interior(kind, n):
    """The luma indices 0 .. 2n - 1 of an axis whose two nearest chroma samples exist (no clamp)."""
    x = np.arange(2 * n)
    if kind is None:
        return np.ones(2 * n, bool)
    return x <= 2 * n - 2 if kind == "co" else (x >= 1) & (x <= 2 * n - 2)


@pytest.mark.parametrize("sampling", [420, 422])
@pytest.mark.parametrize("siting", CS.SITINGS, ids=CS.SITING_NAMES.get)
def test_upsampling_reproduces_a_plane_linear_in_the_sitings_positions(sampling, siting):
    h, w = 12, 20
    ch, cw = YS.chroma_shape(sampling, h, w)
    a, b, c = 3, -2, 90
    x2, y2 = chroma_positions2(sampling, siting, ch, cw)
    plane = a * x2 + b * y2 + c                                 # an integer at every chroma sample
    got = CS.upsample16(plane, sampling, siting, h, w)
    ly, lx = np.indices((h, w))
    want = CS.SCALE * (a * 2 * lx + b * 2 * ly + c)             # the same function at the luma positions, in half pixels
    horizontal, vertical = CS.axes(sampling, siting)
    inside = interior(vertical, ch)[:, None] & interior(horizontal, cw)[None, :] if sampling == 420 else \
        np.ones(h, bool)[:, None] & interior(horizontal, cw)[None, :]
    assert inside.sum() > h * w // 2
    assert np.array_equal(got[inside], want[inside])
    # ... and read with ANOTHER siting it is off by the slope times the half-pixel shift between the two, exactly
    for other in CS.SITINGS:
        dx = OFFSET2[siting][0] - OFFSET2[other][0]
        dy = OFFSET2[siting][1] - OFFSET2[other][1] if sampling == 420 else 0
        ho, vo = CS.axes(sampling, other)
        ins = (interior(vo, ch) if sampling == 420 else np.ones(h, bool))[:, None] & interior(ho, cw)[None, :]
        shifted = CS.upsample16(plane, sampling, other, h, w)
        assert np.array_equal(shifted[ins], (want + CS.SCALE * (a * dx + b * dy))[ins]), (siting, other)


@pytest.mark.parametrize("sampling", [420, 422])
@pytest.mark.parametrize("siting", CS.SITINGS, ids=CS.SITING_NAMES.get)
def test_chroma_sums_of_a_linear_frame_are_its_value_at_the_chroma_position(sampling, siting):
    h, w = 12, 20
    ch, cw = YS.chroma_shape(sampling, h, w)
    a, b, c = 5, 7, 11
    ly, lx = np.indices((h, w))
    p = a * lx + b * ly + c
    got = CS.chroma_sum16(p, sampling, siting)
    x2, y2 = chroma_positions2(sampling, siting, ch, cw)
    want = (CS.SCALE // 2) * (a * x2 + b * y2) + CS.SCALE * c   # SCALE x the value at (X2 / 2, Y2 / 2)
    horizontal, vertical = CS.axes(sampling, siting)
    j, i = np.indices((ch, cw))
    inside = ((i >= 1) | (horizontal != "co")) & ((j >= 1) | (vertical != "co"))   # (index 2i - 1 clamps at i = 0)
    assert np.array_equal(got[inside], want[inside])
    assert got.shape == (ch, cw)


# ---- flat frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=name_of)
def test_flat_frames_give_the_same_bytes_under_every_siting(fmt):
    h, w = 6, 18
    deep = fmt in CS.DEEP
    shapes = [(h, w)] + [YS.chroma_shape(CS.SAMPLING[fmt], h, w)] * 2
    for matrix in CS.MATRICES:
        for values in ((40, 200, 90), (0, 0, 0), (255, 255, 255)):
            dt, k = (np.uint16, 4) if deep else (np.uint8, 1)
            held = CS.to_words(fmt, *(np.full(s, v * k, dt) for s, v in zip(shapes, values)))
            frame = np.empty((h, w, 4), np.uint8)
            frame[...] = values + (0,)
            decoded = [CS.decode_planes(fmt, matrix | s, held, width=w) for s in CS.SITINGS]
            encoded = [CS.encode_planes(fmt, matrix | s, frame=frame) for s in CS.SITINGS]
            assert all(np.array_equal(d, decoded[0]) for d in decoded)
            assert all(same(e, encoded[0]) for e in encoded)
            assert (decoded[0] == decoded[0][0, 0]).all()


# ---- BT.2020 ------------------------------------------------------------------------------------------------------------
KR, KB = Fraction("0.2627"), Fraction("0.0593")
KG = 1 - KR - KB


def rounded(x):
    """round half away from zero of an exact fraction."""
    return int(abs(x) + Fraction(1, 2)) * (1 if x >= 0 else -1)


def test_bt2020_coefficients_follow_from_k_r_and_k_b():
    assert KG == Fraction("0.6780")
    # full range, 8-bit: by hand 0.2627 x 65536 = 17216.3, 0.678 x 65536 = 44433.4, 0.0593 x 65536 = 3886.3
    (y, u, v), oy = CS.encode_coefficients(CS.CS_BT2020_FULL)
    assert y == (17216, 44433, 3886) and oy == 0
    assert u == tuple(rounded(k / (2 * (1 - KB)) * 65536) for k in (-KR, -KG, 1 - KB)) and u[2] == 32768
    assert v == tuple(rounded(k / (2 * (1 - KR)) * 65536) for k in (1 - KR, -KG, -KB)) and v[0] == 32768
    # 2 (1 - K_r) = 1.4746 -> 96639.4; 2 (1 - K_b) = 1.8814 -> 123299.4
    (ky, krv, kbu, kgu, kgv), oy = CS.decode_coefficients(CS.CS_BT2020_FULL)
    assert (ky, krv, kbu, oy) == (65536, 96639, 123299, 0)
    assert kgu == rounded(2 * KB * (1 - KB) / KG * 65536) == 10784
    assert kgv == rounded(2 * KR * (1 - KR) / KG * 65536) == 37444
    # limited range: the luma row x 219 / 255, the chroma rows x 224 / 255; decode the inverse
    (y, u, v), oy = CS.encode_coefficients(CS.CS_BT2020_LIMITED)
    assert y == tuple(rounded(k * Fraction(219, 255) * 65536) for k in (KR, KG, KB)) and oy == 16
    assert u == tuple(rounded(k / (2 * (1 - KB)) * Fraction(224, 255) * 65536) for k in (-KR, -KG, 1 - KB))
    assert v == tuple(rounded(k / (2 * (1 - KR)) * Fraction(224, 255) * 65536) for k in (1 - KR, -KG, -KB))
    (ky, krv, kbu, kgu, kgv), oy = CS.decode_coefficients(CS.CS_BT2020_LIMITED)
    assert (ky, oy) == (rounded(Fraction(255, 219) * 65536), 16)
    assert (krv, kbu) == (rounded(2 * (1 - KR) * Fraction(255, 224) * 65536), rounded(2 * (1 - KB) * Fraction(255, 224) * 65536))
    # 10-bit: 64..940 / 64..960, the ranges of the other matrices
    (ky, krv, _, _, _), oy = CS.decode_coefficients(CS.CS_BT2020_LIMITED, deep=True)
    assert (ky, krv, oy) == (rounded(Fraction(255, 876) * 65536), rounded(2 * (1 - KR) * Fraction(255, 896) * 65536), 64)
    (y, u, v), oy = CS.encode10_coefficients(CS.CS_BT2020_LIMITED)
    assert y == tuple(rounded(k * 876 / 65535 * 2 ** 32) for k in (KR, KG, KB)) and oy == 64
    assert u[2] == v[0] == rounded(Fraction(896, 2) / 65535 * 2 ** 32)
    (y, u, v), oy = CS.encode10_coefficients(CS.CS_BT2020_FULL)
    assert y == tuple(rounded(k * 1023 / 65535 * 2 ** 32) for k in (KR, KG, KB)) and oy == 0


COLOURS = {"white": (255, 255, 255), "black": (0, 0, 0), "red": (255, 0, 0), "green": (0, 255, 0), "blue": (0, 0, 255)}


def real_codes(rgb, limited, top):
    """The real-valued Y, U, V codes of an R'G'B' colour (0 .. 255) for a code range of 0 .. top (255 or 1023)."""
    r, g, b = (Fraction(c, 255) for c in rgb)
    yl = KR * r + KG * g + KB * b
    u, v = (b - yl) / (2 * (1 - KB)), (r - yl) / (2 * (1 - KR))
    unit = (top + 1) // 256
    if limited:
        return 16 * unit + 219 * unit * yl, 128 * unit + 224 * unit * u, 128 * unit + 224 * unit * v
    return top * yl, 128 * unit + top * u, 128 * unit + top * v


@pytest.mark.parametrize("matrix", [CS.CS_BT2020_LIMITED, CS.CS_BT2020_FULL], ids=["limited", "full"])
def test_bt2020_white_black_and_the_primaries_land_on_their_codes(matrix):
    limited = matrix == CS.CS_BT2020_LIMITED
    for name, rgb in COLOURS.items():
        frame = np.empty((2, 2, 4), np.uint8)
        frame[...] = rgb[::-1] + (0,)
        for siting in CS.SITINGS:
            for deep, top in ((False, 255), (True, 1023)):
                codes = CS.encode10(T.p_from_u8(frame), matrix | siting, 420) if deep else CS.encode(frame, matrix | siting, 420)
                want = real_codes(rgb, limited, top)
                for plane, real in zip(codes, want):
                    code = int(plane[0, 0])
                    assert (plane == code).all()
                    # the nearest code of the real value clamped to the range (coefficient rounding moves a sum by < 0.01)
                    assert abs(code - min(max(real, 0), top)) <= Fraction(51, 100), (name, deep, code, float(real))
                # and back: the decode returns the colour within one step
                y, u, v = codes
                back = CS.decode(y, u, v, matrix | siting, 420, deep)
                assert np.abs(back[..., :3].astype(int) - np.array(rgb[::-1])).max() <= 1, (name, deep)
    white = CS.encode(np.full((2, 2, 4), 255, np.uint8), matrix, 420)
    black = CS.encode(np.zeros((2, 2, 4), np.uint8), matrix, 420)
    assert [int(p[0, 0]) for p in white] == ([235, 128, 128] if limited else [255, 128, 128])
    assert [int(p[0, 0]) for p in black] == ([16, 128, 128] if limited else [0, 128, 128])
    white10 = CS.encode10(np.full((2, 2, 3), 65535), matrix, 420)
    assert [int(p[0, 0]) for p in white10] == ([940, 512, 512] if limited else [1023, 512, 512])


def test_bt2020_full_range_luma_of_pure_red_is_67():
    red = np.zeros((2, 2, 4), np.uint8)
    red[..., 2] = 255
    for siting in CS.SITINGS:
        assert (CS.encode(red, CS.CS_BT2020_FULL | siting, 420)[0] == 67).all()
        assert (CS.encode(red, CS.CS_BT2020_FULL | siting, 444)[0] == 67).all()


# ---- the values ---------------------------------------------------------------------------------------------------------
def test_the_headers_values_are_the_runtimes_and_the_definitions():
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()

    def value(name):
        m = re.search(r"\b" + name + r"\s*=\s*([0-9 <]+?)\s*[,}\n]", text)
        assert m, name
        return eval(m.group(1), {"__builtins__": {}})           # (a literal or `n << 8`)
    for name in ("CS_BT601_LIMITED", "CS_BT601_FULL", "CS_BT709_LIMITED", "CS_BT709_FULL", "CS_BT2020_LIMITED",
                 "CS_BT2020_FULL", "CHROMA_LEFT", "CHROMA_CENTER", "CHROMA_TOPLEFT"):
        assert value("JU_" + name) == getattr(R, name) == getattr(CS, name), name
    assert (R.CS_BT2020_LIMITED, R.CS_BT2020_FULL) == (4, 5)
    assert (R.CHROMA_LEFT, R.CHROMA_CENTER, R.CHROMA_TOPLEFT) == (0, 1 << 8, 2 << 8)


def test_what_a_runtime_refuses_the_definition_refuses():
    for bad in (3 << 8, 1 << 10, 6, 0xff, -1, (1 << 8) | 6, 1 << 31):
        with pytest.raises(ValueError):
            CS.split(bad)
    assert CS.split(5 | CS.CHROMA_TOPLEFT) == (5, CS.CHROMA_TOPLEFT)
