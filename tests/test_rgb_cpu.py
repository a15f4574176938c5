"""The definition of the RGB frame formats (tests/rgb_reference.py) and the binding's descriptors of them, without a GPU:
the properties the definition is chosen for -- every 8-bit value survives every deep format, the decodes are monotonic
and ignore what the formats ignore, a deep output decoded again is the frame or one above it -- and host_frame /
device_frame / the header's constants / the test hook."""

import os
import re

import numpy as np
import pytest

import rgb_reference as G
from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
name_of = lambda f: G.FORMAT_NAMES[f]  # noqa: E731


def ramp_frame():
    """[16][16][4]: every byte value once in each of B, G, R (in three different orders), X junk."""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    return np.stack([v, v[::-1, ::-1], v.T, np.full_like(v, 0x5a)], axis=-1)


# ---- 1. round trips and permutations --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", G.DEEP, ids=name_of)
def test_every_byte_value_survives_a_deep_format(fmt):
    frame = ramp_frame()
    back = G.decode_planes(fmt, G.encode_planes(fmt, frame=frame))
    assert np.array_equal(back[..., :3], frame[..., :3]) and (back[..., 3] == 0).all()


def test_the_8_bit_formats_are_permutations():
    frame = ramp_frame()
    b, g, r = frame[..., 0], frame[..., 1], frame[..., 2]
    (bgr24,), (rgb24,), (rgbx,) = (G.encode_planes(f, frame=frame) for f in (G.FMT_BGR24, G.FMT_RGB24, G.FMT_RGBX))
    assert bgr24.shape == (16, 16, 3) and np.array_equal(bgr24, np.stack([b, g, r], -1))
    assert rgb24.shape == (16, 16, 3) and np.array_equal(rgb24, np.stack([r, g, b], -1))
    assert rgbx.shape == (16, 16, 4) and np.array_equal(rgbx, np.stack([r, g, b, np.zeros_like(b)], -1))   # X out: 0
    planes = G.encode_planes(G.FMT_RGBP8, frame=frame)
    assert all(np.array_equal(p, c) for p, c in zip(planes, (r, g, b)))                                  # planes R, G, B
    for fmt in G.EIGHT:
        back = G.decode_planes(fmt, G.encode_planes(fmt, frame=frame))
        assert np.array_equal(back[..., :3], frame[..., :3]) and (back[..., 3] == 0).all()
    junk = rgbx.copy()
    junk[..., 3] = 0xc3                                                                                  # X in: ignored
    assert np.array_equal(G.decode_planes(G.FMT_RGBX, [junk]), G.decode_planes(G.FMT_RGBX, [rgbx]))


def test_packed_deep_layouts():
    frame = ramp_frame()
    (w64,), (f96,) = G.encode_planes(G.FMT_BGRX64, frame=frame), G.encode_planes(G.FMT_BGR96F, frame=frame)
    assert w64.dtype == np.uint16 and w64.shape == (16, 16, 4) and (w64[..., 3] == 0).all()
    assert np.array_equal(w64[..., :3], frame[..., :3].astype(np.uint16) * 257)
    assert f96.dtype == np.float32 and f96.shape == (16, 16, 3) and np.array_equal(f96, frame[..., :3].astype(np.float32))
    junk = w64.copy()
    junk[..., 3] = 0xbeef
    assert np.array_equal(G.decode_planes(G.FMT_BGRX64, [junk]), G.decode_planes(G.FMT_BGRX64, [w64]))
    p10 = G.encode_planes(G.FMT_RGBP10, frame=frame)
    assert all(p.dtype == np.uint16 and int(p.max()) <= 1023 for p in p10)
    assert np.array_equal(p10[0], (frame[..., 2].astype(np.uint16) * 257) >> 6)
    ps, ph = G.encode_planes(G.FMT_RGBPS, frame=frame), G.encode_planes(G.FMT_RGBPH, frame=frame)
    assert ps[2].dtype == np.float32 and ph[2].dtype == np.float16
    assert np.array_equal(ps[2], frame[..., 0].astype(np.float32) / np.float32(255))
    assert np.array_equal(ph[2], ps[2].astype(np.float16))


# ---- 2. the integer decodes ----------------------------------------------------------------------------------------------
def test_all_words_decode_monotonically():
    words = np.arange(65536, dtype=np.uint16)
    u8 = G.u8_from_word16(words).astype(int)
    assert u8[0] == 0 and u8[-1] == 255 and (np.diff(u8) >= 0).all() and (np.diff(u8) <= 1).all()
    assert np.array_equal(u8[np.arange(256) * 257], np.arange(256))                # 257 u8 -> u8
    assert np.array_equal(G.u8_from_word16(np.arange(256) * 257 + 128), np.arange(256))   # rounds to nearest, ties up
    assert np.array_equal(G.u8_from_word16(np.arange(1, 256) * 257 - 129), np.arange(0, 255))


def test_all_ten_bit_values_decode_monotonically_and_ignore_the_upper_bits():
    p = np.arange(1024, dtype=np.uint16)
    u8 = G.u8_from_word10(p).astype(int)
    assert u8[0] == 0 and u8[-1] == 255 and (np.diff(u8) >= 0).all() and (np.diff(u8) <= 1).all()
    rng = np.random.default_rng(1)
    for _ in range(4):
        junk = (rng.integers(0, 64, p.shape, dtype=np.uint16) << 10).astype(np.uint16)
        assert np.array_equal(G.u8_from_word10(p | junk), u8)
    assert np.array_equal(G.u8_from_word10(np.full(4, 0xfc00, np.uint16)), np.zeros(4))
    # the widening is bit replication: 1023 -> 65535, 512 -> 32800
    assert G.u8_from_word10(np.array([512]))[0] == (32800 + 128) // 257


# ---- 3. the float decodes ------------------------------------------------------------------------------------------------
def test_float_decodes_round_clamp_and_take_nan_as_zero():
    k = np.arange(256)
    unit = (k.astype(np.float32) / np.float32(255)).astype(np.float32)
    for v in (unit, np.nextafter(unit, np.float32(2)), np.nextafter(unit, np.float32(-1))):
        assert np.array_equal(G.u8_from_unit(v), k)                                # k / 255 and both f32 neighbours
    assert np.array_equal(G.u8_from_unit(unit.astype(np.float16)), k)              # ... and rounded to f16
    odd = np.array([-1.0, -0.0, 0.0, 1.0, 1.5, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.5, 0.00196, 0.00197], np.float32)
    assert np.array_equal(G.u8_from_unit(odd), [0, 0, 0, 255, 255, 255, 0, 255, 0, 0, 128, 0, 1])
    with np.errstate(over="ignore"):
        odd16 = odd.astype(np.float16)                                             # (1e30 -> inf)
    assert np.array_equal(G.u8_from_unit(odd16), [0, 0, 0, 255, 255, 255, 0, 255, 0, 0, 128, 0, 1])
    f = k.astype(np.float32)
    for v in (f, np.nextafter(f, np.float32(1000)), np.nextafter(f, np.float32(-1000))):
        assert np.array_equal(G.u8_from_f255(v), k)
    odd = np.array([-3.0, 0.49, 0.5, 254.49, 254.5, 255.0, 300.0, np.inf, -np.inf, np.nan], np.float32)
    assert np.array_equal(G.u8_from_f255(odd), [0, 0, 1, 254, 255, 255, 255, 255, 0, 0])
    # a multiply followed by an add, each rounded to f32
    v = np.float32(0.49803925)
    prod = np.float32(v * np.float32(255))
    assert G.u8_from_unit(np.array([v]))[0] == np.floor(np.float32(prod + np.float32(0.5)))


def test_decodes_are_monotonic_in_the_float_formats():
    v = np.sort(np.random.default_rng(5).uniform(-0.1, 1.1, 20000).astype(np.float32))
    for dec, arg in ((G.u8_from_unit, v), (G.u8_from_unit, v.astype(np.float16)), (G.u8_from_f255, v * np.float32(255))):
        assert (np.diff(dec(arg).astype(int)) >= 0).all()


# ---- 4. outputs from the state --------------------------------------------------------------------------------------------
def all_state_values():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    s = bits.view(np.float16)
    with np.errstate(invalid="ignore"):
        s = s[np.isfinite(s) & (np.abs(s.astype(np.float32)) <= 0.5)]
    return s


@pytest.mark.parametrize("fmt", G.DEEP, ids=name_of)
def test_a_deep_output_of_the_state_decodes_to_the_frame_or_one_above(fmt):
    """The frame is trunc((s + 0.5) * 255); the deep output holds s + 0.5 to at least 10 bits and its decode rounds to
    nearest, so decoded again it is that value or one above, for every f16 the state can hold in range."""
    s = all_state_values()
    assert s.size == 28674
    state = np.zeros((1, s.size, 4), np.float16)
    state[0, :, :3] = s[:, None]
    back = G.decode_planes(fmt, G.encode_planes(fmt, state=state))[0, :, :3].astype(int)
    frame = np.trunc((s.astype(np.float64) + 0.5) * 255.0).astype(int)
    diff = back - frame[:, None]
    assert diff.min() >= 0 and diff.max() <= 1, (int(diff.min()), int(diff.max()))
    assert (back[:, 0] == back[:, 1]).all() and (back[:, 0] == back[:, 2]).all()


def test_state_samples():
    s = np.array([-0.5, 0.5, 0.0, -0.25, 0.25, 0.75, -0.75, 2.0 ** -12, -(2.0 ** -24)], np.float16)
    assert np.array_equal(G.samples_from_state("w16", s), [0, 65535, 32768, 16384, 49152, 65535, 0, 32784, 32767])
    assert np.array_equal(G.samples_from_state("w10", s), np.array([0, 65535, 32768, 16384, 49152, 65535, 0, 32784, 32767]) >> 6)
    unit = G.samples_from_state("s", s)
    assert unit.dtype == np.float32
    assert np.array_equal(unit, np.array([0, 1, 0.5, 0.25, 0.75, 1, 0, 0.5 + 2.0 ** -12, 0.5 - 2.0 ** -24], np.float32))
    half = G.samples_from_state("h", s)
    assert half.dtype == np.float16 and np.array_equal(half, unit.astype(np.float16))
    assert half[7] == np.float16(0.5) and half[8] == np.float16(0.5)               # (f16 holds 11 bits: both round to 0.5)
    f255 = G.samples_from_state("f255", s)
    assert f255.dtype == np.float32 and np.array_equal(f255, unit * np.float32(255))


def test_encode_planes_chooses_the_source():
    frame = ramp_frame()
    state = (frame.astype(np.float32) / 255.0 - 0.5).astype(np.float16)
    for fmt in G.DEEP:
        a, b = G.encode_planes(fmt, frame=frame), G.encode_planes(fmt, state=state)
        assert [p.dtype for p in a] == [p.dtype for p in b] == [np.dtype(G.DTYPE[fmt])] * len(a)
        assert any(not np.array_equal(x, y) for x, y in zip(a, b))
    for fmt in G.NEW_FORMATS:
        blank = G.blank_planes(fmt, 3, 5)
        made = G.encode_planes(fmt, frame=np.zeros((3, 5, 4), np.uint8))
        assert [(p.shape, p.dtype) for p in blank] == [(p.shape, p.dtype) for p in made]


# ---- 5. header, binding, hook ---------------------------------------------------------------------------------------------
WANT = {"BGR24": 32, "RGB24": 33, "RGBX": 34, "BGRX64": 35, "RGBP8": 36, "RGBP10": 37, "RGBP16": 38, "RGBPH": 39,
        "RGBPS": 40, "BGR96F": 41}


def test_header_constants_match_the_binding_and_the_definition():
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    for name, value in WANT.items():
        assert re.search(rf"\bJU_FMT_{name} = {value}\b", text), name
        assert getattr(R, "FMT_" + name) == getattr(G, "FMT_" + name) == value
    assert sorted(G.NEW_FORMATS) == sorted(WANT.values())
    assert "no 16-bit RGB output" not in text
    for words in ("x2rgb10", "dithering", "alpha", "unquantised", "castKernel truncates"):
        assert words in text, words


def test_the_hook_is_declared_and_exported_by_the_test_flavour_only(product_library, hip_library):
    assert "ju_debug_rgb" in R.HOOK_SYMBOLS
    assert hasattr(hip_library, "ju_debug_rgb") and not hasattr(product_library, "ju_debug_rgb")
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    assert re.search(r"JU_API\s+int\s+ju_debug_rgb\s*\(", test_header)
    assert "ju_debug_rgb" not in open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()


def test_the_hook_refuses_bad_arguments_without_a_gpu(hip_library):
    import ctypes
    planes, strides = (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)()
    call = hip_library.ju_debug_rgb
    assert call(0, R.FMT_I444, 4, 4, None, 0, planes, strides) == 1                # a YUV format
    assert b"RGB" in hip_library.ju_last_error()
    assert call(0, 42, 4, 4, None, 0, planes, strides) == 1                        # no format
    assert call(3, R.FMT_BGR24, 4, 4, None, 0, planes, strides) == 1
    assert call(2, R.FMT_RGBP8, 4, 4, None, 0, planes, strides) == 1               # op 2 with an 8-bit format
    assert b"deep" in hip_library.ju_last_error()
    assert call(0, R.FMT_BGR24, 0, 4, None, 0, planes, strides) == 1
    assert call(0, R.FMT_BGR24, 3, 3, None, 0, planes, strides) == 1               # (odd sizes pass: the NULL image stops it)
    assert b"null" in hip_library.ju_last_error()


def test_host_frames_of_the_new_formats():
    h, w = 5, 7
    shapes = {R.FMT_BGR24: ((h, w, 3), np.uint8), R.FMT_RGB24: ((h, w, 3), np.uint8), R.FMT_RGBX: ((h, w, 4), np.uint8),
              R.FMT_BGRX64: ((h, w, 4), np.uint16), R.FMT_BGR96F: ((h, w, 3), np.float32)}
    for fmt, (shape, dt) in shapes.items():
        a = np.zeros(shape, dt)
        f = R.host_frame(fmt, [a])
        row = w * shape[2] * np.dtype(dt).itemsize
        assert (f.format, f.width, f.height, f.strides[0], f.location) == (fmt, w, h, row, R.LOC_CPU)
        assert f.planes[0] == a.ctypes.data
        padded = np.zeros((h, w + 3, shape[2]), dt)[::-1, :w]                       # bottom-up, padded rows
        f = R.host_frame(fmt, [padded])
        assert f.strides[0] == -(w + 3) * shape[2] * np.dtype(dt).itemsize and f.planes[0] == padded.ctypes.data
        wrong = np.float64 if dt != np.float64 else np.uint8
        with pytest.raises(ValueError):
            R.host_frame(fmt, [np.zeros(shape, wrong)])
        with pytest.raises(ValueError):
            R.host_frame(fmt, [np.zeros(shape, np.uint16 if dt == np.uint8 else np.uint8)])
        with pytest.raises(ValueError):
            R.host_frame(fmt, [a, a, a])                                            # packed: one array
        with pytest.raises(ValueError):
            R.host_frame(fmt, [np.zeros((h, w, 7 - shape[2]), dt)])                 # 3 samples for 4 and 4 for 3
        with pytest.raises(ValueError):
            R.host_frame(fmt, [np.zeros((h, 2 * w, shape[2]), dt)[:, ::2]])         # columns not contiguous
    planar = {R.FMT_RGBP8: np.uint8, R.FMT_RGBP10: np.uint16, R.FMT_RGBP16: np.uint16, R.FMT_RGBPH: np.float16,
              R.FMT_RGBPS: np.float32}
    for fmt, dt in planar.items():
        size = np.dtype(dt).itemsize
        r, g, b = np.zeros((h, w), dt), np.zeros((h, w + 2), dt)[:, :w], np.zeros((h, w), dt)[::-1]
        f = R.host_frame(fmt, [r, g, b])
        assert (f.format, f.width, f.height) == (fmt, w, h)
        assert (f.strides[0], f.strides[1], f.strides[2]) == (w * size, (w + 2) * size, -w * size)
        assert [f.planes[k] for k in range(3)] == [r.ctypes.data, g.ctypes.data, b.ctypes.data]
        for bad in (np.uint8 if dt != np.uint8 else np.uint16, np.float64):
            with pytest.raises(ValueError):
                R.host_frame(fmt, [np.zeros((h, w), bad)] * 3)
        with pytest.raises(ValueError):
            R.host_frame(fmt, [r, g])                                               # three planes
        with pytest.raises(ValueError):
            R.host_frame(fmt, [r, r, np.zeros((h, w + 1), dt)])                     # of one shape
        with pytest.raises(ValueError):
            R.host_frame(fmt, [np.zeros((h, 2 * w), dt)[:, ::2]] * 3)               # columns not contiguous
        with pytest.raises(ValueError):
            R.host_frame(fmt, [np.zeros((h, w, 3), dt)])
    assert set(shapes) | set(planar) == set(G.NEW_FORMATS)
    # f16 and uint16 share a size, not a format
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_RGBPH, [np.zeros((h, w), np.uint16)] * 3)
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_RGBP16, [np.zeros((h, w), np.float16)] * 3)


def test_device_frames_default_to_dense_strides():
    w, h = 9, 5
    want = {R.FMT_BGR24: [3 * w], R.FMT_RGB24: [3 * w], R.FMT_RGBX: [4 * w], R.FMT_BGRX64: [8 * w],
            R.FMT_BGR96F: [12 * w], R.FMT_RGBP8: [w] * 3, R.FMT_RGBP10: [2 * w] * 3, R.FMT_RGBP16: [2 * w] * 3,
            R.FMT_RGBPH: [2 * w] * 3, R.FMT_RGBPS: [4 * w] * 3}
    assert set(want) == set(G.NEW_FORMATS)
    for fmt, strides in want.items():
        ptrs = [4096 + 256 * k for k in range(len(strides))]
        f = R.device_frame(fmt, w, h, ptrs)
        assert f.format == fmt and f.location == R.LOC_DEVICE and (f.width, f.height) == (w, h)
        assert [f.strides[k] for k in range(len(strides))] == strides
        assert [f.planes[k] for k in range(len(strides))] == ptrs
    f = R.device_frame(R.FMT_BGR24, w, h, [4096], strides=[-32])
    assert f.strides[0] == -32
