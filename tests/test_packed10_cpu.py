"""The definition of the packed 10-bit frame formats (tests/packed10_reference.py) and the binding's descriptors of them,
without a GPU: the words round-trip every sample value in every slot, ignore what the formats ignore and write 0 there;
Y410 and the two RGB formats carry an 8-bit frame without loss; host_frame / device_frame / the header's constants / the
test hook."""

import ctypes
import os
import re

import numpy as np
import pytest

import packed10_reference as P
import yuv10_reference as T
import yuv_sampled_reference as YS
from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
name_of = lambda f: P.FORMAT_NAMES[f]  # noqa: E731
WIDTHS = (2, 4, 6, 8, 46, 48, 50)


def all_values(fmt, w, seed=0):
    """Sample arrays of width w in which every slot of a row position takes all 1024 values (1024 rows, each column a
    permutation of 0..1023 of its own)."""
    rng = np.random.default_rng(seed + w)
    out = []
    for shape in P.sample_shapes(fmt, 1024, w):
        cols = [rng.permutation(1024) for _ in range(shape[1])]
        out.append(np.stack(cols, axis=1).astype(np.uint16))
    return out


# ---- 1. the words -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", P.NEW_FORMATS, ids=name_of)
@pytest.mark.parametrize("w", WIDTHS)
def test_words_round_trip_every_value_in_every_slot(fmt, w):
    samples = all_values(fmt, w)
    planes = P.to_words(fmt, *samples)
    assert len(planes) == 1 and planes[0].dtype == np.dtype(P.DTYPE[fmt])
    assert planes[0].shape == (1024, P.row_words(fmt, w))
    back = P.from_words(fmt, planes, width=w)
    for a, b in zip(samples, back):
        assert a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("fmt", P.NEW_FORMATS, ids=name_of)
@pytest.mark.parametrize("w", WIDTHS)
def test_junk_in_the_ignored_bits_changes_nothing(fmt, w):
    samples = all_values(fmt, w, 1)
    planes = P.to_words(fmt, *samples)
    dirty = P.junk(fmt, planes, w, np.random.default_rng(5))
    assert not np.array_equal(dirty[0], planes[0])
    for a, b in zip(samples, P.from_words(fmt, dirty, width=w)):
        assert np.array_equal(a, b)
    for cs in range(4):
        assert np.array_equal(P.decode_planes(fmt, cs, dirty, width=w)[:16], P.decode_planes(fmt, cs, planes, width=w)[:16])


@pytest.mark.parametrize("fmt", P.NEW_FORMATS, ids=name_of)
@pytest.mark.parametrize("w", WIDTHS)
def test_to_words_writes_zero_in_every_ignored_bit_and_unused_slot(fmt, w):
    full = P.to_words(fmt, *(np.full(s, 1023, np.uint16) for s in P.sample_shapes(fmt, 3, w)))[0]
    if fmt == P.FMT_Y210:
        assert (full == 0xFFC0).all()
        return
    assert (full & np.uint32(P.IGNORED32) == 0).all()
    if fmt != P.FMT_V210:
        assert (full == 0x3FFFFFFF).all()
        return
    # V210: 3 slots a word; exactly the slots of the W luma and W chroma samples are set, in the layout's order
    slots = np.stack([(full >> s) & 0x3ff for s in P.SLOTS], axis=-1).reshape(3, -1, 12)    # [row][group][slot]
    order_y, order_c = (1, 3, 5, 7, 9, 11), (0, 2, 4, 6, 8, 10)                              # Cb Y Cr | Y Cb Y | Cr Y Cb | Y Cr Y
    for g in range(P.groups(w)):
        left = min(6, w - 6 * g)                                                            # pixels of this group
        for k, slot in enumerate(order_y):
            assert (slots[:, g, slot] == (1023 if k < left else 0)).all(), (g, k)
        for k, slot in enumerate(order_c):                                                   # Cb0 Cr0 Cb1 Cr1 Cb2 Cr2
            assert (slots[:, g, slot] == (1023 if k // 2 < left // 2 else 0)).all(), (g, k)


def test_v210_layout_is_the_one_of_the_interface():
    y = np.arange(10, 16, dtype=np.uint16)[None]
    u = np.array([[100, 101, 102]], np.uint16)
    v = np.array([[200, 201, 202]], np.uint16)
    (words,) = P.to_words(P.FMT_V210, y, u, v)
    want = [100 | 10 << 10 | 200 << 20, 11 | 101 << 10 | 12 << 20, 201 | 13 << 10 | 102 << 20, 14 | 202 << 10 | 15 << 20]
    assert words.tolist() == [want]
    (y210,) = P.to_words(P.FMT_Y210, y, u, v)
    assert y210.tolist() == [[10 << 6, 100 << 6, 11 << 6, 200 << 6, 12 << 6, 101 << 6, 13 << 6, 201 << 6, 14 << 6, 102 << 6,
                              15 << 6, 202 << 6]]
    one = np.array([[1]], np.uint16)
    assert P.to_words(P.FMT_Y410, one * 2, one * 1, one * 3)[0].tolist() == [[1 | 2 << 10 | 3 << 20]]          # U Y V
    assert P.to_words(P.FMT_X2RGB10, one * 1, one * 2, one * 3)[0].tolist() == [[1 | 2 << 10 | 3 << 20]]       # B G R
    assert P.to_words(P.FMT_X2BGR10, one * 1, one * 2, one * 3)[0].tolist() == [[3 | 2 << 10 | 1 << 20]]       # R G B


@pytest.mark.parametrize("w", range(2, 60, 2))
def test_v210_row_bytes(w):
    want = 16 * -(-w // 6)
    assert P.row_bytes(P.FMT_V210, w) == want == 4 * R.v210_row_words(w)
    assert P.blank_planes(P.FMT_V210, 2, w)[0].shape == (2, want // 4)
    dt, shape = R.packed10_shape(R.FMT_V210, w, 2)
    assert np.dtype(dt) == np.uint32 and shape == (2, want // 4)
    assert R.device_frame(R.FMT_V210, w, 2, [4096]).strides[0] == want
    for fmt in P.NEW_FORMATS:
        if fmt != P.FMT_V210:
            assert P.row_bytes(fmt, w) == 4 * w


# ---- 2. the samples are the planar formats' ---------------------------------------------------------------------------------
def all_colours_frame():
    """[64][64 * 8][4]: a spread of colours holding every byte value in every channel, X junk."""
    rng = np.random.default_rng(11)
    f = rng.integers(0, 256, (64, 512, 4), dtype=np.uint8)
    v = np.arange(256, dtype=np.uint8)
    f[0, :256, 0], f[1, :256, 1], f[2, :256, 2] = v, v, v
    f[3, :256, :3] = v[:, None]
    return f


@pytest.mark.parametrize("cs", range(4))
def test_y410_carries_an_8_bit_frame_without_loss(cs):
    frame = all_colours_frame()
    samples = YS.encode10(T.p_from_u8(frame), cs, 444)
    words = P.to_words(P.FMT_Y410, *samples)
    assert np.array_equal(words[0], P.encode_planes(P.FMT_Y410, cs, frame=frame)[0])
    back = P.decode_planes(P.FMT_Y410, cs, words)
    assert np.array_equal(back[..., :3], frame[..., :3]) and (back[..., 3] == 0).all()


@pytest.mark.parametrize("fmt", P.RGB, ids=name_of)
def test_the_rgb_formats_round_trip_all_256_byte_values(fmt):
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    frame = np.stack([v, v[::-1, ::-1], v.T, np.full_like(v, 0x5a)], axis=-1)
    (words,) = P.encode_planes(fmt, 0, frame=frame)
    assert words.dtype == np.uint32 and words.shape == (16, 16) and (words >> 30 == 0).all()
    b, g, r = P.from_words(fmt, [words])
    for k, c in enumerate((b, g, r)):
        assert np.array_equal(c, (frame[..., k].astype(np.uint32) * 257) >> 6)
    back = P.decode_planes(fmt, 3, [words])
    assert np.array_equal(back[..., :3], frame[..., :3]) and (back[..., 3] == 0).all()
    other = P.FMT_X2BGR10 if fmt == P.FMT_X2RGB10 else P.FMT_X2RGB10
    assert np.array_equal(P.decode_planes(other, 0, [words])[..., :3], frame[..., 2::-1])


def test_decode_and_encode_delegate_to_the_planar_definitions():
    rng = np.random.default_rng(3)
    h, w = 4, 10
    frame = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    state = (rng.random((h, w, 4)) - 0.5).astype(np.float16)
    p16 = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
    import output_reference as O
    import rgb_reference as G
    for cs in range(4):
        for fmt, twin in ((P.FMT_V210, YS.FMT_P210), (P.FMT_Y210, YS.FMT_P210), (P.FMT_Y410, YS.FMT_I410)):
            for kw, planar in (({"frame": frame}, YS.encode_planes(twin, cs, frame=frame)),
                               ({"state": state}, YS.encode_planes(twin, cs, state=state)),
                               ({"frame16": p16}, O.encode16(twin, cs, p16))):
                words = P.encode_planes(fmt, cs, **kw)
                for a, b in zip(P.from_words(fmt, words, width=w), YS.from_words(twin, planar)):
                    assert np.array_equal(a, b)
                assert np.array_equal(P.decode_planes(fmt, cs, words, width=w), YS.decode_planes(twin, cs, planar))
    for fmt in P.RGB:
        for kw, planar in (({"frame": frame}, G.encode_planes(G.FMT_RGBP10, frame=frame)),
                           ({"state": state}, G.encode_planes(G.FMT_RGBP10, state=state)),
                           ({"frame16": p16}, O.encode16(G.FMT_RGBP10, 0, p16))):
            words = P.encode_planes(fmt, 0, **kw)
            b, g, r = P.from_words(fmt, words)
            for a, c in zip((r, g, b), planar):
                assert np.array_equal(a, c)
            assert np.array_equal(P.decode_planes(fmt, 0, words), G.decode_planes(G.FMT_RGBP10, planar))


# ---- 3. header, binding, hook -----------------------------------------------------------------------------------------------
# (22, 23, 26 and 43 are held to be no format by tests/test_gpu_yuv_sampled.py, test_gpu_rgb.py and test_yuv_lookahead_cpu.py)
WANT = {"V210": 48, "Y210": 49, "Y410": 50, "X2RGB10": 45, "X2BGR10": 44}


def test_header_constants_match_the_binding_and_the_definition():
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    for name, value in WANT.items():
        assert re.search(rf"\bJU_FMT_{name} = {value}\b", text), name
        assert getattr(R, "FMT_" + name) == getattr(P, "FMT_" + name) == value
    assert sorted(P.NEW_FORMATS) == sorted(WANT.values())
    assert "no packed 10-bit" not in text and "without packed 10-bit" not in text
    for words in ("x2rgb10", "dithering", "alpha", "unquantised", "castKernel truncates", "P016", "NV16"):
        assert words in text, words


def test_the_hook_is_declared_and_exported_by_the_test_flavour_only(product_library, hip_library):
    assert "ju_debug_packed10" in R.HOOK_SYMBOLS
    assert hasattr(hip_library, "ju_debug_packed10") and not hasattr(product_library, "ju_debug_packed10")
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    assert re.search(r"JU_API\s+int\s+ju_debug_packed10\s*\(", test_header)
    assert "ju_debug_packed10" not in open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()


def test_the_hook_refuses_bad_arguments_without_a_gpu(hip_library):
    planes, strides = (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)()
    call = hip_library.ju_debug_packed10
    err = hip_library.ju_last_error
    for other in (0, 2, 5, 7, 19, 21, 22, 23, 25, 26, 37, 42, 43, 46, 47, 51):     # old formats and no formats
        assert call(0, other, 0, 4, 4, None, 0, planes, strides) == 1, other
        assert b"packed 10-bit" in err()
    for fmt in P.NEW_FORMATS:
        assert call(4, fmt, 0, 4, 4, None, 0, planes, strides) == 1
        assert call(-1, fmt, 0, 4, 4, None, 0, planes, strides) == 1
        assert call(0, fmt, 0, 0, 4, None, 0, planes, strides) == 1
        for op in range(4):
            assert call(op, fmt, 0, 6, 3, None, 0, planes, strides) == 1             # a NULL image
            assert b"null" in err()
    for fmt in (P.FMT_V210, P.FMT_Y210):
        assert call(0, fmt, 0, 7, 4, None, 0, planes, strides) == 1                # an odd width, before the NULL image
        assert b"even width" in err()
    # (Y410 and the RGB formats take odd sizes: the NULL image stops them)
    assert call(0, P.FMT_Y410, 0, 7, 3, None, 0, planes, strides) == 1 and b"null" in err()
    # alignment and stride, on fake addresses that are never dereferenced: refused before any launch
    image = ctypes.c_void_p(4096)
    for fmt, align in ((P.FMT_V210, 4), (P.FMT_Y210, 2), (P.FMT_Y410, 4), (P.FMT_X2RGB10, 4), (P.FMT_X2BGR10, 4)):
        row = P.row_bytes(fmt, 8)
        planes[0], strides[0] = 8192 + align // 2, row
        aligned = b"even addresses" if align == 2 else b"multiples of 4"
        assert call(0, fmt, 0, 8, 2, image, 32, planes, strides) == 1 and aligned in err()
        planes[0], strides[0] = 8192, row + align // 2
        assert call(0, fmt, 0, 8, 2, image, 32, planes, strides) == 1 and aligned in err()
        planes[0], strides[0] = 8192, row - align
        assert call(0, fmt, 0, 8, 2, image, 32, planes, strides) == 1 and b"|stride| smaller than a row" in err()
        strides[0] = -(row - align)
        assert call(1, fmt, 0, 8, 2, image, 32, planes, strides) == 1 and b"|stride| smaller than a row" in err()
        planes[0], strides[0] = None, row
        assert call(0, fmt, 0, 8, 2, image, 32, planes, strides) == 1 and b"null" in err()


def test_host_frames_of_the_new_formats():
    h, w = 5, 14
    for fmt in (R.FMT_Y410, R.FMT_X2RGB10, R.FMT_X2BGR10):
        a = np.zeros((h, w), np.uint32)
        f = R.host_frame(fmt, [a])
        assert (f.format, f.width, f.height, f.strides[0], f.location) == (fmt, w, h, 4 * w, R.LOC_CPU)
        assert f.planes[0] == a.ctypes.data
        odd = R.host_frame(fmt, [np.zeros((3, 7), np.uint32)])
        assert (odd.width, odd.height) == (7, 3)
        padded = np.zeros((h, w + 3), np.uint32)[::-1, :w]                          # bottom-up, padded rows
        f = R.host_frame(fmt, [padded])
        assert f.strides[0] == -4 * (w + 3) and f.planes[0] == padded.ctypes.data
        for bad in (np.zeros((h, w), np.int32), np.zeros((h, w), np.uint16), np.zeros((h, w), np.float32),
                    np.zeros((h, w, 1), np.uint32), np.zeros((h, 2 * w), np.uint32)[:, ::2]):
            with pytest.raises(ValueError):
                R.host_frame(fmt, [bad])
        with pytest.raises(ValueError):
            R.host_frame(fmt, [a, a])
    a = np.zeros((h, 2 * w), np.uint16)
    f = R.host_frame(R.FMT_Y210, [a])
    assert (f.format, f.width, f.height, f.strides[0]) == (R.FMT_Y210, w, h, 4 * w) and f.planes[0] == a.ctypes.data
    for bad in (np.zeros((h, 2 * w), np.uint32), np.zeros((h, 2 * w), np.uint8), np.zeros((h, 2 * w + 2), np.uint16),
                np.zeros((h, 4 * w), np.uint16)[:, ::2], np.zeros((h, w, 2), np.uint16)):
        with pytest.raises(ValueError):
            R.host_frame(R.FMT_Y210, [bad])
    # V210: the array cannot tell W
    words = R.v210_row_words(w)                                                      # 14 pixels: 3 groups, 12 words
    assert words == 12
    a = np.zeros((h, words), np.uint32)
    with pytest.raises(ValueError, match="width"):
        R.host_frame(R.FMT_V210, [a])
    f = R.host_frame(R.FMT_V210, [a], width=w)
    assert (f.format, f.width, f.height, f.strides[0]) == (R.FMT_V210, w, h, 4 * words) and f.planes[0] == a.ctypes.data
    assert R.host_frame(R.FMT_V210, [a], width=18).width == 18 and R.host_frame(R.FMT_V210, [a], width=16).width == 16
    wide = np.zeros((h, 32), np.uint32)[::-1]                                        # the conventional 128-byte stride
    f = R.host_frame(R.FMT_V210, [wide], width=w)
    assert f.strides[0] == -128 and f.width == w
    for kw, bad in (({"width": 20}, a), ({"width": 13}, a), ({"width": 0}, a), ({"width": w}, a.astype(np.uint16)),
                    ({"width": w}, a.astype(np.int32)), ({"width": w}, np.zeros((h, 2 * words), np.uint32)[:, ::2]),
                    ({"width": w}, np.zeros((h, words, 1), np.uint32))):
        with pytest.raises(ValueError):
            R.host_frame(R.FMT_V210, [bad], **kw)
    # `width` is for V210 alone; the other formats and the old ones work as before without it
    assert R.host_frame(R.FMT_BGRX, [np.zeros((4, 6, 4), np.uint8)]).width == 6


def test_device_frames_default_to_dense_strides():
    w, h = 10, 5
    want = {R.FMT_V210: [32], R.FMT_Y210: [4 * w], R.FMT_Y410: [4 * w], R.FMT_X2RGB10: [4 * w], R.FMT_X2BGR10: [4 * w]}
    assert set(want) == set(P.NEW_FORMATS)
    for fmt, strides in want.items():
        f = R.device_frame(fmt, w, h, [4096])
        assert f.format == fmt and f.location == R.LOC_DEVICE and (f.width, f.height) == (w, h)
        assert f.strides[0] == strides[0] == P.row_bytes(fmt, w) and f.planes[0] == 4096
    assert R.device_frame(R.FMT_V210, w, h, [4096], strides=[-128]).strides[0] == -128
