"""The definition of 4:2:2 and 4:4:4 frame I/O (tests/yuv_sampled_reference.py) against the project's 4:2:0 definitions
and against itself, the packing helpers, and the binding's view of the new formats.  No GPU."""

import os
import re

import numpy as np
import pytest

import yuv10_reference as T
import yuv_reference as Y
import yuv_sampled_reference as S
from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSS = (Y.CS_BT601_LIMITED, Y.CS_BT601_FULL, Y.CS_BT709_LIMITED, Y.CS_BT709_FULL)


def samples(rng, sampling, h, w, deep):
    top, dt = (1024, np.uint16) if deep else (256, np.uint8)
    ch, cw = S.chroma_shape(sampling, h, w)
    return [rng.integers(0, top, s, dtype=dt) for s in ((h, w), (ch, cw), (ch, cw))]


# ---- 1. sampling 4:2:0 is the existing definition -------------------------------------------------------------------------
@pytest.mark.parametrize("cs", CSS)
def test_sampling_420_gives_the_bytes_of_the_existing_definitions(cs):
    rng = np.random.default_rng(cs)
    for (h, w) in [(2, 2), (6, 10), (18, 34)]:
        y, u, v = samples(rng, 420, h, w, False)
        assert np.array_equal(S.decode(y, u, v, cs, 420), Y.decode(y, u, v, cs))
        y, u, v = samples(rng, 420, h, w, True)
        assert np.array_equal(S.decode(y, u, v, cs, 420, deep=True), T.decode10(y, u, v, cs))
        bgrx = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        for a, b in zip(S.encode(bgrx, cs, 420), Y.encode(bgrx, cs)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        for p in (T.p_from_u8(bgrx), rng.integers(0, 65536, (h, w, 3))):
            for a, b in zip(S.encode10(p, cs, 420), T.encode10(p, cs)):
                assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- 2. relations between the samplings ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", CSS)
def test_422_chroma_of_a_frame_with_doubled_rows_is_the_420_chroma(cs):
    rng = np.random.default_rng(10 + cs)
    half = rng.integers(0, 256, (7, 22, 4), dtype=np.uint8)
    frame = np.repeat(half, 2, axis=0)                          # rows 2j and 2j + 1 equal
    _, u2, v2 = S.encode(frame, cs, 422)
    _, u0, v0 = S.encode(frame, cs, 420)
    assert np.array_equal(u2[0::2], u0) and np.array_equal(u2[1::2], u0)
    assert np.array_equal(v2[0::2], v0) and np.array_equal(v2[1::2], v0)
    p = np.repeat(rng.integers(0, 65536, (7, 22, 3)), 2, axis=0)
    _, u2, v2 = S.encode10(p, cs, 422)
    _, u0, v0 = S.encode10(p, cs, 420)
    assert np.array_equal(u2[0::2], u0) and np.array_equal(u2[1::2], u0)
    assert np.array_equal(v2[0::2], v0) and np.array_equal(v2[1::2], v0)


@pytest.mark.parametrize("cs", CSS)
def test_444_chroma_of_a_frame_with_one_colour_per_row_is_the_422_chroma(cs):
    rng = np.random.default_rng(20 + cs)
    frame = np.repeat(rng.integers(0, 256, (9, 1, 4), dtype=np.uint8), 14, axis=1)
    y4, u4, v4 = S.encode(frame, cs, 444)
    y2, u2, v2 = S.encode(frame, cs, 422)
    assert np.array_equal(y4, y2) and np.array_equal(u4[:, 0::2], u2) and np.array_equal(v4[:, 0::2], v2)
    p = np.repeat(rng.integers(0, 65536, (9, 1, 3)), 14, axis=1)
    y4, u4, v4 = S.encode10(p, cs, 444)
    y2, u2, v2 = S.encode10(p, cs, 422)
    assert np.array_equal(y4, y2) and np.array_equal(u4[:, 0::2], u2) and np.array_equal(v4[:, 0::2], v2)


@pytest.mark.parametrize("deep", [False, True], ids=["8-bit", "10-bit"])
def test_flat_chroma_decodes_alike_in_all_samplings(deep):
    rng = np.random.default_rng(31)
    h, w = 8, 12
    top, dt = (1024, np.uint16) if deep else (256, np.uint8)
    for cs in CSS:
        y = rng.integers(0, top, (h, w), dtype=dt)
        cu, cv = (int(c) for c in rng.integers(0, top, 2))
        got = []
        for sampling in (420, 422, 444):
            shape = S.chroma_shape(sampling, h, w)
            got.append(S.decode(y, np.full(shape, cu, dt), np.full(shape, cv, dt), cs, sampling, deep))
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[1], got[2])


def test_422_decode_interpolates_odd_columns_and_clamps_at_the_row_end():
    u = np.array([[10, 30, 200]], np.uint8)
    c8 = S.upsample8_sampled(u, 422, 1, 6)
    assert c8.tolist() == [[80, 160, 240, 920, 1600, 1600]]
    assert S.upsample8_sampled(u, 444, 1, 3).tolist() == [[80, 240, 1600]]
    p = np.arange(6, dtype=np.int64)[None] * 10                 # one row: 0 10 20 30 40 50
    assert S.chroma_sum(p, 422).tolist() == [[0 + 0 + 10, 10 + 40 + 30, 30 + 80 + 50]]
    assert S.chroma_sum(p, 444) is p
    with pytest.raises(ValueError):
        S.chroma_shape(422, 4, 5)
    with pytest.raises(ValueError):
        S.chroma_shape(420, 5, 4)
    assert S.chroma_shape(422, 5, 4) == (5, 2) and S.chroma_shape(444, 5, 3) == (5, 3)


# ---- 3. the 4:4:4 round trips over all 2^24 colours ----------------------------------------------------------------------
def all_colours():
    """The 2^24 colours in 64 slabs of [4 blue values][256][256][3] (B, G, R)."""
    g, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for b0 in range(0, 256, 4):
        slab = np.empty((4, 256, 256, 3), np.uint8)
        slab[..., 1], slab[..., 2] = g, r
        slab[..., 0] = np.arange(b0, b0 + 4, dtype=np.uint8)[:, None, None]
        yield slab.reshape(4 * 256, 256, 3)


@pytest.mark.parametrize("cs", CSS)
def test_i410_carries_every_8_bit_colour_exactly(cs):
    """decode10(encode10(257 u8)) without resampling returns all 2^24 colours."""
    for frame in all_colours():
        y, u, v = S.encode10(T.p_from_u8(frame), cs, 444)
        back = S.decode(y, u, v, cs, 444, deep=True)
        assert np.array_equal(back[..., :3], frame), (cs, int(frame[0, 0, 0]))


@pytest.mark.parametrize("cs", CSS)
def test_i444_round_trip_stays_within_2_lsb_limited_and_1_lsb_full(cs):
    bound = 2 if cs in (Y.CS_BT601_LIMITED, Y.CS_BT709_LIMITED) else 1
    worst = 0
    for frame in all_colours():
        y, u, v = S.encode(frame, cs, 444)
        back = S.decode(y, u, v, cs, 444)
        worst = max(worst, int(np.abs(back[..., :3].astype(np.int16) - frame.astype(np.int16)).max()))
    print("I444 round trip, colour space", cs, "worst deviation", worst)
    assert worst <= bound


# ---- 4. the packing helpers ---------------------------------------------------------------------------------------------
def test_packed_byte_order():
    y = np.array([[1, 2, 3, 4]], np.uint8)
    u, v = np.array([[10, 11]], np.uint8), np.array([[20, 21]], np.uint8)
    assert S.to_yuy2(y, u, v).tolist() == [[1, 10, 2, 20, 3, 11, 4, 21]]
    assert S.to_uyvy(y, u, v).tolist() == [[10, 1, 20, 2, 11, 3, 21, 4]]
    for to, frm in ((S.to_yuy2, S.from_yuy2), (S.to_uyvy, S.from_uyvy)):
        assert all(np.array_equal(a, b) for a, b in zip(frm(to(y, u, v)), (y, u, v)))


@pytest.mark.parametrize("fmt", sorted(S.SAMPLING), ids=lambda f: S.FORMAT_NAMES[f])
def test_words_per_format(fmt):
    rng = np.random.default_rng(fmt)
    h, w = 4, 6
    deep = fmt in S.DEEP
    y, u, v = samples(rng, S.SAMPLING[fmt], h, w, deep)
    planes = S.to_words(fmt, y, u, v)
    ch, cw = S.chroma_shape(S.SAMPLING[fmt], h, w)
    shapes = {S.FMT_YUY2: [(h, 2 * w)], S.FMT_UYVY: [(h, 2 * w)], S.FMT_NV12: [(h, w), (ch, 2 * cw)],
              S.FMT_P010: [(h, w), (ch, 2 * cw)], S.FMT_P210: [(h, w), (ch, 2 * cw)]}.get(fmt, [(h, w), (ch, cw), (ch, cw)])
    assert [p.shape for p in planes] == shapes
    assert all(p.dtype == (np.uint16 if deep else np.uint8) for p in planes)
    assert [p.shape for p in S.blank_planes(fmt, h, w)] == shapes
    assert all(np.array_equal(a, b) for a, b in zip(S.from_words(fmt, planes), (y, u, v)))
    if fmt == S.FMT_P210:                                       # the value in the upper bits, U first
        assert np.array_equal(planes[0], y << 6) and np.array_equal(planes[1][:, 0::2], u << 6)
        assert np.array_equal(planes[1][:, 1::2], v << 6)
    if fmt in (S.FMT_I210, S.FMT_I410):                         # the value in the low bits
        assert np.array_equal(planes[0], y) and int(planes[1].max()) <= 1023


@pytest.mark.parametrize("fmt", [S.FMT_P210, S.FMT_I210, S.FMT_I410], ids=lambda f: S.FORMAT_NAMES[f])
def test_ignored_bits_are_ignored(fmt):
    rng = np.random.default_rng(40 + fmt)
    h, w = 6, 8
    y, u, v = samples(rng, S.SAMPLING[fmt], h, w, True)
    planes = S.to_words(fmt, y, u, v)
    shift = 0 if fmt == S.FMT_P210 else 10
    junk = [p | (rng.integers(1, 64, p.shape, dtype=np.uint16) << shift) for p in planes]
    assert all((a != b).all() for a, b in zip(junk, planes))
    assert all(np.array_equal(a, b) for a, b in zip(S.from_words(fmt, junk), (y, u, v)))
    assert np.array_equal(S.decode_planes(fmt, Y.CS_BT709_LIMITED, junk), S.decode_planes(fmt, Y.CS_BT709_LIMITED, planes))


def test_encode_planes_chooses_the_source():
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (4, 6, 4), dtype=np.uint8)
    state = (frame.astype(np.float32) / 255.0 - 0.5).astype(np.float16)
    cs = Y.CS_BT709_LIMITED
    from_frame = S.encode_planes(S.FMT_I410, cs, frame=frame)
    from_state = S.encode_planes(S.FMT_I410, cs, frame=frame, state=state)
    want = S.to_words(S.FMT_I410, *S.encode10(T.p_from_state(state), cs, 444))
    assert all(np.array_equal(a, b) for a, b in zip(from_state, want))
    assert not all(np.array_equal(a, b) for a, b in zip(from_state, from_frame))
    assert np.array_equal(S.encode_planes(S.FMT_YUY2, cs, frame=frame)[0], S.to_yuy2(*S.encode(frame, cs, 422)))


# ---- 5. header, binding, hook ---------------------------------------------------------------------------------------------
def test_header_constants_match_the_binding_and_the_definition():
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    want = {"YUY2": 16, "UYVY": 17, "I422": 18, "P210": 19, "I210": 20, "I444": 24, "I410": 25}
    for name, value in want.items():
        assert re.search(rf"\bJU_FMT_{name} = {value}\b", text), name
        assert getattr(R, "FMT_" + name) == getattr(S, "FMT_" + name) == value
    assert "no 4:2:2 / 4:4:4" not in text
    assert sorted(S.NEW_FORMATS) == sorted(want.values())


def test_the_hook_is_declared_and_exported_by_the_test_flavour_only(product_library, hip_library):
    assert "ju_debug_yuv_sampled" in R.HOOK_SYMBOLS
    assert hasattr(hip_library, "ju_debug_yuv_sampled") and not hasattr(product_library, "ju_debug_yuv_sampled")
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    assert re.search(r"JU_API\s+int\s+ju_debug_yuv_sampled\s*\(", test_header)
    assert "ju_debug_yuv_sampled" not in open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()


def test_the_hook_refuses_bad_arguments_without_a_gpu(hip_library):
    import ctypes
    planes, strides = (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)()
    call = hip_library.ju_debug_yuv_sampled
    assert call(0, R.FMT_YUY2, 0, 3, 4, None, 0, planes, strides) == 1      # odd width for 4:2:2
    assert b"even width" in hip_library.ju_last_error()
    assert call(0, R.FMT_NV12, 0, 4, 4, None, 0, planes, strides) == 1      # a 4:2:0 format
    assert call(0, 21, 0, 4, 4, None, 0, planes, strides) == 1              # no format
    assert call(2, R.FMT_I444, 0, 4, 4, None, 0, planes, strides) == 1      # op 2 with an 8-bit format
    assert b"10-bit" in hip_library.ju_last_error()
    assert call(0, R.FMT_I444, 0, 3, 3, None, 0, planes, strides) == 1      # (odd sizes pass for 4:4:4: the NULL image stops it)
    assert b"null" in hip_library.ju_last_error()


def test_host_frames_of_the_new_formats():
    h, w = 5, 8
    packed = np.zeros((h, 2 * w), np.uint8)
    f = R.host_frame(R.FMT_YUY2, [packed])
    assert (f.format, f.width, f.height, f.strides[0]) == (16, w, h, 2 * w) and f.planes[0] == packed.ctypes.data
    f = R.host_frame(R.FMT_UYVY, [np.zeros((h, 2 * w + 8), np.uint8)[::-1, :2 * w]])
    assert (f.format, f.width, f.strides[0]) == (17, w, -(2 * w + 8))
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_YUY2, [np.zeros((h, 2 * w + 2), np.uint8)])      # 2W with W odd
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_YUY2, [packed, packed])
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_YUY2, [np.zeros((h, 2 * w), np.uint16)])
    y, c = np.zeros((h, w), np.uint16), np.zeros((h, w // 2), np.uint16)
    f = R.host_frame(R.FMT_I210, [y, c, c[::-1]])
    assert (f.format, f.width, f.height) == (20, w, h) and (f.strides[0], f.strides[1], f.strides[2]) == (2 * w, w, -w)
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_I410, [np.zeros((h, w), np.uint8)] * 3)
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_I444, [np.zeros((h, 2 * w), np.uint8)[:, ::2]] * 3)   # columns not contiguous
    odd = [np.zeros((3, 5), np.uint8)] * 3
    f = R.host_frame(R.FMT_I444, odd)
    assert (f.width, f.height) == (5, 3)


def test_device_frames_default_to_dense_strides():
    w, h = 8, 5
    want = {R.FMT_YUY2: [2 * w], R.FMT_UYVY: [2 * w], R.FMT_I422: [w, w // 2, w // 2], R.FMT_P210: [2 * w, 2 * w],
            R.FMT_I210: [2 * w, w, w], R.FMT_I444: [w, w, w], R.FMT_I410: [2 * w, 2 * w, 2 * w]}
    for fmt, strides in want.items():
        f = R.device_frame(fmt, w, h, [4096 + 256 * k for k in range(len(strides))])
        assert f.format == fmt and f.location == R.LOC_DEVICE and (f.width, f.height) == (w, h)
        assert [f.strides[k] for k in range(len(strides))] == strides
        assert [f.planes[k] for k in range(len(strides))] == [4096 + 256 * k for k in range(len(strides))]
