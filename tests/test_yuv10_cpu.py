"""10-bit 4:2:0 frame I/O (P010 / I010) without a GPU: the numpy definition (tests/yuv10_reference.py) against the
real-valued formulas and the 8-bit definition, the 16-bit sample P of the f16 state in exact arithmetic, the bits the
formats ignore, the header constants, the test hook and the uint16 host frames of the binding."""

import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import yuv10_reference as T
import yuv_reference as Y
from helpers import ROOT
from joshupscale_amd import runtime as R

CSS = sorted(Y.COLORSPACE_NAMES)
LIMITED = (Y.CS_BT601_LIMITED, Y.CS_BT709_LIMITED)


def planes10(kind, h, w, rng):
    shapes = ((h, w), (h // 2, w // 2), (h // 2, w // 2))
    if kind == "random":
        return [rng.integers(0, 1024, s, dtype=np.uint16) for s in shapes]
    if kind == "zero":
        return [np.zeros(s, np.uint16) for s in shapes]
    if kind == "full":
        return [np.full(s, 1023, np.uint16) for s in shapes]
    cb = (np.indices(shapes[1]).sum(0) % 2 * 1023).astype(np.uint16)    # checkerboard chroma, luma random
    return [rng.integers(0, 1024, shapes[0], dtype=np.uint16), cb, (1023 - cb).astype(np.uint16)]


def decode10_real(y, u, v, cs):
    """float64 restatement: [H][W][3] B, G, R before rounding, clamped to 0..255."""
    kr, kb, kg, limited = Y._params(cs)
    oy, sy, sc = (64.0, 876.0, 896.0) if limited else (0.0, 1023.0, 1023.0)
    h, w = y.shape
    yl = (y.astype(np.float64) - oy) / sy
    cb = (Y.upsample8(u, h, w) / 8.0 - 512.0) / sc
    cr = (Y.upsample8(v, h, w) / 8.0 - 512.0) / sc
    r = yl + 2 * (1 - kr) * cr
    b = yl + 2 * (1 - kb) * cb
    g = yl - 2 * kb * (1 - kb) / kg * cb - 2 * kr * (1 - kr) / kg * cr
    return np.clip(np.stack([b, g, r], -1) * 255.0, 0.0, 255.0)


def encode10_real_planes(p, cs):
    """float64 restatement of encode10: (y, u, v) before rounding, clamped to 0..1023."""
    (ky, ku, kv), oy = T.encode10_real(cs)
    b, g, r = (p[..., k].astype(np.float64) / 65535.0 for k in range(3))
    y = oy + ky[0] * r + ky[1] * g + ky[2] * b

    def mean8(c):
        rows = c[0::2] + c[1::2]
        left = np.concatenate([rows[:, :1], rows[:, 1:-1:2]], axis=1)
        return (left + 2 * rows[:, 0::2] + rows[:, 1::2]) / 8.0
    mr, mg, mb = mean8(r), mean8(g), mean8(b)
    u = 512.0 + ku[0] * mr + ku[1] * mg + ku[2] * mb
    v = 512.0 + kv[0] * mr + kv[1] * mg + kv[2] * mb
    return [np.clip(x, 0.0, 1023.0) for x in (y, u, v)]


# ---- 1. decode10 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", CSS)
def test_decode10_follows_the_real_valued_formula(cs):
    rng = np.random.default_rng(10 + cs)
    for kind in ("random", "zero", "full", "checker"):
        y, u, v = planes10(kind, 46, 30, rng)
        got = T.decode10(y, u, v, cs)
        assert (got[..., 3] == 0).all()
        err = np.abs(got[..., :3].astype(np.float64) - decode10_real(y, u, v, cs)).max()
        print(f"decode10 cs {cs} {kind}: worst {err:.4f} code")
        assert err <= 0.5 + 0.02, (kind, err)
        # the kernel keeps these in 32-bit integers
        worst = max(int(np.abs(t).max()) for t in T.decode10_terms(y, u, v, cs))
        print(f"decode10 cs {cs} {kind}: largest accumulator {worst:.3e}")
        assert worst < 2 ** 31, (kind, worst)


@pytest.mark.parametrize("cs", CSS)
def test_decode10_accumulators_fit_32_bits_on_the_extreme_planes(cs):
    worst = 0
    for yv in (0, 1023):
        for uv in (0, 1023):
            for vv in (0, 1023):
                y = np.full((4, 4), yv, np.uint16)
                u, v = np.full((2, 2), uv, np.uint16), np.full((2, 2), vv, np.uint16)
                worst = max(worst, max(int(np.abs(t).max()) for t in T.decode10_terms(y, u, v, cs)))
    assert worst < 2 ** 31, worst


@pytest.mark.parametrize("cs", LIMITED)
def test_decode10_limited_black_and_white(cs):
    c = np.full((1, 1), 512, np.uint16)
    assert (T.decode10(np.full((2, 2), 64, np.uint16), c, c, cs)[..., :3] == 0).all()
    assert (T.decode10(np.full((2, 2), 940, np.uint16), c, c, cs)[..., :3] == 255).all()


# ---- 2. encode10 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", CSS)
def test_encode10_follows_the_real_valued_formula(cs):
    rng = np.random.default_rng(20 + cs)
    h, w = 46, 30
    sat = rng.choice(np.array([0, 65535], np.int64), (h, w, 3))         # saturated primaries, pixel by pixel
    for name, p in (("random", rng.integers(0, 65536, (h, w, 3))), ("saturated", sat)):
        got = T.encode10(p, cs)
        for plane, real in zip(got, encode10_real_planes(p, cs)):
            err = np.abs(plane.astype(np.float64) - real).max()
            print(f"encode10 cs {cs} {name}: worst {err:.5f} code")
            assert err <= 0.5 + 0.01, (name, err)


@pytest.mark.parametrize("cs", CSS)
def test_encode10_clamps_exactly_at_both_ends(cs):
    lo, hi = ((64, 512, 512), (940, 512, 512)) if cs in LIMITED else ((0, 512, 512), (1023, 512, 512))
    for value, want in ((0, lo), (65535, hi)):
        y, u, v = T.encode10(np.full((4, 6, 3), value, np.int64), cs)
        assert (y == want[0]).all() and (u == want[1]).all() and (v == want[2]).all(), (value, y[0, 0], u[0, 0], v[0, 0])
    # primaries never leave 0..1023
    for b in (0, 65535):
        for g in (0, 65535):
            for r in (0, 65535):
                p = np.empty((2, 2, 3), np.int64)
                p[...] = (b, g, r)
                for plane in T.encode10(p, cs):
                    assert plane.dtype == np.uint16 and int(plane.max()) <= 1023


def test_encode10_coefficients_fit_32_bits():
    for cs in CSS:
        rows, _ = T.encode10_coefficients(cs)
        assert all(abs(c) < 2 ** 26 for row in rows for c in row)


# ---- 3. the tie to the 8-bit definition ----------------------------------------------------------------------------
@pytest.mark.parametrize("cs", CSS)
def test_encode10_of_an_8_bit_frame_is_4_times_the_8_bit_encode(cs):
    """Real-valued, the 10-bit limited codes are exactly 4 x the 8-bit ones (64 = 4 x 16, 876 = 4 x 219, 896 = 4 x 224):
    the roundings leave 4 x 0.5 + 0.5 < 3, i.e. at most 2; full range scales by 1023 instead of 1020: 3 more."""
    rng = np.random.default_rng(30 + cs)
    bgrx = rng.integers(0, 256, (46, 30, 4), dtype=np.uint8)
    ten = T.encode10(T.p_from_u8(bgrx), cs)
    eight = Y.encode(bgrx, cs)
    bound = 2 if cs in LIMITED else 5
    for a, b in zip(ten, eight):
        d = np.abs(a.astype(np.int64) - 4 * b.astype(np.int64)).max()
        print(f"encode10(257 u8) - 4 encode(u8), cs {cs}: worst {d}")
        assert d <= bound, d


@pytest.mark.parametrize("cs", CSS)
def test_decode10_of_4_times_8_bit_planes_is_the_8_bit_decode(cs):
    rng = np.random.default_rng(40 + cs)
    h, w = 46, 30
    y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    ten = T.decode10(*(4 * p.astype(np.uint16) for p in (y, u, v)), cs)
    d = np.abs(ten.astype(np.int64) - Y.decode(y, u, v, cs).astype(np.int64)).max()
    print(f"decode10(4 x planes) - decode(planes), cs {cs}: worst {d}")
    assert d <= 1, d


# ---- 4. P from the f16 state ------------------------------------------------------------------------------------------
def test_p_from_state_is_exact_for_every_f16_in_range():
    bits = np.arange(0, 0x3800 + 1, dtype=np.uint16)                    # +0 .. +0.5: 14 337 bit patterns
    assert bits.size == 14337
    both = np.concatenate([bits, bits | 0x8000]).view(np.float16)       # and -0 .. -0.5
    assert float(both[14336]) == 0.5 and float(both[-1]) == -0.5
    got = T.p_from_state(both.reshape(-1, 1).repeat(3, axis=1))[:, 0]
    for s, p in zip(both, got):
        want = (Fraction(float(s)) + Fraction(1, 2)) * 65536
        want = min(max(want.numerator // want.denominator, 0), 65535)   # floor, saturated
        assert int(p) == want, (float(s), int(p), want)
    assert int(T.p_from_state(np.array([[-0.5] * 3], np.float16))[0, 0]) == 0
    assert int(T.p_from_state(np.array([[0.5] * 3], np.float16))[0, 0]) == 65535
    assert int(T.p_from_state(np.array([[0.0] * 3], np.float16))[0, 0]) == 32768
    assert int(T.p_from_state(np.array([[-0.0] * 3], np.float16))[0, 0]) == 32768
    # beyond the clip the sample saturates
    assert int(T.p_from_state(np.array([[0.75] * 3], np.float16))[0, 0]) == 65535
    assert int(T.p_from_state(np.array([[-0.75] * 3], np.float16))[0, 0]) == 0


def test_p_from_state_takes_float32_copies_of_f16_values():
    s16 = np.linspace(-0.5, 0.5, 777).astype(np.float16).reshape(-1, 1).repeat(4, axis=1)
    assert (T.p_from_state(s16) == T.p_from_state(s16.astype(np.float32))).all()


# ---- 5. the bits the formats ignore -----------------------------------------------------------------------------------
def test_ignored_bits_do_not_reach_the_frame():
    rng = np.random.default_rng(50)
    y, u, v = planes10("random", 18, 22, rng)
    want = T.decode10(y, u, v, Y.CS_BT709_LIMITED)
    yw, uvw = T.to_p010(y, u, v)
    assert (yw & 63 == 0).all() and (uvw & 63 == 0).all() and (uvw[:, 0::2] >> 6 == u).all()
    junk = lambda a: a | rng.integers(0, 64, a.shape, dtype=np.uint16)  # noqa: E731
    assert (T.decode10(*T.from_p010(junk(yw), junk(uvw)), Y.CS_BT709_LIMITED) == want).all()
    hi = lambda a: a | (rng.integers(0, 64, a.shape, dtype=np.uint16) << 10)  # noqa: E731
    planes = [hi(p) for p in T.to_i010(y, u, v)]
    assert any((p > 1023).any() for p in planes)
    assert (T.decode10(*T.from_i010(*planes), Y.CS_BT709_LIMITED) == want).all()
    for fmt in (T.FMT_P010, T.FMT_I010):
        back = T.from_words(fmt, T.to_words(fmt, y, u, v))
        assert all((a == b).all() for a, b in zip(back, (y, u, v)))


# ---- 6. header, binding, hook -----------------------------------------------------------------------------------------
def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    line = [ln for ln in text.splitlines() if "JU_FMT_BGRX = 0, JU_FMT_I420 = 1, JU_FMT_NV12 = 2" in ln]
    assert len(line) == 1 and "JU_FMT_P010 = 3" in line[0] and "JU_FMT_I010 = 4" in line[0]
    assert (R.FMT_P010, R.FMT_I010) == (T.FMT_P010, T.FMT_I010) == (3, 4)
    assert "hbd_from_state" in text
    assert not re.search(r"8-bit 4:2:0 only", text)


def test_the_hook_is_declared_and_exported_by_the_test_flavour_only(product_library, hip_library):
    assert "ju_debug_yuv10" in R.HOOK_SYMBOLS
    assert hasattr(hip_library, "ju_debug_yuv10") and not hasattr(product_library, "ju_debug_yuv10")
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    assert re.search(r"JU_API\s+int\s+ju_debug_yuv10\s*\(", test_header)
    product_header = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    assert "ju_debug_yuv10" not in product_header


def test_host_frames_take_uint16_planes():
    h, w = 6, 8
    y = np.zeros((h, w), np.uint16)
    uv = np.zeros((h // 2, w), np.uint16)
    f = R.host_frame(R.FMT_P010, [y, uv])
    assert (f.format, f.width, f.height) == (3, w, h)
    assert (f.strides[0], f.strides[1]) == (2 * w, 2 * w) and f.planes[0] == y.ctypes.data
    u, v = np.zeros((h // 2, w // 2), np.uint16), np.zeros((h // 2, w // 2), np.uint16)
    padded = np.zeros((h, w + 5), np.uint16)[:, :w]
    f = R.host_frame(R.FMT_I010, [padded, u[::-1], v], Y.CS_BT601_FULL)
    assert f.format == 4 and f.colorspace == Y.CS_BT601_FULL
    assert f.strides[0] == 2 * (w + 5) and f.strides[1] == -w and f.strides[2] == w      # bytes; bottom-up view
    assert f.planes[1] == u.ctypes.data + (h // 2 - 1) * w
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_P010, [y.astype(np.uint8), uv])
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_NV12, [y, uv])
    with pytest.raises(ValueError):
        R.host_frame(R.FMT_I010, [y[:, ::2], u, v])
    d = R.device_frame(R.FMT_P010, w, h, [1024, 4096])
    assert (d.strides[0], d.strides[1]) == (2 * w, 2 * w)
    d = R.device_frame(R.FMT_I010, w, h, [1024, 4096, 8192])
    assert (d.strides[0], d.strides[1], d.strides[2]) == (2 * w, w, w)


def test_the_hook_refuses_bad_arguments_without_a_gpu(hip_library):
    planes = (ctypes.c_void_p * 3)()
    strides = (ctypes.c_ssize_t * 3)()
    lib = hip_library
    assert lib.ju_debug_yuv10(0, 3, 0, 3, 4, None, 0, planes, strides) == 1          # odd width
    assert b"even" in lib.ju_last_error()
    assert lib.ju_debug_yuv10(0, 4, 0, 4, 5, None, 0, planes, strides) == 1          # odd height
    assert lib.ju_debug_yuv10(0, 3, 0, 4, 4, None, 0, planes, strides) == 1          # NULL buffers
    assert b"null" in lib.ju_last_error()
    assert lib.ju_debug_yuv10(0, 2, 0, 4, 4, None, 0, planes, strides) == 1          # NV12 is not a 10-bit format
    assert b"10-bit" in lib.ju_last_error()
    assert lib.ju_debug_yuv10(3, 3, 0, 4, 4, None, 0, planes, strides) == 1          # no such kernel
    buf = (ctypes.c_uint8 * 256)()
    base = ctypes.addressof(buf)
    planes[0], planes[1] = base + 1, base + 64                                       # an odd plane address
    strides[0], strides[1] = 8, 8
    assert lib.ju_debug_yuv10(0, 3, 0, 4, 4, base + 128, 16, planes, strides) == 1
    assert b"even addresses" in lib.ju_last_error()
    planes[0], strides[1] = base, 9                                                  # an odd stride
    assert lib.ju_debug_yuv10(0, 3, 0, 4, 4, base + 128, 16, planes, strides) == 1
    assert b"even addresses" in lib.ju_last_error()
    # a frame call without a runtime is refused before the format is looked at
    f = R.host_frame(R.FMT_P010, [np.zeros((2, 2), np.uint16), np.zeros((1, 2), np.uint16)])
    assert lib.ju_process_frame(None, f, f) == 1
