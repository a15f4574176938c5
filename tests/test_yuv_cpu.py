"""YUV frame I/O without a GPU: the numpy definition of the conversions (tests/yuv_reference.py), the ju_frame
layout and the exported entry points."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import yuv_reference as Y
from helpers import ROOT
from joshupscale_amd import runtime as R

ANCHORS = {  # x 65536: kY, kRV, kBU, kGU, kGV (the issue's table)
    Y.CS_BT601_LIMITED: (76309, 104597, 132201, 25675, 53279),
    Y.CS_BT601_FULL: (65536, 91881, 116130, 22553, 46802),
    Y.CS_BT709_LIMITED: (76309, 117489, 138438, 13975, 34925),
    Y.CS_BT709_FULL: (65536, 103206, 121609, 12276, 30679),
}
# Worst |channel| error of encode(decode(constant colour)) -> decode, over every constant Y/U/V the test sweeps: the
# round trip quantises twice (8-bit BGR, then 8-bit YUV), and limited range stretches one YUV step over ~1.16 BGR steps.
# Found by this sweep: 2 LSB in limited range, 1 LSB in full range
ROUND_TRIP_BOUND = 2


@pytest.mark.parametrize("cs", sorted(ANCHORS))
def test_decode_coefficients_match_the_anchors(cs):
    k, oy = Y.decode_coefficients(cs)
    assert k == ANCHORS[cs]
    assert oy == (16 if cs in (Y.CS_BT601_LIMITED, Y.CS_BT709_LIMITED) else 0)


def test_no_coefficient_falls_on_a_tie():
    for cs in ANCHORS:
        kr, kb = (0.299, 0.114) if cs < 2 else (0.2126, 0.0722)
        # round_half_away only matters at exact .5: none of the real products is within 1e-6 of one
        limited = cs in (0, 2)
        s = 255 / 224 if limited else 1.0
        kg = 1 - kr - kb
        for k in [255 / 219, 2 * (1 - kr) * s, 2 * (1 - kb) * s, 2 * kb * (1 - kb) / kg * s, 2 * kr * (1 - kr) / kg * s]:
            frac = (k * 65536) % 1
            assert abs(frac - 0.5) > 1e-6


def test_full_range_601_grey_is_exact():
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    c = np.full((8, 8), 128, np.uint8)
    out = Y.decode(y, c, c, Y.CS_BT601_FULL)
    for ch in range(3):
        assert (out[..., ch] == y).all()
    assert (out[..., 3] == 0).all()


@pytest.mark.parametrize("cs", [Y.CS_BT601_LIMITED, Y.CS_BT709_LIMITED])
def test_limited_range_black_and_white(cs):
    c = np.full((1, 1), 128, np.uint8)
    assert (Y.decode(np.full((2, 2), 16, np.uint8), c, c, cs)[..., :3] == 0).all()
    assert (Y.decode(np.full((2, 2), 235, np.uint8), c, c, cs)[..., :3] == 255).all()
    # and back: black and white encode to 16 / 235 with neutral chroma
    for v, want in ((0, 16), (255, 235)):
        yy, u, vv = Y.encode(np.full((2, 2, 4), v, np.uint8), cs)
        assert (yy == want).all() and (u == 128).all() and (vv == 128).all()


@pytest.mark.parametrize("cs", sorted(ANCHORS))
def test_constant_colour_round_trip_is_bounded(cs):
    """decode(Y,U,V) -> BGR -> encode -> decode again: the BGR of both decodes differ by at most ROUND_TRIP_BOUND."""
    worst = 0
    lo, hi = (16, 235) if cs in (0, 2) else (0, 255)
    clo, chi = (16, 240) if cs in (0, 2) else (0, 255)
    for yv in range(lo, hi + 1, 9):
        for uv in range(clo, chi + 1, 28):
            for vv in range(clo, chi + 1, 28):
                y = np.full((4, 4), yv, np.uint8)
                u, v = np.full((2, 2), uv, np.uint8), np.full((2, 2), vv, np.uint8)
                bgr = Y.decode(y, u, v, cs)
                y2, u2, v2 = Y.encode(bgr, cs)
                bgr2 = Y.decode(y2, u2, v2, cs)
                worst = max(worst, int(np.abs(bgr2[..., :3].astype(int) - bgr[..., :3].astype(int)).max()))
    assert worst <= ROUND_TRIP_BOUND, worst


def test_in_gamut_grey_round_trips_exactly_in_full_range():
    for v in range(256):
        bgrx = np.full((4, 6, 4), v, np.uint8)
        y, u, vv = Y.encode(bgrx, Y.CS_BT601_FULL)
        assert (y == v).all() and (u == 128).all() and (vv == 128).all()


def test_edges_clamp_with_odd_chroma_counts():
    """30 x 46 luma -> 15 x 23 chroma: the last chroma column / row repeat; column 2i - 1 of the encoder clamps to 0."""
    rng = np.random.default_rng(3)
    h, w = 46, 30
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    up = Y.upsample8(u, h, w)
    assert up.shape == (h, w)
    # last (odd) column: Cv(i) + Cv(i + 1) with i + 1 clamped = 2 Cv(i); first / last rows: C[jn] clamped = C[j]
    assert (up[:, -1] == up[:, -2]).all()
    assert up[0, 0] == 8 * int(u[0, 0]) and up[-1, 0] == 8 * int(u[-1, 0])
    # a brute-force restatement of the siting formulas, index by index
    for yy in (0, 1, 2, h - 2, h - 1):
        for xx in (0, 1, 2, w - 2, w - 1):
            j = yy >> 1
            jn = min(max(j - 1 if yy % 2 == 0 else j + 1, 0), h // 2 - 1)
            cv = lambda i: 3 * int(u[j, min(i, w // 2 - 1)]) + int(u[jn, min(i, w // 2 - 1)])  # noqa: E731
            i = xx >> 1
            assert up[yy, xx] == (2 * cv(i) if xx % 2 == 0 else cv(i) + cv(i + 1))
    out = Y.decode(y, u, v, Y.CS_BT709_LIMITED)
    assert out.shape == (h, w, 4)
    bgrx = out
    y2, u2, v2 = Y.encode(bgrx, Y.CS_BT709_LIMITED)
    assert y2.shape == (h, w) and u2.shape == (h // 2, w // 2) and v2.shape == u2.shape
    # cell 0: columns -1 (clamped to 0), 0, 1 -> 3 * px(0) + px(1) per row
    ((_, _, _), (cur, cug, cub), _), _ = Y.encode_coefficients(Y.CS_BT709_LIMITED)
    s = [3 * bgrx[0:2, 0, c].astype(int).sum() + bgrx[0:2, 1, c].astype(int).sum() for c in (2, 1, 0)]
    want = min(255, max(0, 128 + ((cur * s[0] + cug * s[1] + cub * s[2] + (1 << 18)) >> 19)))
    assert u2[0, 0] == want


def test_nv12_interleave_round_trips():
    rng = np.random.default_rng(0)
    u = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    v = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    uv = Y.to_nv12(u, v)
    assert uv.shape == (3, 10) and (uv[:, 0] == u[:, 0]).all() and (uv[:, 1] == v[:, 0]).all()
    u2, v2 = Y.from_nv12(uv)
    assert (u2 == u).all() and (v2 == v).all()


def test_odd_sizes_are_refused_by_the_reference():
    with pytest.raises(ValueError):
        Y.encode(np.zeros((3, 4, 4), np.uint8), 0)


def test_frame_struct_matches_the_header(tmp_path):
    """ju_frame's layout as the system compiler sees include/joshupscale_amd.h."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "joshupscale_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ju_frame), '
                   'offsetof(ju_frame, format), offsetof(ju_frame, colorspace), offsetof(ju_frame, location), '
                   'offsetof(ju_frame, width), offsetof(ju_frame, height), offsetof(ju_frame, planes), '
                   'offsetof(ju_frame, strides)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = R.JuFrame
    want = [ctypes.sizeof(F), F.format.offset, F.colorspace.offset, F.location.offset, F.width.offset, F.height.offset,
            F.planes.offset, F.strides.offset]
    assert got == want, (got, want)


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    assert "JU_FMT_BGRX = 0, JU_FMT_I420 = 1, JU_FMT_NV12 = 2" in text
    assert (R.FMT_BGRX, R.FMT_I420, R.FMT_NV12) == (Y.FMT_BGRX, Y.FMT_I420, Y.FMT_NV12) == (0, 1, 2)
    assert (R.CS_BT601_LIMITED, R.CS_BT601_FULL, R.CS_BT709_LIMITED, R.CS_BT709_FULL) == (0, 1, 2, 3)


def test_product_library_exports_the_frame_calls(product_library, hip_library):
    for lib in (product_library, hip_library):
        assert hasattr(lib, "ju_process_frame") and hasattr(lib, "ju_enqueue_frame")
    assert hasattr(hip_library, "ju_debug_yuv") and not hasattr(product_library, "ju_debug_yuv")


def test_frame_calls_refuse_null_arguments_without_a_gpu(hip_library):
    f = R.JuFrame()
    assert hip_library.ju_process_frame(None, None, None) == 1          # JU_ERR_INVALID_ARGUMENT
    assert hip_library.ju_enqueue_frame(None, f, f) == 1
    planes = (ctypes.c_void_p * 3)()
    strides = (ctypes.c_ssize_t * 3)()
    assert hip_library.ju_debug_yuv(0, 1, 0, 3, 4, None, 0, planes, strides) == 1   # odd width
    assert b"even" in hip_library.ju_last_error()
    assert hip_library.ju_debug_yuv(0, 0, 0, 4, 4, None, 0, planes, strides) == 1   # BGRX is not a YUV format
