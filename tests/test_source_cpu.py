"""The source stage without a GPU: the integer definition of the scaler and of the masked pass-through
(tests/source_reference.py; docs/source_stage.md) against their own invariants, a float64 evaluation of the same filter,
Pillow's BILINEAR and the reference's mask.png; the new entry points; the limits' message in C and in Python."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import source_reference as S
from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_MASK = os.path.join(ROOT, "tests", "golden", "obs_mask.png")

# (source extent, model extent) of one axis: the sizes of the GPU tests, the flagship ratios, the ratio limits both ways
AXES = [(30, 16), (46, 24), (17, 16), (23, 24), (8, 16), (12, 24), (16, 16), (256, 16), (384, 24), (33, 16), (49, 24),
        (64, 16), (1920, 480), (1080, 270), (1280, 480), (720, 270), (272, 270), (48, 30), (72, 48),
        (2, 32), (32, 2), (8192, 512), (512, 8192), (8191, 512), (7679, 480), (100, 7)]


def smooth(h, w):
    y, x = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 0] = (127.5 + 127.5 * np.sin(x / 37.0 + y / 91.0)).astype(np.uint8)
    img[..., 1] = (127.5 + 127.5 * np.cos(x / 53.0 - y / 29.0)).astype(np.uint8)
    img[..., 2] = (x * 255) // max(w - 1, 1)
    img[..., 3] = 255
    return img


def noise(h, w, seed=11):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


@pytest.mark.parametrize("n,m", AXES)
def test_every_table_row_sums_to_4096_and_holds_at_most_33_taps(n, m):
    start, count, taps = S.axis_table(n, m)
    assert (taps.sum(1) == 4096).all() and (taps >= 0).all()
    assert 1 <= count.min() and count.max() <= S.MAX_TAPS
    assert (start >= 0).all() and (start + count <= n).all()
    assert (np.diff(start) >= 0).all() and (np.diff(start + count) >= 0).all()    # (what the kernel's tile span relies on)
    for d in range(m):
        assert (taps[d, count[d]:] == 0).all()


def test_the_ratio_limits_reach_but_do_not_pass_33_taps():
    """Downscaling by 16 is the widest support: 2 * 16 source samples wide, at most 33 integer positions."""
    most = max(int(S.axis_table(n, m)[1].max()) for n, m in [(8192, 512), (32, 2), (7679, 480), (8191, 512)])
    assert 32 <= most <= S.MAX_TAPS
    assert int(S.axis_table(2, 32)[1].max()) <= 2


def test_equal_sizes_are_the_identity():
    for (h, w) in [(16, 24), (30, 48), (2, 2), (7, 301)]:
        src = noise(h, w)
        out = S.scale(src, h, w)
        assert np.array_equal(out[..., :3], src[..., :3]) and (out[..., 3] == 0).all()


def test_an_all_255_frame_stays_within_32_bits_and_stays_255():
    """255 * 4096 * 4096 + 2^23 < 2^32: scale() asserts the accumulator bound; rows summing to exactly 4096 keep white white."""
    assert 255 * 4096 * 4096 + (1 << 23) < 1 << 32
    for (h, w, mh, mw) in [(30, 46, 16, 24), (8, 12, 16, 24), (256, 384, 16, 24), (32, 16, 2, 256)]:
        out = S.scale(np.full((h, w, 4), 255, np.uint8), mh, mw)
        assert (out[..., :3] == 255).all() and (out[..., 3] == 0).all()
        assert (S.scale(np.zeros((h, w, 4), np.uint8), mh, mw) == 0).all()


@pytest.mark.parametrize("h,w,mh,mw", [(108, 192, 27, 48), (30, 46, 16, 24), (17, 23, 16, 24), (8, 12, 16, 24), (256, 384, 16, 24),
                                       (33, 49, 16, 24), (48, 72, 30, 48), (272, 480, 270, 480)])
def test_the_integer_scaler_against_the_same_filter_in_float64(h, w, mh, mw):
    """|integer result - float64 value| <= 0.5 + 255 ((Ty - 1) + (Tx - 1)) / 4096, T the most taps of an axis' rows.

    Per row of an axis the true coefficients are c_i = w_i / S and the table holds q_i / 4096 = c_i - e_i / 4096 with
    0 <= e_i < 1 for every tap but the largest, which also receives the remainder sum(e) / 4096: the errors sum to 0.
    So sum_i (q_i / 4096 - c_i) x_i = sum_{i != largest} (-e_i / 4096) (x_i - x_largest), at most 255 (T - 1) / 4096 in
    size for 8-bit x.  The two axes compose as convex combinations (either set of coefficients is non-negative and sums
    to 1), so their bounds add; nothing is rounded between the axes; the final >> 24 after + 2^23 rounds to nearest, 0.5."""
    for src in (smooth(h, w), noise(h, w)):
        got = S.scale(src, mh, mw)[..., :3].astype(np.float64)
        want = S.scale_float(src, mh, mw)
        ty, tx = int(S.axis_table(h, mh)[1].max()), int(S.axis_table(w, mw)[1].max())
        bound = 0.5 + 255.0 * ((ty - 1) + (tx - 1)) / 4096.0
        worst = float(np.abs(got - want).max())
        print(f"{h}x{w} -> {mh}x{mw}: |int - float64| max {worst:.4f}, bound {bound:.4f} (taps {ty}, {tx})")
        assert worst <= bound + 1e-9


# Pillow computes the same triangle coefficients but runs two passes with the intermediate image rounded to 8 bits and
# its own coefficient precision, so equality is not expected.  Measured with Pillow 12.2.0 on the twelve cases below
# (smooth and noise clip at each size): the largest difference is 1 LSB, in eleven of the twelve (272x480 smooth: 0).
# Asserted: that value plus 1 LSB.
PILLOW_MEASURED_MAX = 1


@pytest.mark.parametrize("h,w,mh,mw", [(1080, 1920, 270, 480), (720, 1280, 270, 480), (272, 480, 270, 480),
                                       (30, 46, 16, 24), (17, 23, 16, 24), (8, 12, 16, 24)])
def test_against_pillows_bilinear_resize(h, w, mh, mw):
    Image = pytest.importorskip("PIL.Image")
    for name, src in (("smooth", smooth(h, w)), ("noise", noise(h, w))):
        got = S.scale(src, mh, mw)[..., :3].astype(np.int64)
        rgb = np.ascontiguousarray(src[..., 2::-1])
        pil = np.asarray(Image.fromarray(rgb).resize((mw, mh), Image.BILINEAR))[..., ::-1].astype(np.int64)
        worst = int(np.abs(got - pil).max())
        print(f"{h}x{w} -> {mh}x{mw} {name}: max |ours - Pillow| = {worst}")
        assert worst <= PILLOW_MEASURED_MAX + 1


def test_the_blend_on_hand_made_pixels():
    gen = np.array([[[10, 20, 30, 0], [200, 100, 0, 0], [255, 255, 255, 0], [1, 2, 3, 77]]], np.uint8)
    src = np.array([[[250, 40, 31, 9], [0, 101, 255, 9], [0, 0, 0, 9], [9, 9, 9, 9]]], np.uint8)
    white = np.full((1, 4, 4), 255, np.uint8)
    black = np.zeros((1, 4, 4), np.uint8)
    grey = np.full((1, 4, 4), 128, np.uint8)
    assert np.array_equal(S.blend(gen, src, white), gen)                      # (a == 0: not rewritten, X kept)
    out = S.blend(gen, src, black)
    assert np.array_equal(out[..., :3], src[..., :3]) and (out[..., 3] == 0).all()
    out = S.blend(gen, src, grey)                                             # a = 381, 765 - a = 384
    want = (src[..., :3].astype(int) * 381 + gen[..., :3].astype(int) * 384 + 382) // 765
    assert np.array_equal(out[..., :3], want) and (out[..., 3] == 0).all()
    assert np.abs(want - (src[..., :3].astype(int) + gen[..., :3].astype(int)) / 2.0).max() <= 1.0   # the rounded mean
    # the mask's X is ignored; a mask and a source of their own sizes are point sampled at the pixel centres
    mask = np.array([[[255, 255, 255, 0], [0, 0, 0, 255]]], np.uint8)          # left half shows gen, right half the source
    src2 = np.array([[[7, 7, 7, 0]], [[9, 9, 9, 0]]], np.uint8)               # 2 rows x 1 column
    gen2 = np.full((4, 4, 4), 100, np.uint8)
    out = S.blend(gen2, src2, mask)
    assert (out[:, :2] == 100).all()
    assert (out[:2, 2:, :3] == 7).all() and (out[2:, 2:, :3] == 9).all() and (out[:, 2:, 3] == 0).all()
    assert list(S.texel(np.arange(5), 3, 5)) == [0, 0, 1, 2, 2]


def test_the_blend_through_the_references_mask():
    """obs_plugin/data/mask.png (880 bytes, 1920x1440, 1-bit): black and white only, the black inside rows 82..325, columns
    1488..1821.  (Inside that box the file holds three black rectangles, 33557 pixels, not one filled box.)  Exactly the
    pixels under black mask texels come from the source."""
    assert os.path.getsize(GOLDEN_MASK) == 880
    mask = S.read_png_palette_1bit(GOLDEN_MASK)
    assert mask.shape == (1440, 1920, 4)
    assert (np.unique(mask[..., :3]) == [0, 255]).all()
    dark = mask[..., :3].astype(int).sum(-1) == 0
    assert (mask[..., :3].astype(int).sum(-1)[~dark] == 765).all()
    rows, cols = np.flatnonzero(dark.any(1)), np.flatnonzero(dark.any(0))
    assert (rows[0], rows[-1], cols[0], cols[-1]) == (82, 325, 1488, 1821) and dark.sum() == 33557
    # at the mask's own size, with a source of a quarter of it
    rng = np.random.default_rng(5)
    gen = rng.integers(0, 256, (1440, 1920, 4), dtype=np.uint8)
    gen[..., 3] = 0
    src = rng.integers(0, 256, (360, 480, 4), dtype=np.uint8)
    out = S.blend(gen, src, mask)
    assert np.array_equal(out[~dark], gen[~dark])
    up = src[np.arange(1440)[:, None] // 4, np.arange(1920)[None, :] // 4]
    assert np.array_equal(out[dark][:, :3], up[dark][:, :3]) and (out[dark][:, 3] == 0).all()
    # at the small model's output (120 x 192): the output pixels whose centre falls on a black texel
    gen = rng.integers(0, 256, (120, 192, 4), dtype=np.uint8)
    src = rng.integers(0, 256, (30, 48, 4), dtype=np.uint8)
    out = S.blend(gen, src, mask)
    hit = dark[(2 * np.arange(120)[:, None] + 1) * 1440 // 240, (2 * np.arange(192)[None, :] + 1) * 1920 // 384]
    assert 0 < hit.sum() < 21 * 34 and hit[7:27, 149:182].sum() == hit.sum()   # (inside the box, scaled by 1 / 12 and 1 / 10)
    assert np.array_equal(out[~hit], gen[~hit])
    assert np.array_equal(out[hit][:, :3], src[np.arange(120)[:, None] // 4, np.arange(192)[None, :] // 4][hit][:, :3])
    assert (out[hit][:, 3] == 0).all()


def test_new_entry_points_are_declared_and_exported(hip_library, product_library):
    header = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    for name in ("ju_set_source_size", "ju_get_source_size", "ju_set_source_mask"):
        assert re.search(r"JU_API\s+int\s+" + name + r"\s*\(", header)
        assert name in R.PRODUCT_SYMBOLS
        assert hasattr(product_library, name) and hasattr(hip_library, name)
    assert re.search(r"JU_SCALE_TRIANGLE\s*=\s*0", header) and R.SCALE_TRIANGLE == 0
    assert re.search(r"JU_API\s+int\s+ju_debug_source\s*\(", test_header)
    assert "ju_debug_source" in R.HOOK_SYMBOLS
    assert hasattr(hip_library, "ju_debug_source") and not hasattr(product_library, "ju_debug_source")
    for name in ("set_source_size", "get_source_size", "set_source_mask"):
        assert callable(getattr(R.Runtime, name)) and callable(getattr(R.Session, name))


def c_limit_message(lib, sw, sh, mw, mh):
    rc = lib.ju_debug_source(2, None, 0, mw, mh, None, 0, sw, sh, None, 0, 0, 0)
    return rc, lib.ju_last_error().decode() if rc else ""


def test_the_limits_and_their_message_match_between_c_and_python(hip_library):
    assert (S.AXIS_MIN, S.AXIS_MAX, S.RATIO_MAX) == (R.SOURCE_AXIS_MIN, R.SOURCE_AXIS_MAX, R.SOURCE_RATIO_MAX)
    model = (48, 30)
    good = [(48, 30), (72, 48), (768, 480), (3, 2), (46, 30), (767, 31)]
    bad = [(2, 2), (769, 30), (48, 481), (1, 30), (48, 1), (0, 30), (48, 0), (8193, 8192), (2, 1), (10 ** 6, 30)]
    for (sw, sh) in good:
        assert R.source_size_problem(sw, sh, *model) == ""
        assert c_limit_message(hip_library, sw, sh, *model) == (0, "")
    for (sw, sh) in bad:
        text = R.source_size_problem(sw, sh, *model)
        assert text.startswith(f"source size {sw}x{sh}: ") and "48x30" in text
        rc, message = c_limit_message(hip_library, sw, sh, *model)
        assert rc == 1                                                        # JU_ERR_INVALID_ARGUMENT
        assert message == "std::invalid_argument: ju_set_source_size: " + text
    # a big model: the axis cap binds before the ratio does; a small axis: the ratio binds both ways
    assert R.source_size_problem(8192, 8192, 8192, 8192) == "" and R.source_size_problem(8193, 8192, 8192, 8192) != ""
    assert c_limit_message(hip_library, 8192, 8192, 8192, 8192)[0] == 0
    assert R.source_size_problem(2, 2, 33, 2) != "" and c_limit_message(hip_library, 2, 2, 33, 2)[0] == 1
    assert R.source_size_problem(2, 2, 32, 2) == "" and c_limit_message(hip_library, 2, 2, 32, 2)[0] == 0
