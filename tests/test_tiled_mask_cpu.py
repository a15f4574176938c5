"""A tiled frame under a source mask without a GPU (docs/tiled.md "A mask"): the properties of the numpy definition
(tests/tiled_mask_reference.py) over the geometries and the masks the GPU tests use -- white, black, one tile, the source
texel -- the box against the pixels it has to cover, csrc/mask_box.h against the box from a stand-alone host program under
the address and undefined-behaviour sanitizers and through the no-device hook, the refusals' words, the declared surface."""

import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import source_reference as S
import tiled_mask_reference as TM
import tiled_reference as T
from helpers import ROOT
from joshupscale_amd import runtime as R
from test_tiled_output_cpu import GEOMETRIES, H, W, tiles_of

JU_ERR_INVALID_ARGUMENT = 1
OBS = os.path.join(ROOT, "tests", "golden", "obs_mask.png")

_SOURCES, _MASKS, _OBS = {}, {}, []


def source_of(sw, sh):
    """The source frame of one geometry (X random: the blend writes 0), computed once."""
    if (sw, sh) not in _SOURCES:
        src = np.random.default_rng(31 + sw * 100 + sh).integers(0, 256, (sh, sw, 4), dtype=np.uint8)
        src.setflags(write=False)
        _SOURCES[(sw, sh)] = src
    return _SOURCES[(sw, sh)]


def obs_mask():
    if not _OBS:
        m = S.read_png_palette_1bit(OBS)
        m.setflags(write=False)
        _OBS.append(m)
    return _OBS[0]


def seam(S_, t, ov):
    """The blended coordinate in the middle of the first seam of one axis (the frame's middle where there is one tile)."""
    _, first, q = T.layout(S_, t, ov)
    at = np.flatnonzero(q) if ov else np.flatnonzero(np.diff(first)) + 1
    return int(at[at.size // 2]) if at.size else 2 * S_


def grey(rng, mh, mw):
    """Random grey levels per channel, with white and black texels among them: a takes values across 0 .. 765."""
    m = rng.integers(0, 256, (mh, mw, 4), dtype=np.uint8)
    pick = rng.integers(0, 8, (mh, mw))
    m[pick == 0, :3] = 255
    m[pick == 1, :3] = 0
    return m


def masks_of(sw, sh, ov):
    """{name: mask} of one geometry, computed once: the masks of the issue's list."""
    key = (sw, sh, ov)
    if key in _MASKS:
        return _MASKS[key]
    B, Bh = 4 * sw, 4 * sh
    rng = np.random.default_rng(17 + sw * 1000 + sh * 10 + ov)
    white = np.full((5, 9, 4), 255, np.uint8)
    white[..., 3] = rng.integers(0, 256, (5, 9))                      # (X is ignored)
    black = np.zeros((3, 2, 4), np.uint8)
    black[..., 3] = 255
    # a black rectangle across the first seam of each axis -- a ramp and, where both axes have one, a four-tile corner --
    # its edges not multiples of 4
    cx, cy = seam(sw, W, ov), seam(sh, H, ov)
    x0, x1, y0, y1 = max(cx - 9, 1), min(cx + 10, B - 1), max(cy - 7, 1), min(cy + 6, Bh - 1)
    x0, x1, y0, y1 = x0 + (x0 % 4 == 0), x1 - (x1 % 4 == 0), y0 + (y0 % 4 == 0), y1 - (y1 % 4 == 0)
    assert all(v % 4 for v in (x0, x1, y0, y1)) and x0 < cx < x1 and y0 < cy < y1
    rect = np.full((Bh, B, 4), 255, np.uint8)
    rect[y0:y1, x0:x1, :3] = 0
    corners = np.full((Bh // 2, B // 2, 4), 255, np.uint8)
    for y, x, v in ((0, 0, (254, 255, 255)), (0, -1, (255, 0, 255)), (-1, 0, (255, 255, 128)), (-1, -1, (0, 0, 0))):
        corners[y, x, :3] = v
    masks = {"white": white, "black": black, "grey-blended": grey(rng, Bh, B), "grey-source": grey(rng, sh, sw),
             "grey-7x5": grey(rng, 5, 7), "grey-larger": grey(rng, 3 * Bh, 2 * B + 1), "rectangle": rect, "corners": corners,
             "grey-1x1": np.array([[[200, 100, 7, 0]]], np.uint8), "obs": obs_mask()}
    for m in masks.values():
        m.setflags(write=False)
    _MASKS[key] = masks
    return masks


def alpha(mask, B, Bh):
    ys, xs = S.texel(np.arange(Bh), mask.shape[0], Bh), S.texel(np.arange(B), mask.shape[1], B)
    return 765 - mask[ys[:, None], xs[None, :], :3].astype(np.int64).sum(-1)


def test_the_masks_reach_every_branch():
    for sw, sh, ov in GEOMETRIES:
        B, Bh = 4 * sw, 4 * sh
        masks = masks_of(sw, sh, ov)
        assert len(masks) == 10
        for name in ("grey-blended", "grey-source", "grey-7x5", "grey-larger"):
            a = alpha(masks[name], B, Bh)
            assert a.min() == 0 and a.max() == 765 and len(np.unique(a)) > (20 if name == "grey-7x5" else 300), name
            assert TM.box(masks[name], B, Bh) == (0, 0, B, Bh), name           # the box is the whole frame
        larger = masks["grey-larger"]
        assert larger.shape[1] > B and len(np.unique(S.texel(np.arange(B), larger.shape[1], B))) < larger.shape[1]
        x0, y0, x1, y1 = TM.box(masks["rectangle"], B, Bh)
        assert all(v % 4 for v in (x0, y0, x1, y1)) and (x1 - x0) * (y1 - y0) < B * Bh // 4
        assert TM.box(masks["corners"], B, Bh) == (0, 0, B, Bh)
        a = alpha(masks["corners"], B, Bh)
        assert np.count_nonzero(a) == 16 and a[0, 0] == 1 and a[-1, -1] == 765   # (a 2 x 2 block of pixels per texel)
        a = alpha(masks["grey-1x1"], B, Bh)
        assert (a == 765 - 307).all()


@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_white_is_the_blend_and_black_is_the_source_in_blocks(sw, sh, ov):
    tiles, src, masks = tiles_of(sw, sh, ov), source_of(sw, sh), masks_of(sw, sh, ov)
    blended = T.stitch(tiles, sw, sh, W, H, ov)
    assert np.array_equal(TM.masked(tiles, src, masks["white"], W, H, ov), blended)
    assert np.array_equal(TM.masked(tiles, src, None, W, H, ov), blended)
    want = np.repeat(np.repeat(src, 4, 0), 4, 1).copy()              # the source, point sampled: 4 x 4 blocks
    want[..., 3] = 0
    assert np.array_equal(TM.masked(tiles, src, masks["black"], W, H, ov), want)
    got = TM.masked(tiles, src, masks["grey-blended"], W, H, ov)
    assert not got[..., 3].any() and not np.array_equal(got, blended) and not np.array_equal(got, want)
    # under an output size: the mask first, the scale behind it
    import scale_filter_reference as F
    assert np.array_equal(TM.frame8(tiles, src, masks["rectangle"], W, H, ov, 3 * sh + 1, 3 * sw - 1, F.MITCHELL),
                          F.scale8(TM.masked(tiles, src, masks["rectangle"], W, H, ov), 3 * sh + 1, 3 * sw - 1, F.MITCHELL))


def test_the_source_texel_of_a_blended_pixel_is_a_shift():
    """floor((2 X + 1) Ws / (2 B)) == X >> 2 for B = 4 Ws, every Ws <= 3840: what the kernels use."""
    for ws in range(1, 3841):
        x = np.arange(4 * ws)
        assert np.array_equal(S.texel(x, ws, 4 * ws), x >> 2), ws


def test_one_tile_is_the_plain_blend_of_that_tile():
    sw, sh, ov = 48, 30, 7
    tiles, src = tiles_of(sw, sh, ov), source_of(sw, sh)
    assert len(tiles) == 1
    gen = tiles[0].copy()
    gen[..., 3] = 0                                                   # (what ju_process hands to the plain runtime's blend)
    for name, mask in masks_of(sw, sh, ov).items():
        assert np.array_equal(TM.masked(tiles, src, mask, W, H, ov), S.blend(gen, src, mask)), name


@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_the_box_covers_every_pixel_the_mask_touches_and_is_empty_exactly_without_one(sw, sh, ov):
    B, Bh = 4 * sw, 4 * sh
    empty = []
    for name, mask in masks_of(sw, sh, ov).items():
        x0, y0, x1, y1 = TM.box(mask, B, Bh)
        a = alpha(mask, B, Bh)
        outside = np.ones((Bh, B), bool)
        outside[y0:y1, x0:x1] = False
        assert not a[outside].any(), name                             # coverage: all that correctness rests on
        assert 0 <= x0 <= x1 <= B and 0 <= y0 <= y1 <= Bh
        assert ((x0, y0, x1, y1) == (0, 0, 0, 0)) == (not a.any()), name
        if not a.any():
            empty.append(name)
    assert empty == ["white"]
    # a mask larger than the frame whose only non-white texels are never sampled: empty too
    mask = np.full((3 * Bh, 2 * B + 1, 4), 255, np.uint8)
    sampled_y, sampled_x = S.texel(np.arange(Bh), 3 * Bh, Bh), S.texel(np.arange(B), 2 * B + 1, B)
    free_y = np.setdiff1d(np.arange(3 * Bh), sampled_y)
    free_x = np.setdiff1d(np.arange(2 * B + 1), sampled_x)
    assert free_y.size and free_x.size
    mask[free_y, :, :3] = 0
    mask[:, free_x, :3] = 7
    assert TM.box(mask, B, Bh) == (0, 0, 0, 0) and not alpha(mask, B, Bh).any()


def test_the_obs_mask_leaves_most_of_the_frame_outside_the_box():
    mask = obs_mask()
    assert mask.shape == (1440, 1920, 4)
    rows, cols = np.nonzero(mask[..., :3].sum(-1) != 765)
    assert (rows.min(), rows.max(), cols.min(), cols.max()) == (82, 325, 1488, 1821)
    x0, y0, x1, y1 = TM.box(mask, 400, 280)
    assert 0 < (x1 - x0) * (y1 - y0) < 400 * 280 // 10               # both sides of the kernels' box test run
    bx = TM.box(mask, 3840, 2160)
    assert (bx[2] - bx[0]) * (bx[3] - bx[1]) < 3840 * 2160 // 10


# ---- csrc/mask_box.h against box() ----------------------------------------------------------------------------------------
def box_cases():
    """(mask, stride in bytes, B, Bh): every mask of every geometry, dense, padded and bottom-up in rotation, and sizes at
    which a texel run is one pixel, many pixels, or none."""
    cases, k = [], 0
    for sw, sh, ov in GEOMETRIES:
        for name, mask in masks_of(sw, sh, ov).items():
            pad = (0, 12, 0)[k % 3]
            cases.append((mask, (mask.shape[1] * 4 + pad) * (-1 if k % 3 == 2 else 1), 4 * sw, 4 * sh))
            k += 1
    rng = np.random.default_rng(5)
    for mw, mh, B, Bh in [(1, 1, 4, 4), (3, 2, 4, 8), (9, 9, 4, 4), (16, 16, 8, 8), (400, 280, 400, 280), (37, 41, 1536, 960)]:
        m = np.full((mh, mw, 4), 255, np.uint8)
        m[rng.integers(0, mh), rng.integers(0, mw), rng.integers(0, 3)] = 254          # one texel a shade off white
        cases.append((m, mw * 4, B, Bh))
        cases.append((m, -(mw * 4 + 4), B, Bh))
    return cases


def memory_of(mask, stride):
    """The rows of `mask` in memory order at |stride| bytes per row (padding 0xEE), and the offset of texel (0, 0)."""
    mh, mw = mask.shape[:2]
    pitch = abs(stride)
    mem = np.full((mh, pitch), 0xEE, np.uint8)
    rows = mask.reshape(mh, mw * 4)
    mem[:, :mw * 4] = rows if stride > 0 else rows[::-1]
    return mem.reshape(-1), (0 if stride > 0 else (mh - 1) * pitch)


def test_mask_box_header_agrees_with_the_restatement(tmp_path):
    exe, data = str(tmp_path / "mask_box"), str(tmp_path / "cases.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "joshupscale_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "mask_box.cpp"), "-o", exe])
    cases = box_cases()
    with open(data, "wb") as f:
        for mask, stride, B, Bh in cases:
            f.write(struct.pack("<5i", mask.shape[1], mask.shape[0], stride, B, Bh))
            f.write(memory_of(mask, stride)[0].tobytes())
    out = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert not out.stderr.strip(), out.stderr
    lines = out.stdout.strip().splitlines()
    boxes = [tuple(int(v) for v in l.split()) for l in lines if not l.startswith("problem")]
    assert len(boxes) == len(cases)
    for got, (mask, stride, B, Bh) in zip(boxes, cases):
        assert got == TM.box(mask, B, Bh), (mask.shape, stride, B, Bh)
    assert sum(b == (0, 0, 0, 0) for b in boxes) >= len(GEOMETRIES) and len(set(boxes)) > 12
    problems = dict(l[len("problem "):].split(": ", 1) if ": " in l else (l[len("problem "):].rstrip(":"), "") for l in lines
                    if l.startswith("problem"))
    size = "the mask must be 1 .. 16384 pixels on each axis"
    assert problems["1 1 4 4"] == "" and problems["16384 16384 1536 960"] == "" and problems["16384 5 131071 280"] == ""
    assert problems["0 5 400 280"] == size and problems["7 16385 400 280"] == size
    assert problems["16384 5 131072 280"] == ("a 16384x5 mask over the blended frame 131072x280: 2 x blended extent x mask extent "
                                              "must stay below 2^32")
    assert problems["7 16384 400 131072"].endswith("must stay below 2^32") and problems["7 5 4294967296 280"].endswith("below 2^32")


def c_box(lib, mask, stride, B, Bh):
    mem, first = memory_of(mask, stride)
    out = (C.c_int * 4)(-1, -1, -1, -1)
    rc = lib.ju_debug_mask_box(mem.ctypes.data + first, stride, mask.shape[1], mask.shape[0], B, Bh, out)
    return rc, tuple(out)


def test_the_no_device_hook_gives_the_same_boxes(hip_library):
    for mask, stride, B, Bh in box_cases():
        assert c_box(hip_library, mask, stride, B, Bh) == (0, TM.box(mask, B, Bh)), (mask.shape, stride, B, Bh)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_the_refusals_messages(hip_library):
    """All of these come before any device call, so they are the same words without a GPU."""
    lib = hip_library
    m = np.full((5, 7, 4), 255, np.uint8)
    out = (C.c_int * 4)()

    def refused(rc, word):
        text = lib.ju_last_error().decode()
        assert rc == JU_ERR_INVALID_ARGUMENT and word in text, (rc, word, text)

    refused(lib.ju_debug_mask_box(None, 28, 7, 5, 400, 280, out), "ju_debug_mask_box: null argument")
    refused(lib.ju_debug_mask_box(m.ctypes.data, 28, 7, 5, 400, 280, None), "null argument")
    refused(lib.ju_debug_mask_box(m.ctypes.data, 28, 0, 5, 400, 280, out), "the mask must be 1 .. 16384 pixels on each axis")
    refused(lib.ju_debug_mask_box(m.ctypes.data, 28, 7, 16385, 400, 280, out), "1 .. 16384")
    refused(lib.ju_debug_mask_box(m.ctypes.data, 24, 7, 5, 400, 280, out), "|stride| smaller than a row")
    refused(lib.ju_debug_mask_box(m.ctypes.data, -27, 7, 5, 400, 280, out), "|stride| smaller than a row")
    refused(lib.ju_debug_mask_box(m.ctypes.data, 28, 7, 5, 0, 280, out), "a frame size outside")
    refused(lib.ju_debug_mask_box(m.ctypes.data, 4 * 16384, 16384, 5, 131072, 280, out), "must stay below 2^32")
    assert lib.ju_tiled_set_source_mask(None, None) == JU_ERR_INVALID_ARGUMENT
    # the kernels' hooks, on addresses that are never touched: every refusal precedes the first device call
    fake = 0x10000
    tiles = (C.c_void_p * 9)(*[fake + 0x100000 * (k + 1) for k in range(9)])

    def plain(dst=fake, stride=1600, sw=100, sh=70, ov=4, t=tiles, n=9, src=fake, sstride=400, mask=fake, mstride=28, mw=7, mh=5):
        return lib.ju_debug_tile_stitch_mask(dst, stride, sw, sh, W, H, ov, t, n, src, sstride, mask, mstride, mw, mh)

    def scaled(dst=fake, stride=1200, ow=300, oh=210, filt=0, sw=100, sh=70, ov=4, t=tiles, n=9, src=fake, sstride=400, mask=fake,
               mstride=28, mw=7, mh=5):
        return lib.ju_debug_tile_stitch_mask_scale(dst, stride, ow, oh, filt, sw, sh, W, H, ov, t, n, src, sstride, mask, mstride, mw, mh)

    odd = (C.c_void_p * 9)(*[fake + 0x100000 * (k + 1) + (8 if k == 5 else 0) for k in range(9)])
    for call in (plain, scaled):
        for kw, word in [(dict(dst=None), "null"), (dict(t=None), "null"), (dict(t=odd), "tile 5"), (dict(n=4), "9 tiles"),
                         (dict(ov=8), "overlap"), (dict(sw=47), "source size"), (dict(src=None), "null source"),
                         (dict(src=fake + 2), "multiples of 4"), (dict(sstride=402), "multiples of 4"),
                         (dict(mask=fake + 1), "multiples of 4"), (dict(mstride=30), "multiples of 4"),
                         (dict(sstride=396), "smaller than a row"), (dict(mstride=-24), "smaller than a row"),
                         (dict(mw=0), "1 .. 16384"), (dict(mh=16385), "1 .. 16384")]:
            refused(call(**kw), word)
            assert call.__name__ == "plain" or "ju_debug_tile_stitch_mask_scale: " in lib.ju_last_error().decode()
    refused(plain(dst=fake + 2), "multiples of 4")
    refused(plain(stride=1596), "smaller than a row")
    refused(scaled(stride=1196), "smaller than a row")
    refused(scaled(ow=24), "the blended frame 400x280, four times the tiled source size")
    refused(scaled(filt=1), "unknown filter 1")
    # 2 B MW >= 2^32 needs a frame the small model cannot reach: a model of 8192 x 8192 and a source of eight tiles
    big = (C.c_void_p * 8)(*[fake + 0x100000 * (k + 1) for k in range(8)])
    rc = lib.ju_debug_tile_stitch_mask(fake, 4 * 262144, 65536, 8192, 8192, 8192, 0, big, 8, fake, 4 * 65536, fake, 4 * 16384, 16384, 5)
    refused(rc, "a 16384x5 mask over the blended frame 262144x32768: 2 x blended extent x mask extent must stay below 2^32")


def test_the_surface_is_declared():
    def declared(header):
        text = open(os.path.join(ROOT, "include", header)).read()
        return set(re.findall(r"JU_API\s+[\w\s\*]+?\b(ju_\w+)\s*\(", text))
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    assert "ju_tiled_set_source_mask" in declared("joshupscale_amd.h")
    assert "ju_tiled_set_source_mask" in R.PRODUCT_SYMBOLS and "ju_tiled_set_source_mask" not in R.HOOK_SYMBOLS
    at = text.index("JU_API int ju_tiled_set_source_mask")
    comment = text[text.rindex("/*", 0, at):at]
    assert "no reference counterpart in the core; the OBS filter's" in comment and "blend.effect" in comment
    assert "obs_plugin/src/filter.cc:215-217, 393-402" in comment
    for key in ('"source_mask"', '"source_mask_frames"', '"mask_box_x0"', '"mask_box_y0"', '"mask_box_x1"', '"mask_box_y1"'):
        assert key in comment, key
    for name in ("ju_debug_tile_stitch_mask", "ju_debug_tile_stitch_mask_scale", "ju_debug_mask_box"):
        assert name in declared("joshupscale_amd_test.h") and name not in declared("joshupscale_amd.h")
        assert name in R.HOOK_SYMBOLS and name not in R.PRODUCT_SYMBOLS
    assert callable(R.TiledRuntime.set_source_mask)
    assert "ju_set_source_size and the mask" not in text              # (the "Not provided for a tiled object" line)
    doc = open(os.path.join(ROOT, "docs", "tiled.md")).read()
    assert "## A mask" in doc and "ju_tiled_set_source_mask" in doc
    scope = doc[doc.index("## Out of scope"):]
    assert "ju_set_source_size" in scope and "- the mask" not in scope.lower()
    kernels = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "tile_kernels.hip")).read()
    assert "tile_stitch_mask_kernel" in kernels and "tile_stitch_mask_scale_kernel" in kernels and "StitchMaskSource8" in kernels
    assert "asm" not in kernels[kernels.index("---- the source mask"):kernels.index("---- the blend of the tiles' f16 states")]
    box = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "mask_box.h")).read()
    assert "hip" not in box.replace("HIP.", "").replace("no HIP", "").lower()
