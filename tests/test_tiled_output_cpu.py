"""A tiled frame under an output size without a GPU (docs/tiled.md "An output size"): the properties of the numpy
definition (tests/tiled_output_reference.py) over the geometries, output sizes and filters the GPU tests use -- the
identity, one tile, constants, the definition's own sum bounds -- the limits' Python twin against the C++ message, and the
declared surface."""

import os
import re

import numpy as np
import pytest

import scale_filter_reference as F
import tiled_deep_reference as D
import tiled_output_reference as TO
import tiled_reference as T
from helpers import ROOT
from joshupscale_amd import runtime as R

W, H = 48, 30                                  # helpers.small_config()
# (Ws, Hs, ov): nine tiles with four-tile corners; four tiles, almost all seam; a hard cut; two tiles; one tile; and four
# tiles whose ramps begin at 2 (mod 4) on both axes, so that a lane's four columns straddle a ramp's edge (the ramps of
# the others begin at 0 mod 4 in x)
GEOMETRIES = [(100, 70, 4), (49, 31, 7), (80, 30, 0), (48, 50, 4), (48, 30, 7), (49, 31, 4)]


def sizes(sw, sh, filt):
    """The output sizes of one geometry and filter as {name: (OW, OH)}, B x Bh the blended size: itself, 3/4, twice, an
    odd pair, the strongest reduction the filter allows (32-tap rows) and an anisotropic one."""
    B, Bh = 4 * sw, 4 * sh
    down = F.down_max(filt)
    return {"same": (B, Bh), "3/4": (3 * B // 4, 3 * Bh // 4), "twice": (2 * B, 2 * Bh),
            "odd": (3 * B // 4 - 1, 3 * Bh // 4 + 1), "least": (-(-B // down), -(-Bh // down)), "aniso": (2 * B, Bh + 3)}


def count(sw, sh, ov):
    return len(T.origins(sw, W, ov)) * len(T.origins(sh, H, ov))


_TILES = {}


def tiles_of(sw, sh, ov):
    """Random tile outputs of one geometry with 0 and 255 present in every tile (X random), computed once."""
    if (sw, sh, ov) not in _TILES:
        rng = np.random.default_rng(7 + sw * 1000 + sh * 10 + ov)
        tiles = []
        for _ in range(count(sw, sh, ov)):
            t = rng.integers(0, 256, (4 * H, 4 * W, 4), dtype=np.uint8)
            t[rng.integers(0, 4 * H, 200), rng.integers(0, 4 * W, 200), :3] = np.repeat([[0], [255]], 100, 0)
            # flat runs of the extremes next to each other: what a cubic filter overshoots on, both clamps
            t[8:16, 16:48, :3], t[8:16, 48:80, :3] = 0, 255
            t.setflags(write=False)
            tiles.append(t)
        _TILES[(sw, sh, ov)] = tiles
    return _TILES[(sw, sh, ov)]


def p_tiles_of(sw, sh, ov):
    """16-bit samples with both ends of the range: the 8-bit tiles' bytes spread over 16 bits, low bits random."""
    rng = np.random.default_rng(9 + sw * 1000 + sh * 10 + ov)
    out = []
    for t in tiles_of(sw, sh, ov):
        low = rng.integers(0, 256, t.shape, dtype=np.uint16)
        p = t.astype(np.uint16) * 256 + np.where((t == 0) | (t == 255), t.astype(np.uint16), low)
        out.append(p)
    return out


def test_the_cases_reach_every_branch():
    assert sorted(count(*g) for g in GEOMETRIES) == [1, 2, 2, 4, 4, 9]
    assert all(T.problem(sw, sh, W, H, ov) == "" for sw, sh, ov in GEOMETRIES)
    for (sw, sh, ov) in GEOMETRIES:
        for filt in F.FILTERS:
            for name, (ow, oh) in sizes(sw, sh, filt).items():
                assert R.tiled_output_size_problem(ow, oh, sw, sh, filt) == "", (sw, sh, filt, name)
    # the widest rows these sizes reach: 32 taps, with every filter (33, the most a table holds, needs a longer axis: the
    # scaler's own tests have it); partial 32 x 8 tiles on both axes; a column quad that straddles a ramp's edge
    widest = {filt: max(int(F.axis_table(4 * g[k], sizes(*g[:2], filt)["least"][k], filt)[1].max()) for g in GEOMETRIES for k in (0, 1))
              for filt in F.FILTERS}
    assert widest == {F.TRIANGLE: 32, F.CATMULL_ROM: 32, F.MITCHELL: 32}
    assert any(ow % 32 and oh % 8 for g in GEOMETRIES for (ow, oh) in sizes(*g[:2], 0).values())
    phases = set()
    for sw, sh, ov in GEOMETRIES:
        _, first, q = T.layout(sw, W, ov)
        edges = np.flatnonzero(np.diff(first) != 0) + 1 if ov == 0 else np.flatnonzero((q[1:] != 0) & (q[:-1] == 0)) + 1
        phases |= {int(e) % 4 for e in edges}
    assert phases == {0, 2}


@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_the_blended_size_is_the_identity_for_the_triangle_and_catmull_rom(sw, sh, ov):
    tiles, p = tiles_of(sw, sh, ov), p_tiles_of(sw, sh, ov)
    B, Bh = 4 * sw, 4 * sh
    want8, want16 = T.stitch(tiles, sw, sh, W, H, ov), D.stitch16(p, sw, sh, W, H, ov)
    for filt in (F.TRIANGLE, F.CATMULL_ROM):
        assert np.array_equal(TO.frame8(tiles, sw, sh, W, H, ov, Bh, B, filt), want8)
        assert np.array_equal(TO.frame16(p, sw, sh, W, H, ov, Bh, B, filt), want16)
    assert not np.array_equal(TO.frame8(tiles, sw, sh, W, H, ov, Bh, B, F.MITCHELL), want8)      # Mitchell filters the frame
    assert not np.array_equal(TO.frame16(p, sw, sh, W, H, ov, Bh, B, F.MITCHELL), want16)


@pytest.mark.parametrize("filt", F.FILTERS, ids=lambda f: F.NAMES[f])
def test_one_tile_is_the_plain_scaler(filt):
    sw, sh, ov = 48, 30, 7
    tiles, p = tiles_of(sw, sh, ov), p_tiles_of(sw, sh, ov)
    for name, (ow, oh) in sizes(sw, sh, filt).items():
        got8 = TO.frame8(tiles, sw, sh, W, H, ov, oh, ow, filt)
        masked = tiles[0].copy()
        masked[..., 3] = 0
        assert np.array_equal(got8, F.scale8(masked, oh, ow, filt)), name
        assert np.array_equal(TO.frame16(p, sw, sh, W, H, ov, oh, ow, filt), F.scale16(p[0], oh, ow, filt)), name
        assert got8.shape == (oh, ow, 4) and got8.dtype == np.uint8 and not got8[..., 3].any()


@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_constants_the_sum_bounds_and_x(sw, sh, ov):
    """Every shape of the list goes through the definition: its own assertions (|vertical sum| < 2^21 / 2^29, |whole sum| <
    2^34 / 2^42, the blend below 2^32) hold at each; equal constant tiles stay that constant; X is 0."""
    n = count(sw, sh, ov)
    tiles, p = tiles_of(sw, sh, ov), p_tiles_of(sw, sh, ov)
    assert min(int(t[..., :3].min()) for t in tiles) == 0 and max(int(t[..., :3].max()) for t in tiles) == 255
    assert min(int(q[..., :3].min()) for q in p) == 0 and max(int(q[..., :3].max()) for q in p) == 65535
    for filt in F.FILTERS:
        for name, (ow, oh) in sizes(sw, sh, filt).items():
            out8 = TO.frame8(tiles, sw, sh, W, H, ov, oh, ow, filt)
            out16 = TO.frame16(p, sw, sh, W, H, ov, oh, ow, filt)
            assert out8.shape == (oh, ow, 4) and out16.shape == (oh, ow, 4) and out16.dtype == np.uint16
            assert not out8[..., 3].any() and not out16[..., 3].any()
    for filt in F.FILTERS:
        ow, oh = sizes(sw, sh, filt)["odd"]
        for c in (0, 1, 200, 255):
            out = TO.frame8([np.full((4 * H, 4 * W, 4), c, np.uint8)] * n, sw, sh, W, H, ov, oh, ow, filt)
            assert (out[..., :3] == c).all()
        for c in (0, 257, 65535):
            out = TO.frame16([np.full((4 * H, 4 * W, 3), c, np.uint16)] * n, sw, sh, W, H, ov, oh, ow, filt)
            assert (out[..., :3] == c).all()


def test_planes_take_the_route_the_definition_names():
    sw, sh, ov = 49, 31, 7
    tiles, p = tiles_of(sw, sh, ov), p_tiles_of(sw, sh, ov)
    ow, oh = 146, 94
    out8 = TO.frame8(tiles, sw, sh, W, H, ov, oh, ow, F.TRIANGLE)
    assert np.array_equal(TO.planes(R.FMT_BGRX, 0, tiles, p, sw, sh, W, H, ov, oh, ow, F.TRIANGLE, False)[0], out8)
    shallow = TO.planes(R.FMT_BGRX64, 0, tiles, p, sw, sh, W, H, ov, oh, ow, F.TRIANGLE, False)[0]
    assert np.array_equal(shallow[..., :3], out8[..., :3].astype(np.uint16) * 257)            # a deep format from 8 bits: 257 u8
    deep = TO.planes(R.FMT_BGRX64, 0, tiles, p, sw, sh, W, H, ov, oh, ow, F.TRIANGLE, True)[0]
    assert np.array_equal(deep[..., :3], TO.frame16(p, sw, sh, W, H, ov, oh, ow, F.TRIANGLE)[..., :3])


def c_limit(lib, filt, size, blended):
    rc = lib.ju_debug_scale(3, filt, None, 0, size[0], size[1], None, 0, blended[0], blended[1], None, None, None)
    return rc, lib.ju_last_error().decode() if rc else ""


def test_the_limits_twin_is_the_c_layers_message_for_the_blended_frame(hip_library):
    """ju_tiled_set_output_size's limits are outputSizeProblem's with the blended frame in the model output's place; a
    limit's message then names that frame as four times the tiled source size."""
    sw, sh = 100, 70
    blended = (400, 280)
    tail = " (of a tiled object: the blended frame 400x280, four times the tiled source size)"
    for filt, down in ((F.TRIANGLE, 16), (F.CATMULL_ROM, 8), (F.MITCHELL, 8)):
        least = (-(-400 // down), -(-280 // down))
        for size in [(400, 280), least, (16 * 400, 16 * 280), (300, 210), (799, 283)]:
            assert R.tiled_output_size_problem(*size, sw, sh, filt) == "", (filt, size)
            assert c_limit(hip_library, filt, size, blended) == (0, "")
        for size in [(least[0] - 1, 280), (400, least[1] - 1), (16 * 400 + 1, 280), (1, 280), (400, 16385), (0, 280)]:
            text = R.tiled_output_size_problem(*size, sw, sh, filt)
            assert text.startswith(f"output size {size[0]}x{size[1]}: ") and text.endswith(tail), text
            assert "400x280" in text and "four times the tiled source size" in text
            assert c_limit(hip_library, filt, size, blended) == (1, "std::invalid_argument: ju_set_output_size: " + text[:-len(tail)])
    for filt in (1, 4, -1):
        text = R.tiled_output_size_problem(300, 210, sw, sh, filt)
        assert text == R.scale_filter_problem(filt) and "JU_SCALE_MITCHELL = 3" in text
        assert c_limit(hip_library, filt, (300, 210), blended) == (1, "std::invalid_argument: ju_set_output_size: " + text)


def test_the_surface_is_declared():
    def declared(header):
        text = open(os.path.join(ROOT, "include", header)).read()
        return set(re.findall(r"JU_API\s+[\w\s\*]+?\b(ju_\w+)\s*\(", text))
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    for name in ("ju_tiled_set_output_size", "ju_tiled_get_output_size"):
        assert name in declared("joshupscale_amd.h")
        assert name in R.PRODUCT_SYMBOLS and name not in R.HOOK_SYMBOLS
    at = text.index("JU_API int ju_tiled_set_output_size")
    assert "no reference counterpart" in text[text.rindex("/*", 0, at):at]
    for name in ("ju_debug_tile_stitch_scale", "ju_debug_tile_stitch_scale_state"):
        assert name in declared("joshupscale_amd_test.h") and name not in declared("joshupscale_amd.h")
        assert name in R.HOOK_SYMBOLS and name not in R.PRODUCT_SYMBOLS
    for method in ("set_output_size", "get_output_size", "frame_output_size"):
        assert callable(getattr(R.TiledRuntime, method))
    assert "ju_set_output_size / the mask" not in text                        # (the "Not provided for a tiled object" line)
    doc = open(os.path.join(ROOT, "docs", "tiled.md")).read()
    assert "## An output size" in doc
    for key in ('"output_scaled"', '"output_filter"', '"output_scaled_frames"'):
        assert key in doc and key in text[text.index("ju_tiled_set_output_size"):], key
