"""A tiled frame's deep outputs without a GPU (docs/tiled.md "Deep outputs"): the properties of the numpy definition
(tests/tiled_deep_reference.py) over the geometries of tests/test_gpu_tiled.py -- one tile, 2 x 2 tiles that overlap almost
entirely, 3 x 3 tiles, ramps that start at both phases mod 4 -- and the declared surface."""

import os
import re
from fractions import Fraction

import numpy as np
import pytest

import tiled_deep_reference as D
import tiled_reference as T
from helpers import ROOT
from joshupscale_amd import runtime as R

W, H = 48, 30
SOURCES = [(48, 30), (49, 31), (80, 30), (48, 50), (100, 70)]
OVERLAPS = [0, 4, 7]
GEOMETRIES = [(sw, sh, ov) for sw, sh in SOURCES for ov in OVERLAPS]


def count(sw, sh, ov):
    return len(T.origins(sw, W, ov)) * len(T.origins(sh, H, ov))


def random_p(sw, sh, ov, seed=0):
    rng = np.random.default_rng(seed + sw * 1000 + sh * 10 + ov)
    return [rng.integers(0, 65536, (4 * H, 4 * W, 4), dtype=np.uint16) for _ in range(count(sw, sh, ov))]   # (X random)


def test_the_geometries_are_the_gpu_tests():
    assert len(GEOMETRIES) == 15 and all(T.problem(sw, sh, W, H, ov) == "" for sw, sh, ov in GEOMETRIES)
    assert sorted({count(*g) for g in GEOMETRIES}) == [1, 2, 4, 9]
    # ramps (and hard cuts) begin at 0 and at 2 (mod 4): a group of four pixels straddles a seam's edge
    phases = set()
    for sw, sh, ov in GEOMETRIES:
        for S, t in ((sw, W), (sh, H)):
            _, first, q = T.layout(S, t, ov)
            edges = np.flatnonzero(np.diff(first) != 0) + 1 if ov == 0 else np.flatnonzero((q[1:] != 0) & (q[:-1] == 0)) + 1
            phases |= {int(e) % 4 for e in edges}
    assert phases == {0, 2}


@pytest.mark.parametrize("ov", OVERLAPS)
def test_one_tile_is_the_identity(ov):
    p = random_p(48, 30, ov)
    out = D.stitch16(p, 48, 30, W, H, ov)
    assert out.dtype == np.uint16 and out.shape == (4 * H, 4 * W, 4)
    assert np.array_equal(out[..., :3], p[0][..., :3]) and (out[..., 3] == 0).all()


@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_constants_x_and_the_sum_bound(sw, sh, ov):
    n = count(sw, sh, ov)
    full = [np.full((4 * H, 4 * W, 4), 65535, np.uint16)] * n
    out = D.stitch16(full, sw, sh, W, H, ov)
    assert (out[..., :3] == 65535).all() and (out[..., 3] == 0).all()           # 65535 stays 65535; X is 0
    assert D.stitch16_sum_max(full, sw, sh, W, H, ov) == 65535 * 65536 + 32768 < 1 << 32
    zero = D.stitch16([np.zeros((4 * H, 4 * W, 4), np.uint16)] * n, sw, sh, W, H, ov)
    assert not zero.any()
    p = random_p(sw, sh, ov)
    out = D.stitch16(p, sw, sh, W, H, ov)
    assert (out[..., 3] == 0).all() and D.stitch16_sum_max(p, sw, sh, W, H, ov) < 1 << 32
    # a pixel under one tile is that tile's P unchanged; equal tiles blend to themselves
    wt = T.weights(sw, sh, W, H, ov)
    xs, ys = T.origins(sw, W, ov), T.origins(sh, H, ov)
    for k in range(n):
        Y, X = 4 * ys[k // len(xs)], 4 * xs[k % len(xs)]
        alone = wt[k][Y:Y + 4 * H, X:X + 4 * W] == 65536
        assert alone.any()
        assert np.array_equal(out[Y:Y + 4 * H, X:X + 4 * W, :3][alone], p[k][..., :3][alone]), k
    if n > 1:                                                                   # any frame cut into its tiles ...
        frame = np.random.default_rng(3).integers(0, 65536, (4 * sh, 4 * sw, 3), dtype=np.uint16)
        cut = [frame[4 * y:4 * y + 4 * H, 4 * x:4 * x + 4 * W] for y in ys for x in xs]
        assert np.array_equal(D.stitch16(cut, sw, sh, W, H, ov)[..., :3], frame)   # ... blends to itself


@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_the_16_bit_blend_of_an_8_bit_frame_lies_within_one_of_the_8_bit_blend(sw, sh, ov):
    """With x = sum w v / 65536 the two are floor(x + x / 256 + 1 / 512) and floor(x + 1 / 2): at most 1 apart (the
    argument of docs/output_stage.md); the bound is derived, not measured."""
    rng = np.random.default_rng(sw * 1000 + sh * 10 + ov)
    u8 = [rng.integers(0, 256, (4 * H, 4 * W, 4), dtype=np.uint8) for _ in range(count(sw, sh, ov))]
    deep = D.stitch16([t.astype(np.uint16) * 257 for t in u8], sw, sh, W, H, ov)
    eight = T.stitch(u8, sw, sh, W, H, ov)
    d = np.abs((deep[..., :3] >> 8).astype(int) - eight[..., :3].astype(int))
    assert d.max() <= 1


def test_p_from_state_at_the_clamps():
    one = np.float16(1.0)
    half = np.float16(0.5)
    values = np.array([-half, half, np.float16(0.0), -np.float16(0.0),
                       np.nextafter(half, np.float16(0)), np.nextafter(half, one),            # one ulp inside, outside
                       np.nextafter(-half, np.float16(0)), np.nextafter(-half, -one)], np.float16)
    assert values[4] < half < values[5] and values[7] < -half < values[6]
    state = np.zeros((1, len(values), 4), np.float16)
    state[0, :, 0] = state[0, :, 1] = state[0, :, 2] = values
    state[0, :, 3] = np.float16(7.0)                                            # (ignored)
    p = D.p_from_state(state)
    assert p.shape == (1, len(values), 3)
    want = [0, 65535, 32768, 32768, 65520, 65535, 16, 0]
    exact = [min(max((Fraction(float(v)) + Fraction(1, 2)) * 65536 // 1, 0), 65535) for v in values]
    assert want == [int(e) for e in exact]
    for c in range(3):
        assert p[0, :, c].tolist() == want
    assert (Fraction(float(values[5])) + Fraction(1, 2)) * 65536 > 65535 and Fraction(float(values[7])) + Fraction(1, 2) < 0


def test_the_surface_is_declared():
    def declared(header):
        text = open(os.path.join(ROOT, "include", header)).read()
        return set(re.findall(r"JU_API\s+[\w\s\*]+?\b(ju_\w+)\s*\(", text))
    assert "ju_tiled_set_deep_from_state" in declared("joshupscale_amd.h")
    assert "ju_tiled_set_deep_from_state" in R.PRODUCT_SYMBOLS and "ju_tiled_set_deep_from_state" not in R.HOOK_SYMBOLS
    assert "ju_debug_tile_stitch_state" in declared("joshupscale_amd_test.h")
    assert "ju_debug_tile_stitch_state" in R.HOOK_SYMBOLS and "ju_debug_tile_stitch_state" not in declared("joshupscale_amd.h")
    assert callable(R.TiledRuntime.set_deep_from_state)
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    at = text.index("JU_API int ju_tiled_set_deep_from_state")
    assert "no reference counterpart" in text[text.rindex("/*", 0, at):at]
    doc = open(os.path.join(ROOT, "docs", "tiled.md")).read()
    assert "## Deep outputs" in doc
    for key in ('"deep_from_state"', '"hbd_from_state"', '"deep_state_frames"'):
        assert key in doc and key in text, key
