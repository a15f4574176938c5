"""Tiled upscaling without a GPU (docs/tiled.md): the properties of the numpy definition (tests/tiled_reference.py),
joshupscale_amd/csrc/tile_geometry.h against it entry for entry -- from a stand-alone host program, tests/cxx/
tile_geometry.cpp, under the address and undefined-behaviour sanitizers -- and the declared surface."""

import os
import re
import subprocess

import numpy as np
import pytest

import tiled_reference as T
from helpers import ROOT
from joshupscale_amd import runtime as R

# (src_w, src_h, w, h, ov): one tile, one pixel more than a tile, the largest ratio, no overlap, the largest overlap,
# odd sizes, three tiles on an axis
GEOMETRIES = [(48, 30, 48, 30, 0), (48, 30, 48, 30, 7), (49, 31, 48, 30, 4), (49, 31, 48, 30, 0), (384, 240, 48, 30, 0),
              (384, 30, 48, 30, 7), (48, 240, 48, 30, 7), (80, 30, 48, 30, 4), (48, 50, 48, 30, 7), (100, 70, 48, 30, 4),
              (100, 70, 48, 30, 0), (100, 70, 48, 30, 7), (500, 280, 480, 270, 16), (960, 540, 480, 270, 16),
              (1280, 720, 480, 270, 67), (96, 64, 48, 30, 4)]


def test_weights_sum_to_one_everywhere():
    for sw, sh, w, h, ov in GEOMETRIES:
        if sw * sh > 200 * 200:
            continue  # (the dense weight tensor of a full-size layout is large; its axes are checked below)
        wt = T.weights(sw, sh, w, h, ov)
        assert (wt.sum(axis=0) == 65536).all(), (sw, sh, w, h, ov)
        assert wt.min() >= 0
    for sw, sh, w, h, ov in GEOMETRIES:  # per axis: the two weights are 256 - q and q, and a tile behind the first exists
        for S, t in ((sw, w), (sh, h)):
            x, first, q = T.layout(S, t, ov)
            assert first.size == 4 * S and 0 <= q.min() and q.max() <= 256
            assert ((first + 1 < len(x)) | (q == 0)).all()
            assert (np.diff(first) >= 0).all() and first[0] == 0 and first[-1] == len(x) - 1


def test_a_single_tile_is_the_identity():
    rng = np.random.default_rng(1)
    tile = rng.integers(0, 256, (120, 192, 4), dtype=np.uint8)
    for ov in (0, 4, 7):
        assert T.origins(48, 48, ov) == [0] and T.origins(30, 30, ov) == [0]
        out = T.stitch([tile], 48, 30, 48, 30, ov)
        assert (out[..., :3] == tile[..., :3]).all() and (out[..., 3] == 0).all()
        frame = rng.integers(0, 256, (30, 48, 4), dtype=np.uint8)
        (only,) = T.split(frame, 48, 30, ov)
        assert (only[..., :3] == frame[..., :3]).all() and (only[..., 3] == 0).all()


def test_equal_constant_tiles_stitch_to_that_constant():
    for sw, sh, w, h, ov in [(100, 70, 48, 30, 4), (49, 31, 48, 30, 7), (80, 30, 48, 30, 0)]:
        n = len(T.origins(sw, w, ov)) * len(T.origins(sh, h, ov))
        for value in (0, 1, 127, 255):
            tiles = [np.full((4 * h, 4 * w, 4), value, np.uint8)] * n
            out = T.stitch(tiles, sw, sh, w, h, ov)
            assert (out[..., :3] == value).all() and (out[..., 3] == 0).all()


def test_a_pixel_under_one_tile_is_that_tiles_byte():
    rng = np.random.default_rng(2)
    sw, sh, w, h, ov = 100, 70, 48, 30, 4
    xs, ys = T.origins(sw, w, ov), T.origins(sh, h, ov)
    tiles = [rng.integers(0, 256, (4 * h, 4 * w, 4), dtype=np.uint8) for _ in range(len(xs) * len(ys))]
    out = T.stitch(tiles, sw, sh, w, h, ov)
    wt = T.weights(sw, sh, w, h, ov)
    for k, tile in enumerate(tiles):
        Y, X = 4 * ys[k // len(xs)], 4 * xs[k % len(xs)]
        alone = wt[k][Y:Y + 4 * h, X:X + 4 * w] == 65536
        assert alone.any()
        assert (out[Y:Y + 4 * h, X:X + 4 * w, :3][alone] == tile[..., :3][alone]).all()


@pytest.mark.parametrize("t", [30, 48, 270, 480])
def test_ramps_are_disjoint_and_inside_their_overlaps(t):
    """Every overlap up to t / 4 and every source length up to 8 t: neighbours overlap by at least ov, every ramp lies
    inside its overlap and consecutive ramps do not intersect -- so no output coordinate needs three tiles."""
    for ov in range(t // 4 + 1):
        S = np.arange(t + 1, 8 * t + 1, dtype=np.int64)
        n = -((S - ov) // -(t - ov))
        assert n.min() >= 2
        R = 4 * ov
        end_prev = np.zeros_like(S)
        for i in range(int(n.max()) - 1):
            live = i + 1 < n
            xi, xj = i * (S - t) // (n - 1), (i + 1) * (S - t) // (n - 1)
            L = xi + t - xj
            r0 = 4 * xj + (4 * L - R) // 2
            assert (L[live] >= ov).all(), (t, ov, i)
            assert (r0[live] >= 4 * xj[live]).all() and (r0[live] + R <= 4 * (xi[live] + t)).all(), (t, ov, i)
            assert (r0[live] >= end_prev[live]).all(), (t, ov, i)
            end_prev = np.where(live, r0 + R, end_prev)
        assert ((n - 1) * (S - t) // (n - 1) == S - t).all()  # the last tile ends exactly at S


def test_limits():
    assert T.problem(100, 70, 48, 30, 4) == ""
    assert "overlap" in T.problem(100, 70, 48, 30, 8) and "overlap" in T.problem(100, 70, 48, 30, -1)
    assert T.problem(100, 70, 48, 30, 7) == ""
    assert "source size" in T.problem(47, 70, 48, 30, 4) and "source size" in T.problem(100, 241, 48, 30, 4)
    assert T.problem(384, 240, 48, 30, 0) == ""                 # 8 x 8 tiles
    assert "tiles" in T.problem(384, 240, 48, 30, 7)            # 10 x 11


def run_program(tmp_path, cases):
    exe = str(tmp_path / "tile_geometry")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "joshupscale_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "tile_geometry.cpp"), "-o", exe])
    args = [str(v) for case in cases for v in case]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert not out.stderr.strip(), out.stderr
    blocks = out.stdout.strip().split("case ")[1:]
    assert len(blocks) == len(cases)
    return [b.splitlines() for b in blocks]


def test_tile_geometry_header_matches_the_reference(tmp_path):
    refused = [(100, 70, 48, 30, 8), (47, 30, 48, 30, 0), (385, 30, 48, 30, 0), (384, 240, 48, 30, 7)]
    cases = GEOMETRIES + refused
    for lines, case in zip(run_program(tmp_path, cases), cases):
        sw, sh, w, h, ov = case
        assert lines[0].split() == [str(v) for v in case]
        if case in refused:
            assert T.problem(*case) and lines[1] == "refused " + T.problem(*case), (case, lines[1])
            continue
        assert T.problem(*case) == "" and len(lines) == 6, (case, lines[1])
        for (S, t), (o_line, t_line), name in (((sw, w), lines[1:3], "x"), ((sh, h), lines[3:5], "y")):
            x, first, q = T.layout(S, t, ov)
            assert o_line.split() == [name, "origins"] + [str(v) for v in x], case
            got = t_line.split()
            assert got[:2] == [name, "table"] and len(got) == 2 + 4 * S, case
            entries = np.array([[int(v) for v in e.split(":")] for e in got[2:]])
            assert (entries[:, 0] == first).all() and (entries[:, 1] == q).all(), case
        # the passes: consecutive, all tiles, at most 8 each, the fewest, and none of one tile beside larger ones
        n = len(T.origins(sw, w, ov)) * len(T.origins(sh, h, ov))
        passes = [tuple(int(v) for v in p.split("+")) for p in lines[5].split()[1:]]
        assert len(passes) == -(n // -8) and passes[0][0] == 0 and sum(c for _, c in passes) == n
        assert all(a + c == b for (a, c), (b, _) in zip(passes, passes[1:]))
        assert all(1 <= c <= 8 for _, c in passes) and max(c for _, c in passes) - min(c for _, c in passes) <= 1


def test_the_surface_is_declared():
    product = ["ju_tiled_create", "ju_tiled_create_from_memory", "ju_tiled_destroy", "ju_tiled_reset", "ju_tiled_process",
               "ju_tiled_process_frame", "ju_tiled_get_info", "ju_tiled_get_tile", "ju_tiled_get_stat"]
    hooks = ["ju_debug_tile_split", "ju_debug_tile_stitch"]

    def declared(header):
        text = open(os.path.join(ROOT, "include", header)).read()
        return set(re.findall(r"JU_API\s+[\w\s\*]+?\b(ju_\w+)\s*\(", text))
    assert set(product) <= declared("joshupscale_amd.h") and set(product) <= set(R.PRODUCT_SYMBOLS)
    assert set(hooks) <= declared("joshupscale_amd_test.h") and set(hooks) <= set(R.HOOK_SYMBOLS)
    assert not set(hooks) & declared("joshupscale_amd.h")
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    block = text[text.index("---- tiled upscaling"):text.index("ju_tiled_create_from_memory")]
    assert "no reference counterpart" in block
    assert R.TiledRuntime.__init__.__defaults__[-2] == 16  # overlap
