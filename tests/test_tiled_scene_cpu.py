"""The scene detector of a tiled stream without a GPU (docs/tiled.md "Scene cuts"): the ownership rule of
tests/tiled_scene_reference.py -- a partition of the source, inside the tiles -- and joshupscale_amd/csrc/tile_geometry.h
tileOwnedEnds against it from a stand-alone host program (tests/cxx/tile_ownership.cpp) under the address and
undefined-behaviour sanitizers; the clips the GPU tests rely on; the declared surface."""

import os
import re
import subprocess

import numpy as np
import pytest

import scene_reference as S
import tiled_reference as T
import tiled_scene_reference as TS
from helpers import M, ROOT
from joshupscale_amd import runtime as R

TILE_LENGTHS = [30, 48, 270, 480]


@pytest.mark.parametrize("t", TILE_LENGTHS)
def test_ownership_partitions_the_source_inside_the_tiles(t):
    """Every overlap up to t / 4 and every source length up to 8 t, vectorised over the lengths: the intervals follow each
    other without a gap from 0 to S, and interval i lies inside tile i."""
    for ov in range(t // 4 + 1):
        lengths = np.arange(t + 1, 8 * t + 1, dtype=np.int64)
        n = -((lengths - ov) // -(t - ov))
        begin = np.zeros_like(lengths)                            # where the next interval has to begin
        for i in range(int(n.max())):
            live = i < n
            x = i * (lengths - t) // (n - 1)
            end = np.where(i + 1 == n, lengths, (i + 1) * (lengths - t) // (n - 1))
            assert (x[live] == begin[live]).all(), (t, ov, i)                       # no gap, no pixel twice
            assert (end[live] >= x[live]).all() and (end[live] <= x[live] + t).all(), (t, ov, i)   # inside tile i
            begin = np.where(live, end, begin)
        assert (begin == lengths).all(), (t, ov)                  # the last interval ends at S
        assert TS.owned(t, t, ov) == [(0, t)]                     # one tile owns everything


def test_ownership_restatement_and_the_three_tile_example():
    assert T.origins(90, 48, 7) == [0, 21, 42] and TS.owned(90, 48, 7) == [(0, 21), (21, 42), (42, 90)]
    covered = [sum(x <= p < x + 48 for x in T.origins(90, 48, 7)) for p in range(90)]
    assert max(covered) == 3 and covered[42:48] == [3] * 6        # three tiles over one pixel: "the first of two" would count it twice
    for sw, sh, ov in [(48, 30, 7), (49, 31, 0), (80, 30, 4), (100, 70, 4), (90, 54, 7)]:
        m = TS.owner_map(sw, sh, 48, 30, ov)
        assert (m >= 0).all()                                      # every pixel has exactly one owner (owner_map asserts "at most")
        xs, ys = T.origins(sw, 48, ov), T.origins(sh, 30, ov)
        for k in range(len(xs) * len(ys)):                         # ... which covers it
            yy, xx = np.nonzero(m == k)
            x0, y0 = xs[k % len(xs)], ys[k // len(xs)]
            assert yy.size and x0 <= xx.min() and xx.max() < x0 + 48 and y0 <= yy.min() and yy.max() < y0 + 30, (sw, sh, ov, k)
        rng = np.random.default_rng(sw + sh + ov)
        a, b = (rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8) for _ in range(2))
        assert TS.owned_sad(a, b, 48, 30, ov) == S.sad(a, b)      # tile by tile over what each owns: the plain sum


def test_tile_geometry_header_agrees_with_the_restatement(tmp_path):
    exe = str(tmp_path / "tile_ownership")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "joshupscale_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "tile_ownership.cpp"), "-o", exe])
    out = subprocess.run([exe] + [str(t) for t in TILE_LENGTHS], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert not out.stderr.strip(), out.stderr
    lines = out.stdout.strip().splitlines()
    sums = [tuple(int(v) for v in l.split()) for l in lines if not l.startswith("example")]
    assert [(t, ov) for t, ov, _, _ in sums] == [(t, ov) for t in TILE_LENGTHS for ov in range(t // 4 + 1)]
    for t, ov, total, tiles in sums:
        assert TS.owned_sums(t, ov) == (total, tiles), (t, ov)
    examples = [l.split() for l in lines if l.startswith("example")]
    assert len(examples) == len(TILE_LENGTHS)
    for e, t in zip(examples, TILE_LENGTHS):
        ov, length = t * 7 // 48, 2 * t - 6
        assert e[1:4] == [str(t), str(ov), str(length)]
        assert [tuple(int(v) for v in p.split(":")) for p in e[4:]] == TS.owned(length, t, ov), e
    assert examples[1][4:] == ["0:21", "21:42", "42:90"]


@pytest.mark.parametrize("size,thr,around", [((70, 100), 18500, [20.00, 17.35, 19.67, 17.45]),
                                             ((54, 90), 19000, [22.91, 18.36, 20.23, 16.34])])
def test_known_clips(size, thr, around):
    """The clips of the GPU tests, asserted before anything relies on them: the cuts at the source size and the scores per
    byte of frames 4, 5, 7 and 8 -- a cut, then the frame behind it, whose score stays under the threshold."""
    h, w = size
    clip = S.known_clip(M.synthetic_frames, h, w)
    assert clip.shape == (13, h, w, 4)
    recs = TS.run(clip, thr)
    assert TS.cuts(recs) == S.KNOWN_CUTS == [4, 7, 10, 12]
    n = 3 * h * w
    assert [round(recs[t]["score"] / n, 2) for t in (4, 5, 7, 8)] == around
    assert all(a * 1000 < thr for a in around[1::2]) and all(a * 1000 >= thr for a in around[0::2])
    assert [r["step"] for r in recs] == list(range(13))


def test_the_surface_is_declared():
    product = ["ju_tiled_set_scene_detect", "ju_tiled_get_scene_detect", "ju_tiled_get_scene_info"]
    hooks = ["ju_debug_tile_split_scene", "ju_debug_scene_clear_tiles"]

    def declared(header):
        text = open(os.path.join(ROOT, "include", header)).read()
        return set(re.findall(r"JU_API\s+[\w\s\*]+?\b(ju_\w+)\s*\(", text))
    assert set(product) <= declared("joshupscale_amd.h") and set(product) <= set(R.PRODUCT_SYMBOLS)
    assert set(hooks) <= declared("joshupscale_amd_test.h") and set(hooks) <= set(R.HOOK_SYMBOLS)
    assert not set(hooks) & declared("joshupscale_amd.h") and not set(hooks) & set(R.PRODUCT_SYMBOLS)
    for name in ("set_scene_detect", "get_scene_detect", "scene_info"):
        assert callable(getattr(R.TiledRuntime, name))
    assert R.TiledRuntime.set_scene_detect.__defaults__ == (10000,) and R.TiledRuntime.scene_info.__defaults__ == (64,)
    kernels = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "tile_kernels.hip")).read()
    scene = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "scene_kernels.hip")).read()
    assert "tile_split_scene_kernel" in kernels and "scene_clear_tiles_kernel" in scene
    # one copy of the decision arithmetic, shared by both kernels
    assert '#include "scene_decision.h"' in kernels and '#include "scene_decision.h"' in scene
    assert kernels.count("sceneDecide(") == 1 and "1000ull * D" not in kernels
