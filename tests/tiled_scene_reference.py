"""The scene detector of a tiled stream (docs/tiled.md "Scene cuts"): tests/scene_reference.py, imported unchanged, is the
definition -- score, decision, start rules, records -- applied to the SOURCE-size BGRX frame of every call.  This module
adds only what is tiled: which tile counts which source pixel (tile_split_scene_kernel sums inside the split's grid, where
tiles overlap), restated from joshupscale_amd/csrc/tile_geometry.h tileOwnedEnds, and the sum taken that way.

Per axis (S source length, t tile length, ov overlap; x_i the origins of tests/tiled_reference.py): tile i owns
[x_i, x_(i+1)), the last tile up to S.  Three tiles of an axis may cover one pixel (t = 48, ov = 7, S = 90: origins 0, 21,
42 -- pixels 42 .. 47), so ownership is by origin interval, not "the first of two"."""

import numpy as np

import scene_reference as S
import tiled_reference as T

OFF, REPORT, RESET = S.OFF, S.REPORT, S.RESET
problem, run, cuts, Detector, known_clip = S.problem, S.run, S.cuts, S.Detector, S.known_clip


def owned(length: int, t: int, ov: int) -> list:
    """``[(begin, end), ...]``: the interval of source coordinates each tile of one axis counts."""
    x = T.origins(length, t, ov)
    return [(x[i], x[i + 1] if i + 1 < len(x) else length) for i in range(len(x))]


def owned_sums(t: int, ov: int):
    """What tests/cxx/tile_ownership.cpp prints per (t, ov): over every t <= S <= 8 t the sum of
    (end_i + 1) (i + 1) (S + 7) and the sum of the tile counts -- vectorised over S."""
    lengths = np.arange(t, T.MAX_RATIO * t + 1, dtype=np.int64)
    n = np.where(lengths == t, 1, -((lengths - ov) // -(t - ov)))
    total, tiles = 0, int(n.sum())
    for i in range(int(n.max())):
        live = i < n
        last = i + 1 == n
        nxt = (i + 1) * (lengths - t) // np.maximum(n - 1, 1)
        end = np.where(last, lengths, nxt)
        total += int(((end + 1) * (i + 1) * (lengths + 7))[live].sum())
    return total, tiles


def owner_map(src_w: int, src_h: int, w: int, h: int, ov: int) -> np.ndarray:
    """``[Hs, Ws]`` int: the tile (row-major over the tile grid) that counts each source pixel; -1 nowhere."""
    ox, oy = owned(src_w, w, ov), owned(src_h, h, ov)
    m = np.full((src_h, src_w), -1, np.int32)
    for j, (y0, y1) in enumerate(oy):
        for i, (x0, x1) in enumerate(ox):
            assert (m[y0:y1, x0:x1] == -1).all()
            m[y0:y1, x0:x1] = j * len(ox) + i
    return m


def owned_sad(cur: np.ndarray, prev: np.ndarray, w: int, h: int, ov: int) -> int:
    """S as the fused kernel takes it: tile by tile over what each owns.  Equals ``scene_reference.sad``."""
    src_h, src_w = cur.shape[:2]
    total = 0
    for y0, y1 in owned(src_h, h, ov):
        for x0, x1 in owned(src_w, w, ov):
            if y1 > y0 and x1 > x0:
                total += S.sad(np.ascontiguousarray(cur[y0:y1, x0:x1]), np.ascontiguousarray(prev[y0:y1, x0:x1]))
    return total


def masked(frame: np.ndarray) -> np.ndarray:
    """The kept frame after a step: the source with X = 0."""
    out = np.ascontiguousarray(frame).copy()
    out[..., 3] = 0
    return out
