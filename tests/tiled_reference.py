"""The definition of tiled upscaling in numpy (docs/tiled.md): the layout of the tiles along one axis, the cut of a
source into tile inputs and the blend of the tile outputs into one frame.  joshupscale_amd/csrc/tile_geometry.h restates
``layout``; tile_split_kernel and tile_stitch_kernel compute ``split`` and ``stitch`` byte for byte.

Per axis: ``S`` the source length, ``t`` the tile (model) length, ``ov`` the overlap in source pixels; the scale is 4.
"""

from __future__ import annotations

import numpy as np

SCALE = 4
MAX_TILES = 64
MAX_RATIO = 8


def problem(src_w: int, src_h: int, w: int, h: int, ov: int) -> str:
    """``""`` when a ``src_w x src_h`` source may be tiled by a ``w x h`` model at overlap ``ov``, else what is wrong."""
    if not 0 <= ov <= min(w, h) // 4:
        return f"overlap {ov} outside 0 .. {min(w, h) // 4}"
    if not (w <= src_w <= MAX_RATIO * w and h <= src_h <= MAX_RATIO * h):
        return f"source size {src_w}x{src_h} outside {w}x{h} .. {MAX_RATIO * w}x{MAX_RATIO * h}"
    nx, ny = len(origins(src_w, w, ov)), len(origins(src_h, h, ov))
    if nx * ny > MAX_TILES:
        return f"{nx}x{ny} tiles are more than {MAX_TILES}"
    return ""


def origins(S: int, t: int, ov: int) -> list:
    """Where the tiles of one axis begin, in source pixels."""
    if S == t:
        return [0]
    n = -((S - ov) // -(t - ov))
    return [i * (S - t) // (n - 1) for i in range(n)]


def layout(S: int, t: int, ov: int):
    """``(origins, first, weight)``: per output coordinate X of the 4 S the first tile that covers it and the weight
    0 .. 256 of the tile behind that one (0: the first tile alone)."""
    x = origins(S, t, ov)
    n = len(x)
    first = np.zeros(SCALE * S, np.int32)
    weight = np.zeros(SCALE * S, np.int32)
    R = SCALE * ov
    begin = 0  # the first coordinate tile i has alone (or shares with tile i + 1 only)
    for i in range(n - 1):
        L = x[i] + t - x[i + 1]
        r0 = SCALE * x[i + 1] + (SCALE * L - R) // 2
        first[begin:r0] = i
        for d in range(R):
            first[r0 + d] = i
            weight[r0 + d] = ((2 * d + 1) * 256 + R) // (2 * R)
        begin = r0 + R
    first[begin:] = n - 1
    return x, first, weight


def split(frame: np.ndarray, w: int, h: int, ov: int) -> list:
    """The tile inputs of a ``[Hs, Ws, 4]`` BGRX source, row-major over the tile grid, X = 0."""
    xs, ys = origins(frame.shape[1], w, ov), origins(frame.shape[0], h, ov)
    tiles = []
    for y in ys:
        for x in xs:
            tile = np.ascontiguousarray(frame[y:y + h, x:x + w]).copy()
            tile[..., 3] = 0
            tiles.append(tile)
    return tiles


def weights(src_w: int, src_h: int, w: int, h: int, ov: int) -> np.ndarray:
    """``[tiles, 4 Hs, 4 Ws]`` int64: the weight wy wx of every tile at every output pixel (they sum to 65536)."""
    xs, fx, qx = layout(src_w, w, ov)
    ys, fy, qy = layout(src_h, h, ov)
    nx, ny = len(xs), len(ys)

    def axis(n, first, q):
        a = np.zeros((n, first.size), np.int64)
        idx = np.arange(first.size)
        a[first, idx] += 256 - q
        second = np.minimum(first + 1, n - 1)
        a[second, idx] += np.where(first + 1 < n, q, 0)
        assert not np.any((first + 1 >= n) & (q != 0))
        return a
    ax, ay = axis(nx, fx, qx), axis(ny, fy, qy)
    return (ay[:, None, :, None] * ax[None, :, None, :]).reshape(ny * nx, fy.size, fx.size)


def stitch(tiles, src_w: int, src_h: int, w: int, h: int, ov: int) -> np.ndarray:
    """The ``[4 Hs, 4 Ws, 4]`` frame of the tile outputs (``[4 h, 4 w, 4]`` each): per byte of B, G, R
    ``(sum wy wx v + 32768) >> 16`` over the tiles the two axes name, X = 0."""
    xs, ys = origins(src_w, w, ov), origins(src_h, h, ov)
    wt = weights(src_w, src_h, w, h, ov)
    acc = np.zeros((SCALE * src_h, SCALE * src_w, 3), np.int64)
    k = 0
    for y in ys:
        for x in xs:
            Y, X = SCALE * y, SCALE * x
            region = (slice(Y, Y + SCALE * h), slice(X, X + SCALE * w))
            assert not wt[k][:Y].any() and not wt[k][Y + SCALE * h:].any()      # no weight outside the tile
            assert not wt[k][:, :X].any() and not wt[k][:, X + SCALE * w:].any()
            acc[region] += wt[k][region][..., None] * tiles[k][..., :3].astype(np.int64)
            k += 1
    out = np.zeros((SCALE * src_h, SCALE * src_w, 4), np.uint8)
    out[..., :3] = (acc + 32768) >> 16
    return out
