"""The definition of a tiled frame's deep outputs in numpy (docs/tiled.md "Deep outputs"): the blend of the tiles' 16-bit
samples with the unchanged weights of tiled_reference, and the planes the existing encode from a 16-bit frame makes of
it.  tile_stitch_state_kernel (csrc/tile_kernels.hip) computes ``stitch16(p_from_state(states))`` word for word.

For tile ``k``, ``P_k`` is the 16-bit samples of its f16 state ``[4 h, 4 w, 4]`` (B, G, R, 0):
``P = clamp(floor((s + 0.5) * 65536), 0, 65535)`` -- ``output_reference.p_from_state``.  Per channel of B, G, R

    out16 = (sum wy wx P + 32768) >> 16

over the tiles the two axes name (``tiled_reference.weights``: wy wx, summing to 65536 per pixel), X = 0.  The sum is at
most 65535 * 65536 + 32768 < 2^32 (asserted): an unsigned 32-bit word holds it.  A pixel under one tile is that tile's P
unchanged, equal tiles blend to themselves, 65535 stays 65535."""

from __future__ import annotations

import numpy as np

import output_reference as O
import tiled_reference as T

SCALE = T.SCALE
SUM_BOUND = 1 << 32


def p_from_state(state) -> np.ndarray:
    """``[H, W, 3]`` int64: the 16-bit samples of B, G, R of an f16 state ``[H, W, 4]`` (the fourth value is ignored)."""
    return O.p_from_state(state)


def _sums(p_tiles, src_w: int, src_h: int, w: int, h: int, ov: int) -> np.ndarray:
    """``[4 Hs, 4 Ws, 3]`` int64: sum wy wx P + 32768 of every output pixel."""
    xs, ys = T.origins(src_w, w, ov), T.origins(src_h, h, ov)
    wt = T.weights(src_w, src_h, w, h, ov)
    assert len(p_tiles) == len(xs) * len(ys)
    acc = np.full((SCALE * src_h, SCALE * src_w, 3), 32768, np.int64)
    k = 0
    for y in ys:
        for x in xs:
            p = np.asarray(p_tiles[k])[..., :3].astype(np.int64)
            assert p.shape == (SCALE * h, SCALE * w, 3)
            assert int(p.min(initial=0)) >= 0 and int(p.max(initial=0)) <= 65535
            Y, X = SCALE * y, SCALE * x
            region = (slice(Y, Y + SCALE * h), slice(X, X + SCALE * w))
            assert not wt[k][:Y].any() and not wt[k][Y + SCALE * h:].any()      # no weight outside the tile
            assert not wt[k][:, :X].any() and not wt[k][:, X + SCALE * w:].any()
            acc[region] += wt[k][region][..., None] * p
            k += 1
    return acc


def stitch16_sum_max(p_tiles, src_w: int, src_h: int, w: int, h: int, ov: int) -> int:
    """The largest sum of ``stitch16``, its rounding constant included: what the 32-bit bound is about."""
    return int(_sums(p_tiles, src_w, src_h, w, h, ov).max())


def stitch16(p_tiles, src_w: int, src_h: int, w: int, h: int, ov: int) -> np.ndarray:
    """The ``[4 Hs, 4 Ws, 4]`` uint16 frame of the tiles' 16-bit samples (``[4 h, 4 w, 3 or 4]`` each, any integer
    dtype, row-major over the tile grid): per channel ``(sum wy wx P + 32768) >> 16``, X = 0."""
    acc = _sums(p_tiles, src_w, src_h, w, h, ov)
    assert int(acc.max()) < SUM_BOUND
    out = np.zeros((SCALE * src_h, SCALE * src_w, 4), np.uint16)
    out[..., :3] = acc >> 16                                                     # (at most 65535: the weights sum to 65536)
    return out


def planes(fmt: int, cs: int, p_tiles, src_w: int, src_h: int, w: int, h: int, ov: int):
    """The planes of the deep format ``fmt`` of a tiled frame: the existing encode from the blended 16-bit frame."""
    return O.encode16(fmt, cs, stitch16(p_tiles, src_w, src_h, w, h, ov))
