"""The definition of a tiled frame under a source mask in numpy (docs/tiled.md "A mask"): the blended frame of
tiled_reference, rounded to bytes, THEN source_reference.blend with the call's source frame and the mask, THEN -- under an
output size -- scale_filter_reference.scale8, and output_reference's 8-bit encode for every other format.  Nothing of its
own, no tolerance.  tile_stitch_mask_kernel and tile_stitch_mask_scale_kernel (csrc/tile_kernels.hip) compute ``masked`` /
``frame8`` byte for byte; csrc/mask_box.h restates ``box``."""

from __future__ import annotations

import numpy as np

import output_reference as O
import scale_filter_reference as F
import source_reference as S
import tiled_output_reference as TO
import tiled_reference as T


def masked_of_blended(blended: np.ndarray, source: np.ndarray, mask) -> np.ndarray:
    """The mask over a blended ``[4 Hs, 4 Ws, 4]`` frame: ``source`` is the ``[Hs, Ws, 4]`` frame of the call, ``mask`` a
    BGRX image of any size, or None for no mask.  The source texel keeps the general formula of ``S.texel``."""
    assert blended.shape[0] == T.SCALE * source.shape[0] and blended.shape[1] == T.SCALE * source.shape[1]
    return blended if mask is None else S.blend(blended, source, mask)


def masked(tiles, source: np.ndarray, mask, w: int, h: int, ov: int) -> np.ndarray:
    """``[4 Hs, 4 Ws, 4]`` uint8 BGRX, X = 0: ``blend(stitch(tile outputs), c_t, mask)``."""
    src_h, src_w = source.shape[:2]
    return masked_of_blended(T.stitch(tiles, src_w, src_h, w, h, ov), source, mask)


def frame8(tiles, source: np.ndarray, mask, w: int, h: int, ov: int, oh: int, ow: int, filter: int) -> np.ndarray:
    """Under an output size: the mask first, at the blended size, and the scale behind it."""
    return F.scale8(masked(tiles, source, mask, w, h, ov), oh, ow, filter)


def planes_of_blended(fmt: int, cs: int, blended: np.ndarray, source: np.ndarray, mask, size=None, filter: int = 0):
    """The planes of format ``fmt`` from the blended frame itself: masked, scaled to ``size = (ow, oh)`` where one is set,
    then BGRX (format 0) as it is or the existing 8-bit encode -- a deep format carries ``257 u8`` while a mask is set."""
    out = masked_of_blended(blended, source, mask)
    if size is not None:
        return TO.planes_of_blended(fmt, cs, out, None, size[1], size[0], filter, False)
    return [out] if fmt == 0 else O.encode8(fmt, cs, out)


def box(mask: np.ndarray, B: int, Bh: int):
    """``(x0, y0, x1, y1)``: the rectangle of blended coordinates that holds every pixel of the ``B x Bh`` frame whose mask
    texel is not white -- the bounding rectangle of those pixels; ``(0, 0, 0, 0)`` where there is none."""
    ys, xs = S.texel(np.arange(Bh), mask.shape[0], Bh), S.texel(np.arange(B), mask.shape[1], B)
    a = 765 - mask[ys[:, None], xs[None, :], :3].astype(np.int64).sum(-1)
    if not a.any():
        return (0, 0, 0, 0)
    cols, rows = np.flatnonzero(a.any(0)), np.flatnonzero(a.any(1))
    return (int(cols[0]), int(rows[0]), int(cols[-1]) + 1, int(rows[-1]) + 1)
