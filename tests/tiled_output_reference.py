"""The definition of a tiled frame under an output size in numpy (docs/tiled.md "An output size"): the blended frame of
tiled_reference / tiled_deep_reference, rounded to bytes (16-bit words), THEN scaled by scale_filter_reference and encoded
by output_reference -- nothing of its own.  tile_stitch_scale_kernel and tile_stitch_scale_state_kernel
(csrc/tile_kernels.hip) compute ``frame8`` / ``frame16`` byte for byte without storing the blended frame."""

from __future__ import annotations

import numpy as np

import output_reference as O
import scale_filter_reference as F
import tiled_deep_reference as D
import tiled_reference as T


def frame8(tiles, src_w: int, src_h: int, w: int, h: int, ov: int, oh: int, ow: int, filter: int) -> np.ndarray:
    """``[oh, ow, 4]`` uint8 BGRX (X = 0) of the tiles' 8-bit outputs: ``scale8(stitch(tiles))``."""
    return F.scale8(T.stitch(tiles, src_w, src_h, w, h, ov), oh, ow, filter)


def frame16(p_tiles, src_w: int, src_h: int, w: int, h: int, ov: int, oh: int, ow: int, filter: int) -> np.ndarray:
    """``[oh, ow, 4]`` uint16 (X = 0) of the tiles' 16-bit samples ``P``: ``scale16(stitch16(p_tiles))``."""
    return F.scale16(D.stitch16(p_tiles, src_w, src_h, w, h, ov), oh, ow, filter)


def planes_of_blended(fmt: int, cs: int, blended8, blended16, oh: int, ow: int, filter: int, deep: bool):
    """``planes`` from the blended frames themselves (``T.stitch`` / ``D.stitch16`` of the tiles): the frame of the route
    scaled, then BGRX (format 0) as it is or the existing encode."""
    if deep:
        assert fmt in O.DEEP
        return O.encode16(fmt, cs, F.scale16(blended16, oh, ow, filter))
    out8 = F.scale8(blended8, oh, ow, filter)
    return [out8] if fmt == 0 else O.encode8(fmt, cs, out8)


def planes(fmt: int, cs: int, tiles, p_tiles, src_w: int, src_h: int, w: int, h: int, ov: int, oh: int, ow: int, filter: int,
           deep: bool):
    """The planes of format ``fmt`` of a tiled frame under the output size ``ow x oh``.  ``deep``: the 16-bit route -- a
    deep format while ``ju_tiled_set_deep_from_state`` is 1 and "hbd_from_state" is 1 -- from ``p_tiles``; else the 8-bit
    route from ``tiles``, on which a deep format carries ``257 u8``.  BGRX is the 8-bit frame itself."""
    blended8 = None if deep else T.stitch(tiles, src_w, src_h, w, h, ov)
    blended16 = D.stitch16(p_tiles, src_w, src_h, w, h, ov) if deep else None
    return planes_of_blended(fmt, cs, blended8, blended16, oh, ow, filter, deep)
