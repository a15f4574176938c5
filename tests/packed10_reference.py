"""Definition of the packed 10-bit frame formats of ju_process_frame (numpy, integers only): JU_FMT_V210, JU_FMT_Y210,
JU_FMT_Y410, JU_FMT_X2RGB10 and JU_FMT_X2BGR10.

Only the WORDS are stated here.  The samples and every bit of arithmetic are those of the planar formats of the same
sampling and are reached by delegation: 10-bit 4:2:2 / 4:4:4 YUV samples through tests/yuv_sampled_reference.py (decode,
encode10) with the sample P of tests/yuv10_reference.py, 10-bit RGB samples through tests/rgb_reference.py as RGBP10's and,
from a 16-bit frame, tests/output_reference.py.  No coefficient is restated.  The GPU kernels (csrc/colour_kernels.hip)
give these bytes exactly.

Samples: YUV formats (y, u, v) with y [H][W] and u, v [H][W/2] (V210, Y210) or [H][W] (Y410); RGB formats (b, g, r), each
[H][W]; uint16 holding 0..1023.  Every format is ONE plane of little-endian words:

* V210: uint32 [H][4 ceil(W / 6)].  A group of six pixels is four words of three samples at bits 0-9, 10-19, 20-29:
  w0 = Cb0 Y0 Cr0, w1 = Y1 Cb1 Y2, w2 = Cr1 Y3 Cb2, w3 = Y4 Cr2 Y5.  The last group is whole; its sample slots beyond W
  (W mod 6 = 2 or 4) are ignored on input and 0 on output.
* Y210: uint16 [H][2W]: Y0 U Y1 V per pixel pair, word = value << 6 (the low 6 bits ignored in, 0 out), as P010 / P210.
* Y410: uint32 [H][W]: U bits 0-9, Y 10-19, V 20-29.
* X2RGB10: uint32 [H][W]: B bits 0-9, G 10-19, R 20-29.  X2BGR10: R bits 0-9, G 10-19, B 20-29.
* Bits 30-31 of every 32-bit word are ignored on input and 0 on output.
"""

import numpy as np

import output_reference as O
import rgb_reference as G
import yuv10_reference as T
import yuv_sampled_reference as YS

FMT_V210, FMT_Y210, FMT_Y410, FMT_X2RGB10, FMT_X2BGR10 = 48, 49, 50, 45, 44
NEW_FORMATS = (FMT_V210, FMT_Y210, FMT_Y410, FMT_X2RGB10, FMT_X2BGR10)
FORMAT_NAMES = {FMT_V210: "v210", FMT_Y210: "y210", FMT_Y410: "y410", FMT_X2RGB10: "x2rgb10", FMT_X2BGR10: "x2bgr10"}
YUV = (FMT_V210, FMT_Y210, FMT_Y410)
RGB = (FMT_X2RGB10, FMT_X2BGR10)
SAMPLING = {FMT_V210: 422, FMT_Y210: 422, FMT_Y410: 444}
DTYPE = {FMT_V210: np.uint32, FMT_Y210: np.uint16, FMT_Y410: np.uint32, FMT_X2RGB10: np.uint32, FMT_X2BGR10: np.uint32}
# the bit of the first, second and third sample of a 32-bit word
SLOTS = (0, 10, 20)
# X2RGB10 / X2BGR10: the slot of (b, g, r)
RGB_SLOTS = {FMT_X2RGB10: (0, 1, 2), FMT_X2BGR10: (2, 1, 0)}
# bits of a word that carry no sample
IGNORED32 = 0xC0000000
IGNORED_Y210 = 0x003F


def groups(w):
    """V210: groups of six pixels in a row of w pixels."""
    return (w + 5) // 6


def row_bytes(fmt, w):
    """The bytes of one row that hold samples (the least |stride|)."""
    return 16 * groups(w) if fmt == FMT_V210 else 4 * w


def row_words(fmt, w):
    """The words of one row of the format's array."""
    return row_bytes(fmt, w) // np.dtype(DTYPE[fmt]).itemsize


def sample_shapes(fmt, h, w):
    """The shapes of the three sample arrays of an h x w frame."""
    if fmt in RGB:
        return (h, w), (h, w), (h, w)
    c = YS.chroma_shape(SAMPLING[fmt], h, w)
    return (h, w), c, c


def _word(a, b, c):
    return (a.astype(np.uint32) | (b.astype(np.uint32) << SLOTS[1]) | (c.astype(np.uint32) << SLOTS[2])).astype(np.uint32)


def _fields(word):
    return tuple(((word >> s) & 0x3ff).astype(np.uint16) for s in SLOTS)


def _check(fmt, a, b, c):
    shapes = sample_shapes(fmt, *a.shape)
    if (a.shape, b.shape, c.shape) != shapes:
        raise ValueError("sample arrays of the wrong shapes")
    for s in (a, b, c):
        if s.size and int(np.asarray(s).max()) > 1023:
            raise ValueError("samples are 10-bit values")


def to_v210(y, u, v):
    h, w = y.shape
    g = groups(w)
    yp = np.zeros((h, 6 * g), np.uint32)
    up = np.zeros((h, 3 * g), np.uint32)
    vp = np.zeros((h, 3 * g), np.uint32)
    yp[:, :w], up[:, :w // 2], vp[:, :w // 2] = y, u, v                      # (slots beyond W stay 0)
    yp, up, vp = yp.reshape(h, g, 6), up.reshape(h, g, 3), vp.reshape(h, g, 3)
    out = np.empty((h, g, 4), np.uint32)
    out[..., 0] = _word(up[..., 0], yp[..., 0], vp[..., 0])
    out[..., 1] = _word(yp[..., 1], up[..., 1], yp[..., 2])
    out[..., 2] = _word(vp[..., 1], yp[..., 3], up[..., 2])
    out[..., 3] = _word(yp[..., 4], vp[..., 2], yp[..., 5])
    return out.reshape(h, 4 * g)


def from_v210(plane, w):
    """A V210 array (at least 4 ceil(W / 6) words a row; more are padding) -> (y, u, v) of width w."""
    h = plane.shape[0]
    g = groups(w)
    if w % 2 or plane.shape[1] < 4 * g:
        raise ValueError("a V210 row holds whole groups of six pixels of an even width")
    q = np.asarray(plane)[:, :4 * g].astype(np.uint32).reshape(h, g, 4)
    f = [_fields(q[..., k]) for k in range(4)]
    y = np.stack([f[0][1], f[1][0], f[1][2], f[2][1], f[3][0], f[3][2]], axis=-1).reshape(h, 6 * g)
    u = np.stack([f[0][0], f[1][1], f[2][2]], axis=-1).reshape(h, 3 * g)
    v = np.stack([f[0][2], f[2][0], f[3][1]], axis=-1).reshape(h, 3 * g)
    return y[:, :w].copy(), u[:, :w // 2].copy(), v[:, :w // 2].copy()


def to_words(fmt, a, b, c):
    """The one array a caller holds of the samples (y, u, v) or (b, g, r), as a one-element list; every ignored bit and
    unused slot is 0."""
    a, b, c = (np.asarray(s) for s in (a, b, c))
    _check(fmt, a, b, c)
    if fmt == FMT_V210:
        return [to_v210(a, b, c)]
    if fmt == FMT_Y210:
        out = np.empty((a.shape[0], 2 * a.shape[1]), np.uint16)
        out[:, 0::4], out[:, 1::4], out[:, 2::4], out[:, 3::4] = (s.astype(np.uint16) << 6 for s in (a[:, 0::2], b, a[:, 1::2], c))
        return [out]
    if fmt == FMT_Y410:
        return [_word(b, a, c)]                                              # U, Y, V
    if fmt in RGB:
        slot = [None] * 3
        for s, k in zip((a, b, c), RGB_SLOTS[fmt]):
            slot[k] = s
        return [_word(*slot)]
    raise ValueError(f"unknown format {fmt}")


def from_words(fmt, planes, width=None):
    """A caller's array -> the samples (y, u, v) or (b, g, r); bits the format ignores are ignored.  V210: `width` (the
    array cannot tell it; default: all six pixels of every group)."""
    plane = np.asarray(planes[0])
    if fmt == FMT_V210:
        return from_v210(plane, 6 * (plane.shape[1] // 4) if width is None else width)
    if fmt == FMT_Y210:
        s = plane >> 6
        y = np.empty((plane.shape[0], plane.shape[1] // 2), np.uint16)
        y[:, 0::2], y[:, 1::2] = s[:, 0::4], s[:, 2::4]
        return y, s[:, 1::4].copy(), s[:, 3::4].copy()
    if fmt == FMT_Y410:
        u, y, v = _fields(plane)
        return y, u, v
    if fmt in RGB:
        f = _fields(plane)
        return tuple(f[k] for k in RGB_SLOTS[fmt])
    raise ValueError(f"unknown format {fmt}")


def blank_planes(fmt, h, w):
    """The zeroed array of a frame of the format (what to_words gives of zero samples)."""
    return to_words(fmt, *(np.zeros(s, np.uint16) for s in sample_shapes(fmt, h, w)))


def junk(fmt, planes, width, rng):
    """A copy of the planes with random bits wherever the format ignores them: bits 30-31, the low 6 bits of a Y210
    word, the unused slots of V210's last group."""
    a = planes[0].copy()
    if fmt == FMT_Y210:
        return [a | rng.integers(0, IGNORED_Y210 + 1, a.shape).astype(np.uint16)]
    a |= rng.integers(0, 4, a.shape).astype(np.uint32) << 30
    if fmt == FMT_V210 and width % 6:
        # the slots of the last group beyond W: those from_v210 does not return
        g = groups(width)
        keep = to_v210(*(np.full(s, 1023, np.uint16) for s in sample_shapes(fmt, a.shape[0], width)))
        noise = rng.integers(0, 1 << 30, (a.shape[0], 4 * g)).astype(np.uint32)
        a[:, :4 * g] |= noise & ~keep & np.uint32(0x3FFFFFFF)
    return [a]


def decode_planes(fmt, cs, planes, width=None):
    """The BGRX frame the network consumes for a caller's array.  V210 / Y210 decode as P210, Y410 as I410, the RGB
    formats as RGBP10 (`cs` ignored)."""
    s = from_words(fmt, planes, width)
    if fmt in RGB:
        b, g, r = s
        return G.decode_planes(G.FMT_RGBP10, [r, g, b])
    return YS.decode(*s, cs, SAMPLING[fmt], deep=True)


def encode_planes(fmt, cs, frame=None, state=None, frame16=None):
    """What a runtime writes for an output of the format: from the 8-bit frame (P = 257 u8), from the f16 state
    (`state` given) or from a 16-bit frame [H][W][3 or 4] of samples P (`frame16` given: the output stage)."""
    if fmt in RGB:
        if frame16 is not None:
            r, g, b = (O.samples_from_p("w10", np.asarray(frame16)[..., k]) for k in (2, 1, 0))
        else:
            r, g, b = G.encode_planes(G.FMT_RGBP10, frame=frame, state=state)
        return to_words(fmt, b, g, r)
    if frame16 is not None:
        p = np.asarray(frame16)[..., :3].astype(np.int64)
    else:
        p = T.p_from_state(state) if state is not None else T.p_from_u8(frame)
    return to_words(fmt, *YS.encode10(p, cs, SAMPLING[fmt]))
