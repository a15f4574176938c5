"""Definition of the RGB frame formats of ju_process_frame (JU_FMT_BGR24 .. JU_FMT_BGR96F, values 32..41), in numpy.

The GPU kernels (csrc/colour_kernels.hip, "RGB formats") compute exactly this, bit for bit.  No colour space is involved:
an RGB frame is the network's BGRX frame in another layout and, for the deep formats, another sample kind.

* Planes as a caller holds them: packed formats ONE array -- BGR24 / RGB24 [H][W][3] uint8, RGBX [H][W][4] uint8, BGRX64
  [H][W][4] uint16, BGR96F [H][W][3] float32 (0..255) -- planar formats three [H][W] arrays R, G, B: RGBP8 uint8, RGBP10 /
  RGBP16 uint16, RGBPH float16, RGBPS float32 (0..1).
* decode_planes: planes -> the u8 BGRX frame the network consumes (X = 0).  16-bit word P: (P + 128) // 257; 10-bit value p
  (the low 10 bits): P = (p << 6) | (p >> 4), then that rule; RGBPH / RGBPS v (f16 widened to f32, exact):
  floor(clamp(v, 0, 1) * 255 + 0.5) as ONE f32 multiply and ONE f32 add (no fused multiply-add); BGR96F:
  floor(clamp(v, 0, 255) + 0.5); NaN decodes to 0, +-inf clamps.
* encode_planes: from the u8 frame (8-bit formats: a permutation, X = 0; deep: P = 257 u8, 10-bit P >> 6, RGBPS
  f32(u8) / f32(255), RGBPH that value rounded to f16, BGR96F f32(u8)) or, the deep formats, from the f16 state s
  (t = s + 0.5 in f32; P = p_from_state; 10-bit P >> 6; RGBPS clamp(t, 0, 1); RGBPH that rounded to f16 to nearest even;
  BGR96F clamp(t, 0, 1) * 255, one f32 multiply).
"""

import numpy as np

from yuv10_reference import p_from_state

(FMT_BGR24, FMT_RGB24, FMT_RGBX, FMT_BGRX64, FMT_RGBP8, FMT_RGBP10, FMT_RGBP16, FMT_RGBPH, FMT_RGBPS,
 FMT_BGR96F) = range(32, 42)
NEW_FORMATS = tuple(range(32, 42))
FORMAT_NAMES = {FMT_BGR24: "bgr24", FMT_RGB24: "rgb24", FMT_RGBX: "rgbx", FMT_BGRX64: "bgrx64", FMT_RGBP8: "rgbp8",
                FMT_RGBP10: "rgbp10", FMT_RGBP16: "rgbp16", FMT_RGBPH: "rgbph", FMT_RGBPS: "rgbps", FMT_BGR96F: "bgr96f"}
DEEP = (FMT_BGRX64, FMT_RGBP10, FMT_RGBP16, FMT_RGBPH, FMT_RGBPS, FMT_BGR96F)
EIGHT = (FMT_BGR24, FMT_RGB24, FMT_RGBX, FMT_RGBP8)
PLANAR = (FMT_RGBP8, FMT_RGBP10, FMT_RGBP16, FMT_RGBPH, FMT_RGBPS)
FLOAT = (FMT_RGBPH, FMT_RGBPS, FMT_BGR96F)
DTYPE = {FMT_BGR24: np.uint8, FMT_RGB24: np.uint8, FMT_RGBX: np.uint8, FMT_BGRX64: np.uint16, FMT_RGBP8: np.uint8,
         FMT_RGBP10: np.uint16, FMT_RGBP16: np.uint16, FMT_RGBPH: np.float16, FMT_RGBPS: np.float32,
         FMT_BGR96F: np.float32}
# packed formats: samples per pixel, and the position of B, G, R in a pixel
PACKED = {FMT_BGR24: (3, (0, 1, 2)), FMT_RGB24: (3, (2, 1, 0)), FMT_RGBX: (4, (2, 1, 0)), FMT_BGRX64: (4, (0, 1, 2)),
          FMT_BGR96F: (3, (0, 1, 2))}
# the kind of a format's samples
KIND = {FMT_BGR24: "u8", FMT_RGB24: "u8", FMT_RGBX: "u8", FMT_RGBP8: "u8", FMT_BGRX64: "w16", FMT_RGBP16: "w16",
        FMT_RGBP10: "w10", FMT_RGBPH: "h", FMT_RGBPS: "s", FMT_BGR96F: "f255"}


def blank_planes(fmt, h, w):
    if fmt in PLANAR:
        return [np.zeros((h, w), DTYPE[fmt]) for _ in range(3)]
    return [np.zeros((h, w, PACKED[fmt][0]), DTYPE[fmt])]


# ---- samples -> u8 ----------------------------------------------------------------------------------------------------
def u8_from_word16(p):
    return ((np.asarray(p).astype(np.int64) + 128) // 257).astype(np.uint8)


def u8_from_word10(word):
    p = np.asarray(word).astype(np.int64) & 0x3ff               # (the upper 6 bits are ignored)
    return u8_from_word16((p << 6) | (p >> 4))


def _clamp(v, top):
    v = np.asarray(v).astype(np.float32)                        # (f16 -> f32: exact)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), np.float32(0), np.minimum(np.maximum(v, np.float32(0)), np.float32(top)))


def u8_from_unit(v):
    """RGBPS / RGBPH: floor(clamp(v, 0, 1) * 255 + 0.5), an f32 multiply followed by an f32 add."""
    prod = (_clamp(v, 1.0) * np.float32(255.0)).astype(np.float32)
    return np.floor((prod + np.float32(0.5)).astype(np.float32)).astype(np.uint8)


def u8_from_f255(v):
    """BGR96F: floor(clamp(v, 0, 255) + 0.5)."""
    return np.floor((_clamp(v, 255.0) + np.float32(0.5)).astype(np.float32)).astype(np.uint8)


_TO_U8 = {"u8": lambda a: np.asarray(a, np.uint8), "w16": u8_from_word16, "w10": u8_from_word10, "h": u8_from_unit,
          "s": u8_from_unit, "f255": u8_from_f255}


def channels(fmt, planes):
    """The format's (B, G, R) sample arrays [H][W] of a frame's planes."""
    if fmt in PLANAR:
        r, g, b = planes
        return b, g, r
    _, (ib, ig, ir) = PACKED[fmt]
    a = planes[0]
    return a[..., ib], a[..., ig], a[..., ir]


def decode_planes(fmt, planes):
    """planes -> [H][W][4] uint8 BGRX (X = 0): the frame the network consumes."""
    b, g, r = channels(fmt, planes)
    out = np.zeros(b.shape + (4,), np.uint8)
    for k, c in enumerate((b, g, r)):
        out[..., k] = _TO_U8[KIND[fmt]](c)
    return out


# ---- u8 / state -> samples -------------------------------------------------------------------------------------------
def samples_from_u8(kind, u8):
    u8 = np.asarray(u8, np.uint8)
    if kind == "u8":
        return u8.copy()
    if kind == "w16":
        return (u8.astype(np.uint32) * 257).astype(np.uint16)
    if kind == "w10":
        return ((u8.astype(np.uint32) * 257) >> 6).astype(np.uint16)
    if kind == "f255":
        return u8.astype(np.float32)
    unit = (u8.astype(np.float32) / np.float32(255.0)).astype(np.float32)   # one correctly rounded f32 division
    return unit.astype(np.float16) if kind == "h" else unit


def samples_from_state(kind, s):
    """`s`: float16 [...]; the deep kinds only."""
    s = np.asarray(s)
    assert s.dtype == np.float16 and kind != "u8"
    if kind in ("w16", "w10"):
        p = p_from_state(s[..., None].repeat(3, axis=-1))[..., 0]
        return (p >> (6 if kind == "w10" else 0)).astype(np.uint16)
    t = (s.astype(np.float32) + np.float32(0.5)).astype(np.float32)
    unit = np.minimum(np.maximum(t, np.float32(0)), np.float32(1))
    if kind == "s":
        return unit
    if kind == "h":
        return unit.astype(np.float16)                          # (numpy rounds to nearest even)
    return (unit * np.float32(255.0)).astype(np.float32)


def assemble(fmt, b, g, r):
    """(B, G, R) sample arrays -> the planes of the format (X = 0)."""
    if fmt in PLANAR:
        return [np.ascontiguousarray(r), np.ascontiguousarray(g), np.ascontiguousarray(b)]
    n, (ib, ig, ir) = PACKED[fmt]
    a = np.zeros(b.shape + (n,), DTYPE[fmt])
    a[..., ib], a[..., ig], a[..., ir] = b, g, r
    return [a]


def encode_planes(fmt, frame=None, state=None):
    """What a runtime writes for an output of the format: from the u8 BGRX `frame`, or -- `state` given, deep formats --
    from the f16 state [H][W][4] (B, G, R, unused)."""
    kind = KIND[fmt]
    if state is not None:
        return assemble(fmt, *(samples_from_state(kind, np.asarray(state)[..., k]) for k in range(3)))
    return assemble(fmt, *(samples_from_u8(kind, frame[..., k]) for k in range(3)))
