"""Definition of the YUV <-> BGRX conversions of ju_process_frame for every chroma siting and matrix (numpy, integers only).

`colorspace` = JU_CS_* | JU_CHROMA_*: the low byte is the matrix and range (0 .. 3 as tests/yuv_reference.py, 4 / 5 BT.2020
non-constant luminance, limited / full: K_r = 0.2627, K_b = 0.0593), bits 8-9 the siting.  With JU_CHROMA_LEFT and the
matrices 0 .. 3 every byte and word equals the existing definitions (tests/yuv_reference.py, yuv10_reference.py,
yuv_sampled_reference.py, packed10_reference.py): tests/test_chroma_siting_cpu.py holds this file to them.  The GPU kernels
(csrc/colour_kernels.hip) compute exactly this, bit for bit; INTEGRATION.md states the formulas.

Luma samples sit at integer (x, y).  Chroma sample (i, j) of a 4:2:0 plane sits at

* LEFT     (2i,       2j + 1/2)   co-sited horizontally, centred vertically (MPEG-2 / H.264),
* CENTER   (2i + 1/2, 2j + 1/2)   centred on both axes (JPEG / MPEG-1),
* TOPLEFT  (2i,       2j)         co-sited on both axes (H.273 chroma_sample_loc_type 2).

4:2:2 has the horizontal axis only (TOPLEFT is LEFT there); 4:4:4 has a sample per pixel and ignores the siting.

Per axis, every index clamped to its plane:

* decode, co-sited: position 2i takes c[i], 2i + 1 takes (c[i] + c[i + 1]) / 2           -- integers at a scale of 2;
* decode, centred:  position 2i takes (3 c[i] + c[i - 1]) / 4, 2i + 1 (3 c[i] + c[i + 1]) / 4 -- integers at a scale of 4;
* encode, co-sited: [1, 2, 1] on 2i - 1 (clamped to 0), 2i, 2i + 1                      -- a sum of weight 4;
* encode, centred:  [1, 1] on 2i, 2i + 1                                                -- a sum of weight 2.

Nothing is rounded between the axes or between the resampling and the matrix.  Every siting is brought to ONE scale by an
exact power of two -- SCALE = 16 for the upsampled chroma (and the luma term) of a decode and for the chroma sum of an
encode -- so there is one rounding shift at the end, 4 bits longer than the coefficients' 16 (8-bit, 10-bit decode) or 32
(10-bit encode).  (2a + 2^19) >> 20 = (a + 2^18) >> 19: doubling both is free, which is why LEFT keeps today's bytes.

Accumulator widths (asserted below for every matrix): the 8- and 10-bit decodes and the 8-bit encode stay within 32 bits
signed at the scale of 16; the 10-bit encode's products reach 2^46 and are summed in 64 bits, as in yuv10_reference.py.
"""

import numpy as np

import packed10_reference as P
import yuv10_reference as T
import yuv_reference as Y
import yuv_sampled_reference as YS

CS_BT601_LIMITED, CS_BT601_FULL, CS_BT709_LIMITED, CS_BT709_FULL, CS_BT2020_LIMITED, CS_BT2020_FULL = range(6)
CHROMA_LEFT, CHROMA_CENTER, CHROMA_TOPLEFT = 0 << 8, 1 << 8, 2 << 8
MATRICES = tuple(range(6))
SITINGS = (CHROMA_LEFT, CHROMA_CENTER, CHROMA_TOPLEFT)
SITING_NAMES = {CHROMA_LEFT: "left", CHROMA_CENTER: "center", CHROMA_TOPLEFT: "topleft"}
MATRIX_NAMES = {0: "601-limited", 1: "601-full", 2: "709-limited", 3: "709-full", 4: "2020-limited", 5: "2020-full"}
K_R_K_B = {0: (0.299, 0.114), 1: (0.299, 0.114), 2: (0.2126, 0.0722), 3: (0.2126, 0.0722), 4: (0.2627, 0.0593),
           5: (0.2627, 0.0593)}
SCALE_LOG2 = 4
SCALE = 1 << SCALE_LOG2

SAMPLING = dict(YS.SAMPLING)
SAMPLING.update(P.SAMPLING)
DEEP = tuple(YS.DEEP) + tuple(P.YUV)
FORMAT_NAMES = dict(YS.FORMAT_NAMES)
FORMAT_NAMES.update({f: P.FORMAT_NAMES[f] for f in P.YUV})


def split(colorspace):
    """(matrix 0 .. 5, siting: one of SITINGS) of a `colorspace` value; ValueError for what a runtime refuses."""
    if colorspace < 0 or colorspace >> 10:
        raise ValueError(f"unknown colour space {colorspace}: bits above bit 9")
    siting = colorspace & 0x300
    if siting not in SITINGS:
        raise ValueError(f"unknown chroma siting {siting >> 8}")
    matrix = colorspace & 0xff
    if matrix not in MATRICES:
        raise ValueError(f"unknown colour space {matrix}")
    return matrix, siting


def axes(sampling, siting):
    """(horizontal, vertical) of a sampling under a siting: "co", "centre" or None (the axis is not subsampled)."""
    if sampling == 444:
        return None, None
    horizontal = "centre" if siting == CHROMA_CENTER else "co"
    if sampling == 422:
        return horizontal, None
    return horizontal, ("co" if siting == CHROMA_TOPLEFT else "centre")


def _params(matrix):
    kr, kb = K_R_K_B[matrix]
    return kr, kb, 1.0 - kr - kb, matrix % 2 == 0


def decode_coefficients(matrix, deep=False):
    """(kY, kRV, kBU, kGU, kGV) x 65536 and oY: the formulas of Y.decode_coefficients / T.decode10_coefficients."""
    kr, kb, kg, limited = _params(matrix)
    if deep:
        s, ky, oy = (255.0 / 896.0, 255.0 / 876.0, 64) if limited else (255.0 / 1023.0, 255.0 / 1023.0, 0)
    else:
        s, ky, oy = (255.0 / 224.0, 255.0 / 219.0, 16) if limited else (1.0, 1.0, 0)
    real = [ky, 2 * (1 - kr) * s, 2 * (1 - kb) * s, 2 * kb * (1 - kb) / kg * s, 2 * kr * (1 - kr) / kg * s]
    return tuple(Y.round_half_away(k * 65536) for k in real), oy


def _encode_real(matrix, sy, sc):
    kr, kb, kg, _ = _params(matrix)
    du, dv = sc / (2 * (1 - kb)), sc / (2 * (1 - kr))
    return (sy * kr, sy * kg, sy * kb), (-kr * du, -kg * du, (1 - kb) * du), ((1 - kr) * dv, -kg * dv, -kb * dv)


def encode_coefficients(matrix):
    """The nine coefficients x 65536 (rows Y, U, V; columns R, G, B) and oY: the formulas of Y.encode_coefficients."""
    limited = _params(matrix)[3]
    real = _encode_real(matrix, *((219.0 / 255.0, 224.0 / 255.0) if limited else (1.0, 1.0)))
    return tuple(tuple(Y.round_half_away(k * 65536) for k in row) for row in real), (16 if limited else 0)


def encode10_coefficients(matrix):
    """round_half_away(k / 65535 * 2^32) for the nine coefficients that take P to 10-bit codes, and oY (T.encode10_coefficients)."""
    limited = _params(matrix)[3]
    real = _encode_real(matrix, *((876.0, 896.0) if limited else (1023.0, 1023.0)))
    return tuple(tuple(Y.round_half_away(k / 65535.0 * 4294967296.0) for k in row) for row in real), (64 if limited else 0)


# ---- the accumulator widths, for every matrix ---------------------------------------------------------------------------
for _m in MATRICES:
    for _deep, _top in ((False, 255), (True, 1023)):
        (_ky, _krv, _kbu, _kgu, _kgv), _ = decode_coefficients(_m, _deep)
        _chroma = SCALE * (_top + 1) // 2                         # |SCALE x (c - mid)| at most
        assert _ky * SCALE * _top + max(_krv, _kbu, _kgu + _kgv) * _chroma + (1 << 19) < 1 << 31, "decode: 32 bits"
    _rows, _ = encode_coefficients(_m)
    assert all(sum(abs(k) for k in row) * SCALE * 255 + (1 << 19) < 1 << 31 for row in _rows), "8-bit encode: 32 bits"
    _rows, _ = encode10_coefficients(_m)
    assert all(abs(k) < 1 << 26 for row in _rows for k in row), "10-bit encode: coefficients below 2^26"
    assert all(sum(abs(k) for k in row) * SCALE * 65535 + (1 << 35) < 1 << 63 for row in _rows), "10-bit encode: 64 bits"
    assert SCALE * 65535 < 1 << 31, "10-bit encode: the sample sums are 32-bit"


# ---- resampling ---------------------------------------------------------------------------------------------------------
def upsample_axis(c, kind, axis):
    """One axis of the decode, n -> 2n samples along `axis`, in integers: ("co": 2 x, "centre": 4 x) the interpolated value."""
    c = np.moveaxis(np.asarray(c).astype(np.int64), axis, 0)
    n = c.shape[0]
    i = np.arange(n)
    before, after = c[np.maximum(i - 1, 0)], c[np.minimum(i + 1, n - 1)]
    out = np.empty((2 * n,) + c.shape[1:], np.int64)
    if kind == "co":
        out[0::2], out[1::2] = 2 * c, c + after
    else:
        out[0::2], out[1::2] = 3 * c + before, 3 * c + after
    return np.moveaxis(out, 0, axis)


AXIS_SCALE_LOG2 = {"co": 1, "centre": 2, None: 0}


def upsample16(c, sampling, siting, h, w):
    """SCALE x the chroma plane c at every luma position [H][W] (int64)."""
    if c.shape != YS.chroma_shape(sampling, h, w):
        raise ValueError("chroma plane of the wrong shape")
    horizontal, vertical = axes(sampling, siting)
    out = np.asarray(c).astype(np.int64)
    if vertical is not None:
        out = upsample_axis(out, vertical, 0)
    if horizontal is not None:
        out = upsample_axis(out, horizontal, 1)
    return out << (SCALE_LOG2 - AXIS_SCALE_LOG2[horizontal] - AXIS_SCALE_LOG2[vertical])


def decode_terms(y, u, v, colorspace, sampling, deep=False):
    """The three accumulators (R, G, B) of `decode` before the shift by 16 + SCALE_LOG2, int64 [H][W] each."""
    matrix, siting = split(colorspace)
    (ky, krv, kbu, kgu, kgv), oy = decode_coefficients(matrix, deep)
    h, w = y.shape
    mid = SCALE * (512 if deep else 128)
    du = upsample16(u, sampling, siting, h, w) - mid
    dv = upsample16(v, sampling, siting, h, w) - mid
    yd = ky * SCALE * (y.astype(np.int64) - oy)
    half = 1 << (15 + SCALE_LOG2)
    return yd + krv * dv + half, yd - kgu * du - kgv * dv + half, yd + kbu * du + half


def decode(y, u, v, colorspace, sampling, deep=False):
    """Y, U, V samples (uint8, or 10-bit values in uint16 where `deep`) -> [H][W][4] uint8 BGRX (X = 0)."""
    r, g, b = decode_terms(y, u, v, colorspace, sampling, deep)
    assert max(int(np.abs(t).max()) for t in (r, g, b)) < 1 << 31
    out = np.zeros(y.shape + (4,), np.uint8)
    for k, t in ((2, r), (1, g), (0, b)):
        out[..., k] = np.clip(t >> (16 + SCALE_LOG2), 0, 255)
    return out


def downsample_axis(p, kind, axis):
    """One axis of the encode, 2n -> n sums along `axis`: "co" [1, 2, 1] about 2i (weight 4), "centre" [1, 1] (weight 2)."""
    p = np.moveaxis(np.asarray(p).astype(np.int64), axis, 0)
    even, odd = p[0::2], p[1::2]
    if kind == "co":
        before = np.concatenate([p[:1], odd[:-1]], axis=0)        # sample 2i - 1, clamped to 0
        out = before + 2 * even + odd
    else:
        out = even + odd
    return np.moveaxis(out, 0, axis)


SUM_WEIGHT_LOG2 = {"co": 2, "centre": 1, None: 0}


def chroma_sum16(p, sampling, siting):
    """The chroma sum of one channel p [H][W], at SCALE: SCALE x the filtered value at each chroma position (int64)."""
    YS.chroma_shape(sampling, *p.shape)
    horizontal, vertical = axes(sampling, siting)
    out = np.asarray(p).astype(np.int64)
    if vertical is not None:
        out = downsample_axis(out, vertical, 0)
    if horizontal is not None:
        out = downsample_axis(out, horizontal, 1)
    return out << (SCALE_LOG2 - SUM_WEIGHT_LOG2[horizontal] - SUM_WEIGHT_LOG2[vertical])


def encode(bgrx, colorspace, sampling):
    """[H][W][4 (or 3)] uint8 BGR(X) -> (y, u, v) uint8 samples."""
    matrix, siting = split(colorspace)
    ((cyr, cyg, cyb), cu, cv), oy = encode_coefficients(matrix)
    b, g, r = (bgrx[..., k].astype(np.int64) for k in range(3))
    y = np.clip(oy + ((cyr * r + cyg * g + cyb * b + (1 << 15)) >> 16), 0, 255).astype(np.uint8)
    sr, sg, sb = (chroma_sum16(c, sampling, siting) for c in (r, g, b))

    def chroma(c):
        acc = c[0] * sr + c[1] * sg + c[2] * sb + (1 << (15 + SCALE_LOG2))
        assert int(np.abs(acc).max()) < 1 << 31
        return np.clip(128 + (acc >> (16 + SCALE_LOG2)), 0, 255).astype(np.uint8)
    return y, chroma(cu), chroma(cv)


def encode10(p, colorspace, sampling):
    """[H][W][3 (or 4)] 16-bit samples P (B, G, R; T.p_from_state / T.p_from_u8) -> (y, u, v) uint16 samples 0..1023."""
    matrix, siting = split(colorspace)
    ((cyr, cyg, cyb), cu, cv), oy = encode10_coefficients(matrix)
    b, g, r = (p[..., k].astype(np.int64) for k in range(3))
    y = np.clip(oy + ((cyr * r + cyg * g + cyb * b + (1 << 31)) >> 32), 0, 1023).astype(np.uint16)
    sr, sg, sb = (chroma_sum16(c, sampling, siting) for c in (r, g, b))

    def chroma(c):
        acc = c[0] * sr + c[1] * sg + c[2] * sb + (1 << (31 + SCALE_LOG2))
        return np.clip(512 + (acc >> (32 + SCALE_LOG2)), 0, 1023).astype(np.uint16)
    return y, chroma(cu), chroma(cv)


# ---- the planes a caller holds: every YUV format of the table -----------------------------------------------------------
def to_words(fmt, y, u, v):
    return P.to_words(fmt, y, u, v) if fmt in P.YUV else YS.to_words(fmt, y, u, v)


def from_words(fmt, planes, width=None):
    return P.from_words(fmt, planes, width) if fmt in P.YUV else YS.from_words(fmt, planes)


def blank_planes(fmt, h, w):
    return P.blank_planes(fmt, h, w) if fmt in P.YUV else YS.blank_planes(fmt, h, w)


def decode_planes(fmt, colorspace, planes, width=None):
    """The BGRX frame the network consumes for a caller's planes (V210: `width`)."""
    return decode(*from_words(fmt, planes, width), colorspace, SAMPLING[fmt], fmt in DEEP)


def encode_planes(fmt, colorspace, frame=None, state=None, frame16=None):
    """What a runtime writes for an output of the format: from the 8-bit frame, or -- a 10-bit format -- from the f16
    state (`state` given) or a 16-bit frame [H][W][3 or 4] of samples P (`frame16` given)."""
    if fmt in DEEP:
        if frame16 is not None:
            p = np.asarray(frame16)[..., :3].astype(np.int64)
        else:
            p = T.p_from_state(state) if state is not None else T.p_from_u8(frame)
        return to_words(fmt, *encode10(p, colorspace, SAMPLING[fmt]))
    return to_words(fmt, *encode(frame, colorspace, SAMPLING[fmt]))
