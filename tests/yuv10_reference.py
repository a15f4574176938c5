"""Definition of the 10-bit 4:2:0 YUV (P010 / I010) <-> BGRX conversions of ju_process_frame (numpy, integers only).

The GPU kernels (csrc/colour_kernels.hip) compute exactly this, bit for bit; INTEGRATION.md states the formulas.
Siting, the (3, 1) / 4 x (2 | 1, 1) / 2 chroma upsampling, the [1, 2, 1] x [1, 1] downsampling and the index clamping are
those of the 8-bit definition (tests/yuv_reference.py); K_r, K_b and the four colour spaces too.

* Samples are 10-bit values 0..1023 in uint16 arrays: y [H][W], u and v [H/2][W/2].  `to_p010` / `to_i010` make the
  16-bit words a caller's planes hold of them (P010: value << 6, interleaved UV; I010: the value in the low bits),
  `from_p010` / `from_i010` read them back ignoring the bits the format ignores.
* Ranges: limited Y = 64 + 876 Y', C = 512 + 896 C'; full Y = 1023 Y', C = 512 + 1023 C'.
* decode10: 10-bit planes -> the u8 BGRX frame the network consumes (32-bit accumulators suffice).
* encode10: a 16-bit sample P (0..65535) per channel -> 10-bit planes (64-bit accumulators).  P comes from the
  engine's f16 state (`p_from_state`: floor((s + 0.5) * 65536), saturated) or from the u8 frame (`p_from_u8`: 257 u8).
"""

import numpy as np

from yuv_reference import _params, round_half_away, upsample8

FMT_P010, FMT_I010 = 3, 4


def decode10_coefficients(cs):
    """(kY, kRV, kBU, kGU, kGV) x 65536 for 10-bit samples -> 8-bit RGB, and the luma offset oY."""
    kr, kb, kg, limited = _params(cs)
    s = 255.0 / 896.0 if limited else 255.0 / 1023.0
    ky = 255.0 / 876.0 if limited else 255.0 / 1023.0
    real = [ky, 2 * (1 - kr) * s, 2 * (1 - kb) * s, 2 * kb * (1 - kb) / kg * s, 2 * kr * (1 - kr) / kg * s]
    return tuple(round_half_away(k * 65536) for k in real), (64 if limited else 0)


def encode10_real(cs):
    """The nine real coefficients (rows Y, U, V; columns R, G, B) that take P / 65535 to 10-bit codes, and oY."""
    kr, kb, kg, limited = _params(cs)
    sy, sc = (876.0, 896.0) if limited else (1023.0, 1023.0)
    du, dv = sc / (2 * (1 - kb)), sc / (2 * (1 - kr))
    y = (sy * kr, sy * kg, sy * kb)
    u = (-kr * du, -kg * du, (1 - kb) * du)
    v = ((1 - kr) * dv, -kg * dv, -kb * dv)
    return (y, u, v), (64 if limited else 0)


def encode10_coefficients(cs):
    """round_half_away(k / 65535 * 2^32) for each of the nine coefficients, and oY."""
    real, oy = encode10_real(cs)
    return tuple(tuple(round_half_away(k / 65535.0 * 4294967296.0) for k in row) for row in real), oy


def decode10_terms(y, u, v, cs):
    """The three accumulators (R, G, B) of decode10 before the shift, int64 [H][W] each."""
    (ky, krv, kbu, kgu, kgv), oy = decode10_coefficients(cs)
    h, w = y.shape
    if h % 2 or w % 2 or u.shape != (h // 2, w // 2) or v.shape != (h // 2, w // 2):
        raise ValueError("4:2:0 planes need an even size and chroma planes of half the size")
    du = upsample8(u, h, w) - 8 * 512
    dv = upsample8(v, h, w) - 8 * 512
    yd = ky * 8 * (y.astype(np.int64) - oy)
    half = 1 << 18
    return yd + krv * dv + half, yd - kgu * du - kgv * dv + half, yd + kbu * du + half


def decode10(y, u, v, cs):
    """10-bit Y, U, V planes (uint16, 0..1023) -> [H][W][4] uint8 BGRX (X = 0)."""
    r, g, b = decode10_terms(y, u, v, cs)
    out = np.zeros(y.shape + (4,), np.uint8)
    out[..., 2] = np.clip(r >> 19, 0, 255)
    out[..., 1] = np.clip(g >> 19, 0, 255)
    out[..., 0] = np.clip(b >> 19, 0, 255)
    return out


def p_from_u8(bgrx):
    """The 16-bit samples of a u8 frame: 257 u8 (0 -> 0, 255 -> 65535)."""
    return bgrx[..., :3].astype(np.int64) * 257


def p_from_state(state):
    """The 16-bit samples of the f16 state (output_raw in -0.5 .. 0.5): floor((s + 0.5) * 65536), saturated to
    0..65535.  Every finite f16 of magnitude up to 0.5 is an integer multiple of 2^-24, so this is integer
    arithmetic: ((s * 2^24) + 2^23) >> 8.  `state`: a float16 array (or float32 holding f16 values), last axis >= 3."""
    s = np.asarray(state)[..., :3].astype(np.float64)
    m = np.clip(s, -1.0, 1.0) * 16777216.0                      # (beyond +-0.5 the result saturates anyway)
    mi = np.floor(m).astype(np.int64)                           # exact for |s| <= 0.5; floor beyond keeps the order
    return np.clip((mi + (1 << 23)) >> 8, 0, 65535)


def encode10(p, cs):
    """[H][W][3 (or 4)] 16-bit samples P (B, G, R; any integer dtype, 0..65535) -> (y, u, v) uint16 planes, 0..1023."""
    ((cyr, cyg, cyb), (cur, cug, cub), (cvr, cvg, cvb)), oy = encode10_coefficients(cs)
    h, w = p.shape[:2]
    if h % 2 or w % 2:
        raise ValueError("4:2:0 planes need an even size")
    b, g, r = (p[..., k].astype(np.int64) for k in range(3))
    y = np.clip(oy + ((cyr * r + cyg * g + cyb * b + (1 << 31)) >> 32), 0, 1023).astype(np.uint16)

    def sum8(c):                                                # [1, 2, 1] x [1, 1] over each 2x2 cell: 8 x C
        rows = c[0::2] + c[1::2]
        left = np.concatenate([rows[:, :1], rows[:, 1:-1:2]], axis=1)
        return left + 2 * rows[:, 0::2] + rows[:, 1::2]
    sr, sg, sb = sum8(r), sum8(g), sum8(b)
    half = 1 << 34
    u = np.clip(512 + ((cur * sr + cug * sg + cub * sb + half) >> 35), 0, 1023).astype(np.uint16)
    v = np.clip(512 + ((cvr * sr + cvg * sg + cvb * sb + half) >> 35), 0, 1023).astype(np.uint16)
    return y, u, v


def to_p010(y, u, v):
    """10-bit planes -> P010 words: (y [H][W], uv [H/2][W]) uint16, value << 6, U first."""
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint16)
    uv[:, 0::2], uv[:, 1::2] = u.astype(np.uint16) << 6, v.astype(np.uint16) << 6
    return y.astype(np.uint16) << 6, uv


def from_p010(yw, uvw):
    """P010 words -> 10-bit planes (the low 6 bits are ignored)."""
    return yw >> 6, uvw[:, 0::2] >> 6, uvw[:, 1::2] >> 6


def to_i010(y, u, v):
    return y.astype(np.uint16), u.astype(np.uint16), v.astype(np.uint16)


def from_i010(yw, uw, vw):
    """I010 words -> 10-bit planes (the upper 6 bits are ignored)."""
    return yw & 0x3ff, uw & 0x3ff, vw & 0x3ff


def to_words(fmt, y, u, v):
    """The planes a caller holds of 10-bit samples, as a list: P010 [y, uv], I010 [y, u, v]."""
    return list(to_p010(y, u, v)) if fmt == FMT_P010 else list(to_i010(y, u, v))


def from_words(fmt, planes):
    return from_p010(*planes) if fmt == FMT_P010 else from_i010(*planes)
