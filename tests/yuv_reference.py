"""Definition of the 8-bit 4:2:0 YUV <-> BGRX conversions of ju_process_frame (numpy, integer arithmetic).

The GPU kernels (csrc/colour_kernels.hip) compute exactly this, bit for bit; INTEGRATION.md states the formulas.

* Coefficients: K_r, K_b = (0.299, 0.114) for BT.601, (0.2126, 0.0722) for BT.709, K_g = 1 - K_r - K_b; every real
  coefficient k is used as round_half_away(k * 65536).
* Chroma siting (MPEG-2 / H.264 default): horizontally co-sited with the even luma columns, vertically centred between
  rows.  Decoding upsamples with the weights (3, 1) / 4 vertically and (2) or (1, 1) / 2 horizontally; encoding
  filters with [1, 2, 1] x [1, 1].  Every index is clamped to its plane.

Planes are numpy uint8 arrays: y [H][W], u and v [H/2][W/2]; NV12's interleaved plane is [H/2][W] (U, V, U, V ...).
"""

import math

import numpy as np

FMT_BGRX, FMT_I420, FMT_NV12 = 0, 1, 2
CS_BT601_LIMITED, CS_BT601_FULL, CS_BT709_LIMITED, CS_BT709_FULL = 0, 1, 2, 3
FORMAT_NAMES = {FMT_BGRX: "bgrx", FMT_I420: "i420", FMT_NV12: "nv12"}
COLORSPACE_NAMES = {CS_BT601_LIMITED: "601-limited", CS_BT601_FULL: "601-full",
                    CS_BT709_LIMITED: "709-limited", CS_BT709_FULL: "709-full"}


def round_half_away(x: float) -> int:
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def _params(cs):
    if cs not in COLORSPACE_NAMES:
        raise ValueError(f"unknown colour space {cs}")
    kr, kb = (0.299, 0.114) if cs in (CS_BT601_LIMITED, CS_BT601_FULL) else (0.2126, 0.0722)
    limited = cs in (CS_BT601_LIMITED, CS_BT709_LIMITED)
    return kr, kb, 1.0 - kr - kb, limited


def decode_coefficients(cs):
    """(kY, kRV, kBU, kGU, kGV) x 65536 and the luma offset oY."""
    kr, kb, kg, limited = _params(cs)
    s = 255.0 / 224.0 if limited else 1.0
    ky = 255.0 / 219.0 if limited else 1.0
    real = [ky, 2 * (1 - kr) * s, 2 * (1 - kb) * s, 2 * kb * (1 - kb) / kg * s, 2 * kr * (1 - kr) / kg * s]
    return tuple(round_half_away(k * 65536) for k in real), (16 if limited else 0)


def encode_coefficients(cs):
    """((cYR, cYG, cYB), (cUR, cUG, cUB), (cVR, cVG, cVB)) x 65536 and the luma offset oY."""
    kr, kb, kg, limited = _params(cs)
    sy, sc = (219.0 / 255.0, 224.0 / 255.0) if limited else (1.0, 1.0)
    y = (sy * kr, sy * kg, sy * kb)
    # U = (B - Yl) / (2 (1 - K_b)) * sc, V = (R - Yl) / (2 (1 - K_r)) * sc, Yl = K_r R + K_g G + K_b B
    du, dv = sc / (2 * (1 - kb)), sc / (2 * (1 - kr))
    u = (-kr * du, -kg * du, (1 - kb) * du)
    v = ((1 - kr) * dv, -kg * dv, -kb * dv)
    rnd = lambda t: tuple(round_half_away(k * 65536) for k in t)  # noqa: E731
    return (rnd(y), rnd(u), rnd(v)), (16 if limited else 0)


def _clamp8(x):
    return np.clip(x, 0, 255).astype(np.uint8)


def upsample8(c, h, w):
    """8 x the chroma plane c [H/2][W/2] at every luma position [H][W] (int64): 3 fractional bits."""
    c = c.astype(np.int64)
    ch, cw = c.shape
    y = np.arange(h)
    j = y >> 1
    jn = np.clip(np.where(y % 2 == 0, j - 1, j + 1), 0, ch - 1)
    cv = 3 * c[j] + c[jn]                                       # [H][W/2]
    x = np.arange(w)
    i = x >> 1
    i1 = np.minimum(i + 1, cw - 1)
    return np.where(x % 2 == 0, 2 * cv[:, i], cv[:, i] + cv[:, i1])


def decode(y, u, v, cs):
    """Y, U, V planes -> [H][W][4] uint8 BGRX (X = 0)."""
    (ky, krv, kbu, kgu, kgv), oy = decode_coefficients(cs)
    h, w = y.shape
    if h % 2 or w % 2 or u.shape != (h // 2, w // 2) or v.shape != (h // 2, w // 2):
        raise ValueError("4:2:0 planes need an even size and chroma planes of half the size")
    du = upsample8(u, h, w) - 1024
    dv = upsample8(v, h, w) - 1024
    yd = ky * 8 * (y.astype(np.int64) - oy)
    half = 1 << 18
    out = np.zeros((h, w, 4), np.uint8)
    out[..., 2] = _clamp8((yd + krv * dv + half) >> 19)
    out[..., 1] = _clamp8((yd - kgu * du - kgv * dv + half) >> 19)
    out[..., 0] = _clamp8((yd + kbu * du + half) >> 19)
    return out


def encode(bgrx, cs):
    """[H][W][4 (or 3)] uint8 BGR(X) -> (y, u, v) planes."""
    ((cyr, cyg, cyb), (cur, cug, cub), (cvr, cvg, cvb)), oy = encode_coefficients(cs)
    h, w = bgrx.shape[:2]
    if h % 2 or w % 2:
        raise ValueError("4:2:0 planes need an even size")
    b, g, r = (bgrx[..., k].astype(np.int64) for k in range(3))
    y = _clamp8(oy + ((cyr * r + cyg * g + cyb * b + (1 << 15)) >> 16))

    def sum8(p):                                                # [1, 2, 1] x [1, 1] over each 2x2 cell: 8 x C
        rows = p[0::2] + p[1::2]                                # [H/2][W]
        left = np.concatenate([rows[:, :1], rows[:, 1:-1:2]], axis=1)   # column 2i - 1, clamped to 0
        return left + 2 * rows[:, 0::2] + rows[:, 1::2]
    sr, sg, sb = sum8(r), sum8(g), sum8(b)
    half = 1 << 18
    u = _clamp8(128 + ((cur * sr + cug * sg + cub * sb + half) >> 19))
    v = _clamp8(128 + ((cvr * sr + cvg * sg + cvb * sb + half) >> 19))
    return y, u, v


def to_nv12(u, v):
    """Interleave U and V planes into NV12's chroma plane [H/2][W]."""
    uv = np.empty((u.shape[0], 2 * u.shape[1]), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return uv


def from_nv12(uv):
    return uv[:, 0::2], uv[:, 1::2]
