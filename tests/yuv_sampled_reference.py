"""Definition of the YUV <-> BGRX conversions of ju_process_frame for every chroma sampling (numpy, integers only):
4:2:0 as tests/yuv_reference.py and tests/yuv10_reference.py define it, and 4:2:2 / 4:4:4, 8- and 10-bit.

Coefficients, rounding, colour spaces, ranges, the luma formulas, the sample P and `upsample8` are IMPORTED from those two
files; only the chroma resampling is stated here.  The GPU kernels (csrc/colour_kernels.hip, "4:2:2 and 4:4:4") compute
exactly this, bit for bit; INTEGRATION.md states the formulas.

* Siting of 4:2:2: co-sited horizontally with the even luma columns, as in the 4:2:0 definition; every luma row has its
  own chroma row.  4:4:4: a chroma sample per pixel.
* Decode, C8(y, x) = 8 x chroma at luma position (y, x): 4:2:0 `upsample8`; 4:2:2 8 c[y][i] at x = 2i and
  4 (c[y][i] + c[y][min(i + 1, W/2 - 1)]) at x = 2i + 1; 4:4:4 8 c[y][x].
* Encode, the chroma sum S of weight 2^k: 4:2:0 [1, 2, 1] x [1, 1], k = 3; 4:2:2 p[y][max(2i - 1, 0)] + 2 p[y][2i] +
  p[y][2i + 1], k = 2; 4:4:4 the pixel, k = 0.  8-bit C = clamp(128 + ((c . S + 2^(15 + k)) >> (16 + k))), 10-bit
  C = clamp(512 + ((c . S + 2^(31 + k)) >> (32 + k)), 0, 1023).

Samples are numpy arrays y [H][W] and u, v [H/2][W/2] (420), [H][W/2] (422) or [H][W] (444): uint8, or uint16 holding
0..1023.  `to_words` / `from_words` convert between them and the planes a caller holds in each JU_FMT_* format.
"""

import numpy as np

import yuv10_reference as T
import yuv_reference as Y

FMT_I420, FMT_NV12, FMT_P010, FMT_I010 = 1, 2, 3, 4
FMT_YUY2, FMT_UYVY, FMT_I422, FMT_P210, FMT_I210, FMT_I444, FMT_I410 = 16, 17, 18, 19, 20, 24, 25
NEW_FORMATS = (FMT_YUY2, FMT_UYVY, FMT_I422, FMT_P210, FMT_I210, FMT_I444, FMT_I410)
FORMAT_NAMES = {FMT_I420: "i420", FMT_NV12: "nv12", FMT_P010: "p010", FMT_I010: "i010", FMT_YUY2: "yuy2",
                FMT_UYVY: "uyvy", FMT_I422: "i422", FMT_P210: "p210", FMT_I210: "i210", FMT_I444: "i444", FMT_I410: "i410"}
SAMPLING = {FMT_I420: 420, FMT_NV12: 420, FMT_P010: 420, FMT_I010: 420, FMT_YUY2: 422, FMT_UYVY: 422, FMT_I422: 422,
            FMT_P210: 422, FMT_I210: 422, FMT_I444: 444, FMT_I410: 444}
DEEP = (FMT_P010, FMT_I010, FMT_P210, FMT_I210, FMT_I410)
WEIGHT_LOG2 = {420: 3, 422: 2, 444: 0}


def chroma_shape(sampling, h, w):
    if sampling == 420:
        if h % 2 or w % 2:
            raise ValueError("4:2:0 planes need an even size")
        return h // 2, w // 2
    if sampling == 422:
        if w % 2:
            raise ValueError("4:2:2 planes need an even width")
        return h, w // 2
    if sampling == 444:
        return h, w
    raise ValueError(f"unknown sampling {sampling}")


def upsample8_sampled(c, sampling, h, w):
    """C8: 8 x the chroma plane c at every luma position [H][W] (int64)."""
    if c.shape != chroma_shape(sampling, h, w):
        raise ValueError("chroma plane of the wrong shape")
    if sampling == 420:
        return Y.upsample8(c, h, w)
    c = c.astype(np.int64)
    if sampling == 444:
        return 8 * c
    x = np.arange(w)
    i = x >> 1
    i1 = np.minimum(i + 1, w // 2 - 1)
    return np.where(x % 2 == 0, 8 * c[:, i], 4 * (c[:, i] + c[:, i1]))


def decode(y, u, v, cs, sampling, deep=False):
    """Y, U, V samples (uint8, or 10-bit values in uint16 where `deep`) -> [H][W][4] uint8 BGRX (X = 0)."""
    (ky, krv, kbu, kgu, kgv), oy = T.decode10_coefficients(cs) if deep else Y.decode_coefficients(cs)
    h, w = y.shape
    mid = 8 * (512 if deep else 128)
    du = upsample8_sampled(u, sampling, h, w) - mid
    dv = upsample8_sampled(v, sampling, h, w) - mid
    yd = ky * 8 * (y.astype(np.int64) - oy)
    half = 1 << 18
    out = np.zeros((h, w, 4), np.uint8)
    out[..., 2] = np.clip((yd + krv * dv + half) >> 19, 0, 255)
    out[..., 1] = np.clip((yd - kgu * du - kgv * dv + half) >> 19, 0, 255)
    out[..., 0] = np.clip((yd + kbu * du + half) >> 19, 0, 255)
    return out


def chroma_sum(p, sampling):
    """S of one channel p [H][W] (int64): the sum of weight 2^WEIGHT_LOG2[sampling] per chroma sample."""
    chroma_shape(sampling, *p.shape)
    if sampling == 444:
        return p
    rows = p[0::2] + p[1::2] if sampling == 420 else p
    left = np.concatenate([rows[:, :1], rows[:, 1:-1:2]], axis=1)       # column 2i - 1, clamped to 0
    return left + 2 * rows[:, 0::2] + rows[:, 1::2]


def encode(bgrx, cs, sampling):
    """[H][W][4 (or 3)] uint8 BGR(X) -> (y, u, v) uint8 samples."""
    ((cyr, cyg, cyb), cu, cv), oy = Y.encode_coefficients(cs)
    b, g, r = (bgrx[..., k].astype(np.int64) for k in range(3))
    y = np.clip(oy + ((cyr * r + cyg * g + cyb * b + (1 << 15)) >> 16), 0, 255).astype(np.uint8)
    k = WEIGHT_LOG2[sampling]
    sr, sg, sb = (chroma_sum(c, sampling) for c in (r, g, b))

    def chroma(c):
        return np.clip(128 + ((c[0] * sr + c[1] * sg + c[2] * sb + (1 << (15 + k))) >> (16 + k)), 0, 255).astype(np.uint8)
    return y, chroma(cu), chroma(cv)


def encode10(p, cs, sampling):
    """[H][W][3 (or 4)] 16-bit samples P (B, G, R; T.p_from_state / T.p_from_u8) -> (y, u, v) uint16 samples 0..1023."""
    ((cyr, cyg, cyb), cu, cv), oy = T.encode10_coefficients(cs)
    b, g, r = (p[..., k].astype(np.int64) for k in range(3))
    y = np.clip(oy + ((cyr * r + cyg * g + cyb * b + (1 << 31)) >> 32), 0, 1023).astype(np.uint16)
    k = WEIGHT_LOG2[sampling]
    sr, sg, sb = (chroma_sum(c, sampling) for c in (r, g, b))

    def chroma(c):
        return np.clip(512 + ((c[0] * sr + c[1] * sg + c[2] * sb + (1 << (31 + k))) >> (32 + k)), 0, 1023).astype(np.uint16)
    return y, chroma(cu), chroma(cv)


# ---- the planes a caller holds ------------------------------------------------------------------------------------------
def to_yuy2(y, u, v):
    """8-bit 4:2:2 samples -> one plane [H][2W]: Y0 U Y1 V per pixel pair."""
    out = np.empty((y.shape[0], 2 * y.shape[1]), np.uint8)
    out[:, 0::4], out[:, 1::4], out[:, 2::4], out[:, 3::4] = y[:, 0::2], u, y[:, 1::2], v
    return out


def from_yuy2(plane):
    y = np.empty((plane.shape[0], plane.shape[1] // 2), np.uint8)
    y[:, 0::2], y[:, 1::2] = plane[:, 0::4], plane[:, 2::4]
    return y, plane[:, 1::4], plane[:, 3::4]


def to_uyvy(y, u, v):
    """8-bit 4:2:2 samples -> one plane [H][2W]: U Y0 V Y1 per pixel pair."""
    out = np.empty((y.shape[0], 2 * y.shape[1]), np.uint8)
    out[:, 0::4], out[:, 1::4], out[:, 2::4], out[:, 3::4] = u, y[:, 0::2], v, y[:, 1::2]
    return out


def from_uyvy(plane):
    y = np.empty((plane.shape[0], plane.shape[1] // 2), np.uint8)
    y[:, 0::2], y[:, 1::2] = plane[:, 1::4], plane[:, 3::4]
    return y, plane[:, 0::4], plane[:, 2::4]


def to_words(fmt, y, u, v):
    """The planes a caller holds of the samples, as a list (one, two or three arrays)."""
    if fmt == FMT_I420 or fmt == FMT_I422 or fmt == FMT_I444:
        return [y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)]
    if fmt == FMT_NV12:
        return [y.astype(np.uint8), Y.to_nv12(u, v)]
    if fmt == FMT_YUY2:
        return [to_yuy2(y, u, v)]
    if fmt == FMT_UYVY:
        return [to_uyvy(y, u, v)]
    if fmt in (FMT_P010, FMT_P210):                              # value << 6, interleaved UV (T.to_p010 is shape-agnostic)
        return list(T.to_p010(y, u, v))
    if fmt in (FMT_I010, FMT_I210, FMT_I410):                    # the value in the low bits
        return list(T.to_i010(y, u, v))
    raise ValueError(f"unknown format {fmt}")


def from_words(fmt, planes):
    """A caller's planes -> (y, u, v) samples; bits the format ignores are ignored."""
    if fmt in (FMT_I420, FMT_I422, FMT_I444):
        return tuple(planes)
    if fmt == FMT_NV12:
        return (planes[0],) + tuple(Y.from_nv12(planes[1]))
    if fmt == FMT_YUY2:
        return from_yuy2(planes[0])
    if fmt == FMT_UYVY:
        return from_uyvy(planes[0])
    if fmt in (FMT_P010, FMT_P210):
        return T.from_p010(*planes)
    if fmt in (FMT_I010, FMT_I210, FMT_I410):
        return T.from_i010(*planes)
    raise ValueError(f"unknown format {fmt}")


def blank_planes(fmt, h, w):
    """Zeroed planes of a frame of the format (what to_words gives of zero samples)."""
    dt = np.uint16 if fmt in DEEP else np.uint8
    ch, cw = chroma_shape(SAMPLING[fmt], h, w)
    return to_words(fmt, np.zeros((h, w), dt), np.zeros((ch, cw), dt), np.zeros((ch, cw), dt))


def decode_planes(fmt, cs, planes):
    """The BGRX frame the network consumes for a caller's planes."""
    return decode(*from_words(fmt, planes), cs, SAMPLING[fmt], fmt in DEEP)


def encode_planes(fmt, cs, frame=None, state=None):
    """What a runtime writes for an output of the format: from the 8-bit frame, or -- a 10-bit format with the f16 state
    given -- from the state."""
    if fmt in DEEP:
        p = T.p_from_state(state) if state is not None else T.p_from_u8(frame)
        return to_words(fmt, *encode10(p, cs, SAMPLING[fmt]))
    return to_words(fmt, *encode(frame, cs, SAMPLING[fmt]))
