"""The output stage in numpy, in integers only (docs/output_stage.md is the prose): the upscaled frame scaled to the
output size by the source stage's triangle filter (source_reference.axis_table / _apply_axis, unchanged), on the 8-bit
frame or on the state's 16-bit samples, and the encode of a deep format from a 16-bit frame.  The HIP kernels
(scale_state_kernel in csrc/source_kernels.hip, Bgrx16Source in csrc/colour_kernels.hip) must give these bytes exactly.

8-bit frames are ``[H, W, 4]`` uint8 B, G, R, X; 16-bit frames ``[H, W, 4]`` uint16 B, G, R, X with X written 0."""

import numpy as np

import rgb_reference as G
import source_reference as S
import yuv10_reference as T
import yuv_sampled_reference as YS

AXIS_MIN, AXIS_MAX, RATIO_MAX = 2, 16384, 16
DEEP_YUV = YS.DEEP                                               # P010, I010, P210, I210, I410
DEEP_RGB = G.DEEP                                                # BGRX64, RGBP10, RGBP16, RGBPH, RGBPS, BGR96F
DEEP = tuple(DEEP_YUV) + tuple(DEEP_RGB)
NAMES = {**YS.FORMAT_NAMES, **G.FORMAT_NAMES}


def scale8(frame: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """The 8-bit path: the source stage's scaler on the 8-bit BGRX frame the runtime would have handed out."""
    return S.scale(frame, oh, ow)


def p_from_state(state) -> np.ndarray:
    """P = clamp(floor((s + 0.5) * 65536), 0, 65535) of B, G, R of the f16 state: ``[H, W, 3]`` int64."""
    return T.p_from_state(state)


def scale16(p: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """``p [H, W, 3 or 4]`` 16-bit samples (any integer dtype) -> ``[oh, ow, 4]`` uint16, X = 0:
    out = (sum over y, x of qy qx P + 2^23) >> 24 per channel.  The vertical sum is at most 65535 * 4096 < 2^28, the
    whole sum below 2^40 (both asserted); no rounding between the axes, no clipping."""
    h, w = p.shape[:2]
    x = np.asarray(p)[..., :3].astype(np.int64)
    assert int(x.min(initial=0)) >= 0 and int(x.max(initial=0)) <= 65535
    v = S._apply_axis(S.axis_table(h, oh), x)                                        # [oh, W, 3]
    assert int(v.max(initial=0)) < 1 << 28
    acc = S._apply_axis(S.axis_table(w, ow), v.transpose(1, 0, 2)).transpose(1, 0, 2) + (1 << 23)
    assert int(acc.max(initial=0)) < 1 << 40
    out = np.zeros((oh, ow, 4), np.uint16)
    out[..., :3] = acc >> 24                                                         # (at most 65535: rows sum to 4096)
    return out


def scale16_sums(p: np.ndarray, oh: int, ow: int):
    """(largest vertical sum, largest whole sum with its rounding constant) of scale16: what the two bounds are about."""
    h, w = p.shape[:2]
    v = S._apply_axis(S.axis_table(h, oh), np.asarray(p)[..., :3].astype(np.int64))
    acc = S._apply_axis(S.axis_table(w, ow), v.transpose(1, 0, 2)) + (1 << 23)
    return int(v.max()), int(acc.max())


def samples_from_p(kind: str, p) -> np.ndarray:
    """One channel's samples of an RGB format's kind (rgb_reference.KIND) from 16-bit samples P: W16 = P, W10 = P >> 6,
    the unit floats f32(P) / 65535 (one correctly rounded f32 division; "h": that as f16, to nearest even), BGR96F
    f32(P) / 257."""
    p = np.asarray(p).astype(np.uint32)
    assert kind != "u8" and int(p.max(initial=0)) <= 65535
    if kind == "w16":
        return p.astype(np.uint16)
    if kind == "w10":
        return (p >> 6).astype(np.uint16)
    f = p.astype(np.float32)                                                         # (exact: below 2^24)
    if kind == "f255":
        return (f / np.float32(257.0)).astype(np.float32)
    unit = (f / np.float32(65535.0)).astype(np.float32)
    return unit.astype(np.float16) if kind == "h" else unit


def encode16(fmt: int, cs: int, p: np.ndarray):
    """The planes of the deep format ``fmt`` encoded from the 16-bit frame ``p [H, W, 3 or 4]`` (B, G, R): the sample is
    P itself.  10-bit YUV: the encode from the state's P (yuv10_reference / yuv_sampled_reference encode10), unchanged."""
    if fmt in DEEP_YUV:
        return YS.to_words(fmt, *YS.encode10(np.asarray(p)[..., :3].astype(np.int64), cs, YS.SAMPLING[fmt]))
    if fmt in DEEP_RGB:
        return G.assemble(fmt, *(samples_from_p(G.KIND[fmt], np.asarray(p)[..., k]) for k in range(3)))
    raise ValueError(f"format {fmt} is not deep")


def encode8(fmt: int, cs: int, frame: np.ndarray):
    """The planes of any format but BGRX encoded from the 8-bit frame (deep formats: P = 257 u8), as without an output
    size."""
    if fmt in G.NEW_FORMATS:
        return G.encode_planes(fmt, frame=frame)
    return YS.encode_planes(fmt, cs, frame=frame)


def takes_16_bit_path(fmt: int, hbd_from_state: bool, masked: bool) -> bool:
    """A deep format takes the 16-bit path while the runtime encodes deep formats from its state and no mask is set."""
    return fmt in DEEP and hbd_from_state and not masked


def output(fmt: int, cs: int, oh: int, ow: int, frame: np.ndarray, state=None, hbd_from_state=True, masked=False):
    """What a runtime with the output size ``ow x oh`` writes for one frame: ``frame`` is the 8-bit frame it would have
    handed out (after the mask blend), ``state`` the f16 state [H, W, 4] that frame left.  BGRX (format 0): the frame."""
    if fmt == 0:
        return [scale8(frame, oh, ow)]
    if takes_16_bit_path(fmt, hbd_from_state, masked):
        return encode16(fmt, cs, scale16(p_from_state(state), oh, ow))
    return encode8(fmt, cs, scale8(frame, oh, ow))
