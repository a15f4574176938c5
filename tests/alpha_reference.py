"""The alpha channel in numpy, in integers only and without a tolerance anywhere (docs/alpha.md is the prose): what
``ju_set_alpha`` puts into the alpha slot of an output frame.  csrc/alpha_kernels.hip must give these codes exactly.

The slots: byte 3 of BGRX / RGBX (``"byte"``), word 3 of BGRX64 (``"word"``), the two top bits of X2RGB10 / X2BGR10
(``"bits"``); every other format has none (``"none"``).  The scale is the project's scaler on ONE channel of 16-bit
samples: the tables of source_reference / scale_filter_reference and the arithmetic of output_reference.scale16."""

import numpy as np

import output_reference as OUT
import scale_filter_reference as F
import source_reference as S

ZERO, OPAQUE, SOURCE = 0, 1, 2                                   # JU_ALPHA_*
KINDS = ("byte", "word", "bits", "none")                         # the hooks' kinds 0 .. 3
TOP = {"byte": 255, "word": 65535, "bits": 3}
AXIS_MIN, AXIS_MAX, RATIO_MAX = OUT.AXIS_MIN, OUT.AXIS_MAX, S.RATIO_MAX

# formats (JU_FMT_*) with a slot
FORMAT_KIND = {0: "byte", 34: "byte", 35: "word", 44: "bits", 45: "bits"}


def kind_of(fmt: int) -> str:
    return FORMAT_KIND.get(fmt, "none")


def plane(kind: str, codes, h: int = 0, w: int = 0) -> np.ndarray:
    """The 16-bit alpha plane A ``[H, W]`` int64 of an input frame's alpha codes: 257 a of a byte, the word itself,
    21845 a of a two-bit code; a format without a slot: 65535 everywhere (``codes`` unused, ``h x w`` given)."""
    if kind == "none":
        return np.full((h, w), 65535, np.int64)
    a = np.asarray(codes).astype(np.int64)
    assert a.ndim == 2 and int(a.min(initial=0)) >= 0 and int(a.max(initial=0)) <= TOP[kind]
    return a * {"byte": 257, "word": 1, "bits": 21845}[kind]


def sums(a: np.ndarray, oh: int, ow: int, filter: int):
    """(vertical sums [oh, W], whole sums with the rounding constant [oh, ow]) of the plane, int64, before the shift and
    the clamp."""
    v, acc = F.sums(np.repeat(np.asarray(a)[..., None], 3, axis=2), oh, ow, filter)
    return v[..., 0], acc[..., 0]


def scale(a: np.ndarray, oh: int, ow: int, filter: int) -> np.ndarray:
    """A' ``[oh, ow]`` int64: (sum qy qx A + 2^23) >> 24, clamped to 0 .. 65535 (a no-op for the triangle, whose rows of
    non-negative taps summing to 4096 cannot leave the range)."""
    a = np.asarray(a).astype(np.int64)
    assert a.ndim == 2 and int(a.min(initial=0)) >= 0 and int(a.max(initial=0)) <= 65535
    v, acc = sums(a, oh, ow, filter)
    assert int(np.abs(v).max(initial=0)) < 1 << 29 and int(np.abs(acc).max(initial=0)) < 1 << 42
    return np.clip(acc >> 24, 0, 65535)


def code(kind: str, a_scaled: np.ndarray) -> np.ndarray:
    """The slot's code of A': (A' + 128) / 257 of a byte, A' of a word, (A' + 10922) / 21845 of two bits."""
    a = np.asarray(a_scaled).astype(np.int64)
    if kind == "byte":
        return (a + 128) // 257
    if kind == "word":
        return a
    assert kind == "bits"
    return (a + 10922) // 21845


def alpha(mode: int, in_kind: str, codes, in_hw, out_kind: str, out_hw, filter: int = F.TRIANGLE):
    """The codes ``[OH, OW]`` of the output frame's slot, or ``None`` for an output format without one (nothing is
    launched for it).  in_hw / out_hw: (H, W) of the input and the output frame."""
    if out_kind == "none":
        return None
    oh, ow = out_hw
    if mode == ZERO:
        return np.zeros((oh, ow), np.int64)
    if mode == OPAQUE:
        return np.full((oh, ow), TOP[out_kind], np.int64)
    assert mode == SOURCE
    return code(out_kind, scale(plane(in_kind, codes, *in_hw), oh, ow, filter))


def checkerboard(h: int, w: int) -> np.ndarray:
    """0 and 65535 alternating, pixel by pixel: the plane whose cubic sums leave 0 .. 65535 at both ends."""
    y, x = np.mgrid[0:h, 0:w]
    return ((y + x) % 2).astype(np.int64) * 65535


def problem(mode: int, filter: int, in_w: int, in_h: int, out_w: int, out_h: int) -> bool:
    """Whether ju_set_alpha and the two size setters refuse these frame sizes (the limits alone; the message is
    runtime.alpha_problem's)."""
    if mode not in (ZERO, OPAQUE, SOURCE) or filter not in F.FILTERS:
        return True
    if mode != SOURCE:
        return False
    down = F.down_max(filter)

    def ok(n, m):
        return AXIS_MIN <= n <= AXIS_MAX and AXIS_MIN <= m <= AXIS_MAX and n <= down * m and m <= RATIO_MAX * n
    return not (ok(in_w, out_w) and ok(in_h, out_h))
