"""The filters of the source and the output scaler in numpy, in integers only (docs/source_stage.md "Filters" is the
prose): the triangle of source_reference.py, unchanged, and the two cubic filters whose weights are polynomials and so
exact in 64-bit integers -- Catmull-Rom (Pillow's BICUBIC, a = -0.5) and Mitchell-Netravali (B = C = 1/3).  The C++
table builder (buildScaleAxis) and the signed forms of the HIP kernels (csrc/source_kernels.hip) must give these words
and bytes exactly.

8-bit frames are ``[H, W, 4]`` uint8 B, G, R, X; 16-bit samples ``[H, W, 3 or 4]`` of any integer type; X is written 0."""

import functools

import numpy as np

import source_reference as S

TRIANGLE, CATMULL_ROM, MITCHELL = 0, 2, 3
FILTERS = (TRIANGLE, CATMULL_ROM, MITCHELL)
CUBIC = (CATMULL_ROM, MITCHELL)
NAMES = {TRIANGLE: "triangle", CATMULL_ROM: "catmull-rom", MITCHELL: "mitchell"}
MAX_TAPS = S.MAX_TAPS
RATIO_MAX = S.RATIO_MAX                # enlarging, and reducing with the triangle
CUBIC_DOWN_MAX = 8                     # reducing with a cubic filter: twice the support, half the factor
ABS_SUM_MAX = 6144                     # the largest sum |q| of a row a table may hold: what the kernels' widths rest on


def down_max(filter: int) -> int:
    return RATIO_MAX if filter == TRIANGLE else CUBIC_DOWN_MAX


def raw_weight(filter: int, u: np.ndarray, big: int) -> np.ndarray:
    """The integer weight at distance u / D (``big`` = D; int64, u >= 0): the kernel times 2 D^3 (Catmull-Rom) or
    18 D^3 (Mitchell), 0 from 2 D on.  With D <= 32768 every term stays below 2^53."""
    u = np.minimum(u.astype(np.int64), 2 * big)                  # (both outer pieces are 0 at 2 D)
    d = np.int64(big)
    if filter == CATMULL_ROM:
        inner = 3 * u ** 3 - 5 * u ** 2 * d + 2 * d ** 3
        outer = -u ** 3 + 5 * u ** 2 * d - 8 * u * d ** 2 + 4 * d ** 3
    elif filter == MITCHELL:
        inner = 21 * u ** 3 - 36 * u ** 2 * d + 16 * d ** 3
        outer = -7 * u ** 3 + 36 * u ** 2 * d - 60 * u * d ** 2 + 32 * d ** 3
    else:
        raise ValueError(f"filter {filter} is not cubic")
    return np.where(u < d, inner, outer)


@functools.lru_cache(maxsize=None)
def axis_table(n: int, m: int, filter: int = TRIANGLE):
    """One axis, ``n`` source samples -> ``m`` destination samples: ``(start [m], count [m], taps [m, MAX_TAPS])``, taps
    signed.  Filter 0 is source_reference.axis_table.  A cubic row: the run of s in [0, n) with u = |(2s+1) m - (2d+1) n|
    < 2 D, D = 2 max(n, m), zero weights trimmed at both ends (never inside); q = floor(4096 w / S) toward minus infinity,
    S the row's sum (asserted positive); the remainder 4096 - sum(q) goes to the largest w, the first on a tie."""
    if filter == TRIANGLE:
        return S.axis_table(n, m)
    assert n >= 1 and m >= 1 and n <= CUBIC_DOWN_MAX * m and m <= RATIO_MAX * n, (n, m)
    big = 2 * max(n, m)
    assert big <= 32768
    start = np.zeros(m, np.int64)
    count = np.zeros(m, np.int64)
    taps = np.zeros((m, MAX_TAPS), np.int64)
    for d in range(m):
        c = (2 * d + 1) * n
        lo = max(0, (c - 2 * big) // (2 * m) - 1)
        hi = min(n, (c + 2 * big) // (2 * m) + 2)
        s = np.arange(lo, hi, dtype=np.int64)
        u = np.abs((2 * s + 1) * m - c)
        w = np.where(u < 2 * big, raw_weight(filter, u, big), 0)
        nz = np.flatnonzero(w)
        a, b = int(nz[0]), int(nz[-1]) + 1                        # (a zero inside the run stays a tap: one run)
        assert (u[a:b] < 2 * big).all() and b - a <= MAX_TAPS
        w = w[a:b]
        total = int(w.sum())
        assert total > 0 and int(np.abs(w).max()) * 4096 < 1 << 62
        q = w * 4096 // total                                     # (numpy's // floors, also below zero)
        q[int(np.argmax(w))] += 4096 - int(q.sum())
        assert int(np.abs(q).sum()) <= ABS_SUM_MAX
        start[d], count[d] = lo + a, b - a
        taps[d, :b - a] = q
    for t in (start, count, taps):
        t.setflags(write=False)
    return start, count, taps


def abs_sum(table) -> int:
    """A of a table: the largest sum |q| over its rows."""
    return int(np.abs(table[2]).sum(1).max())


def sums(samples: np.ndarray, oh: int, ow: int, filter: int):
    """(vertical sums [oh, W, 3], whole sums with the rounding constant [oh, ow, 3]) of ``samples [H, W, >= 3]``, int64,
    before the shift and the clamp."""
    h, w = samples.shape[:2]
    x = np.asarray(samples)[..., :3].astype(np.int64)
    v = S._apply_axis(axis_table(h, oh, filter), x)
    acc = S._apply_axis(axis_table(w, ow, filter), v.transpose(1, 0, 2)).transpose(1, 0, 2) + (1 << 23)
    return v, acc


def _scale(samples, oh, ow, filter, top, vbits, bits, dtype):
    assert int(samples.min(initial=0)) >= 0 and int(samples.max(initial=0)) <= top
    v, acc = sums(samples, oh, ow, filter)
    assert int(np.abs(v).max(initial=0)) < 1 << vbits             # |vertical sum| <= top * 6144
    assert int(np.abs(acc).max(initial=0)) < 1 << bits            # |whole sum| <= top * 6144^2 + 2^23
    out = np.zeros((oh, ow, 4), dtype)
    out[..., :3] = np.clip(acc >> 24, 0, top)                     # (>> on int64: arithmetic, i.e. floor)
    return out


def scale8(src: np.ndarray, oh: int, ow: int, filter: int) -> np.ndarray:
    """``src [H, W, 4]`` uint8 -> ``[oh, ow, 4]`` uint8: out = clamp((sum qy qx src + 2^23) >> 24, 0, 255), X = 0.
    |vertical sum| < 2^21 and |whole sum| < 2^34 (asserted); nothing is rounded or clipped between the axes."""
    assert src.dtype == np.uint8
    return _scale(src, oh, ow, filter, 255, 21, 34, np.uint8)


def scale16(p: np.ndarray, oh: int, ow: int, filter: int) -> np.ndarray:
    """``p [H, W, 3 or 4]`` 16-bit samples (P of docs/output_stage.md) -> ``[oh, ow, 4]`` uint16: out = clamp((sum qy qx P +
    2^23) >> 24, 0, 65535), X = 0.  |vertical sum| < 2^29 and |whole sum| < 2^42 (asserted)."""
    return _scale(np.asarray(p), oh, ow, filter, 65535, 29, 42, np.uint16)


def kernel_float(filter: int, x: np.ndarray) -> np.ndarray:
    """The filter's kernel at |x| in float64 (x >= 0)."""
    if filter == TRIANGLE:
        return np.maximum(0.0, 1.0 - x)
    if filter == CATMULL_ROM:
        inner, outer = (1.5 * x - 2.5) * x * x + 1.0, ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0
    else:
        inner, outer = ((21.0 * x - 36.0) * x * x + 16.0) / 18.0, (((-7.0 * x + 36.0) * x - 60.0) * x + 32.0) / 18.0
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def matrix_float(n: int, m: int, filter: int) -> np.ndarray:
    """The axis as a float64 matrix [m, n] with its coefficients unquantised, rows normalised to sum 1."""
    big = 2 * max(n, m)
    s, d = np.arange(n, dtype=np.int64)[None, :], np.arange(m, dtype=np.int64)[:, None]
    wgt = kernel_float(filter, np.abs((2 * s + 1) * m - (2 * d + 1) * n).astype(np.float64) / big)
    return wgt / wgt.sum(1, keepdims=True)


def scale_float(samples: np.ndarray, oh: int, ow: int, filter: int, top: int) -> np.ndarray:
    """The same filter unquantised, in float64, not rounded, clamped to [0, top]: ``[oh, ow, 3]``."""
    h, w = samples.shape[:2]
    x = np.asarray(samples)[..., :3].astype(np.float64)
    out = np.einsum("dh,hwc,ew->dec", matrix_float(h, oh, filter), x, matrix_float(w, ow, filter), optimize=True)
    return np.clip(out, 0.0, float(top))


def float_bound(src_hw, dst_hw, filter: int, top: int) -> float:
    """The most |integer result - scale_float| can be (docs/source_stage.md "Filters"): per axis the quantisation moves a
    row's result by at most (T - 1) R / 4096, T the row's taps and R the spread of what it filters; the vertical axis
    filters samples (R = top), the horizontal axis filters exact vertical results (R <= top B_y, B_y the largest sum |c|
    of the unquantised vertical rows) and multiplies the vertical axis' error by A_x / 4096; then 0.5 for the rounding.
    The clamp moves two values no further apart."""
    ty, tx = (int(axis_table(n, m, filter)[1].max()) for n, m in zip(src_hw, dst_hw))
    ax = abs_sum(axis_table(src_hw[1], dst_hw[1], filter))
    by = float(np.abs(matrix_float(src_hw[0], dst_hw[0], filter)).sum(1).max())
    return 0.5 + top * ((ax / 4096.0) * (ty - 1) + by * (tx - 1)) / 4096.0


def step_edges(h: int, w: int, top: int = 255, dtype=np.uint8) -> np.ndarray:
    """Columns and rows of 0 / top in runs of three: edges in both directions, which a cubic filter overshoots."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 4), dtype)
    img[..., 0] = np.where((x // 3) % 2 == 0, 0, top)
    img[..., 1] = np.where((y // 3) % 2 == 0, top, 0)
    img[..., 2] = np.where(((x // 3) + (y // 3)) % 2 == 0, 0, top)
    return img
