"""Exact definitions of the network's compute kernels on DYADIC inputs (docs/exact_tests.md), numpy only.

A launch is dyadic when every activation, weight and bias is a multiple of one power of two, every activation is a value
of the 16-bit type T, and for every output A = sum |x w| + |bias| + |residual| is below 2^20 quanta of the products.  Every
product and every partial sum is then exact in f32 in any order, fused or not; what a kernel converts is the exact result,
and its output is ONE round-to-nearest-even of it.  Every function here computes that result in float64 (exact: the sums
stay far below 2^53 quanta), checks the condition and raises NotDyadic where it does not hold, and returns the words a
correct kernel stores.  Tensors kept in T inside a kernel (the x2 expansion, conv A's tile) are rounded at the same place.

Values travel as float64 arrays; `rne` turns them into the 16-bit words and `to_float` back."""

import numpy as np

F16, BF16 = 0, 1                       # runtime.DTYPE_F16 / DTYPE_BF16
BUDGET_BITS = 20                       # A / q' < 2^20: 4 bits under f32's significand
F16_MAX = 65504.0


class NotDyadic(ValueError):
    pass


# ---- rounding ---------------------------------------------------------------------------------------------------------------
def rne(values, dtype):
    """float64 values that f32 holds exactly -> the words of ONE round to nearest even to f16 / bf16 (uint16)."""
    v = np.asarray(values, np.float64)
    f = v.astype(np.float32)
    if not np.array_equal(f.astype(np.float64), v):
        raise NotDyadic("a value f32 does not hold exactly")
    if dtype == F16:
        if v.size and np.abs(v).max() > F16_MAX:
            raise NotDyadic("an f16 output beyond 65504")
        return v.astype(np.float16).view(np.uint16)
    b = f.view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def rne_any(values, dtype):
    """The same rounding of ANY float64 (normal range), without the detour over f32."""
    v = np.asarray(values, np.float64)
    if dtype == F16:
        return v.astype(np.float16).view(np.uint16)
    _, e = np.frexp(v)
    q = np.ldexp(1.0, e - 8)                                  # spacing of bf16 in v's binade: 8 significant bits
    return rne(np.round(v / q) * q, BF16)                     # (np.round: half to even; v / q is exact)


def to_float(words, dtype):
    w = np.asarray(words, np.uint16)
    if dtype == F16:
        return w.view(np.float16).astype(np.float64)
    return (w.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def in_type(values, dtype):
    v = np.asarray(values, np.float64)
    return np.array_equal(to_float(rne_any(v, dtype), dtype), v)


def fold_zero(words):
    """0x8000 -> 0x0000 (the comparison does not tell the zeros apart); returns (words, how many were mapped)."""
    w = np.asarray(words, np.uint16).copy()
    neg = w == 0x8000
    w[neg] = 0
    return w, int(neg.sum())


def rounding_counts(exact, dtype):
    """(outputs the final rounding changed, exact ties among them)."""
    v = np.asarray(exact, np.float64).ravel()
    w = rne(v, dtype)
    r = to_float(w, dtype)
    d = np.abs(v - r)
    changed = d != 0
    toward = np.where(np.abs(v) > np.abs(r), w + 1, w - 1).astype(np.uint16)      # the neighbour on v's other side
    ties = changed & (np.abs(v - to_float(toward, dtype)) == d)
    return int(changed.sum()), int(ties.sum())


# ---- the dyadic condition ---------------------------------------------------------------------------------------------------
def quantum(*arrays):
    """The largest 2^-k (k = 0 .. 30) every value is a multiple of."""
    for k in range(31):
        s = float(2 ** k)
        if all(np.array_equal(np.round(np.asarray(a, np.float64) * s), np.asarray(a, np.float64) * s) for a in arrays):
            return 1.0 / s
    raise NotDyadic("no common quantum down to 2^-30")


def check_budget(a_max, q, what):
    bits = float(np.log2(max(a_max / q, 1.0)))
    if not a_max / q < 2.0 ** BUDGET_BITS:
        raise NotDyadic("%s: A / q' = 2^%.2f, not below 2^%d" % (what, bits, BUDGET_BITS))
    return bits


# ---- resampling -------------------------------------------------------------------------------------------------------------
def upsample2_exact(x, clamp=True):
    """TF1 asymmetric bilinear x2 before rounding: source = destination / 2, the neighbour clamped to the last row / column."""
    x = np.asarray(x, np.float64)
    h, w, _ = x.shape

    def axis(n):
        d = np.arange(2 * n)
        lo = d // 2
        hi = np.minimum(lo + 1, n - 1) if clamp else lo + 1
        return lo, hi, (d % 2) * 0.5

    y0, y1, fy = axis(h)
    x0, x1, fx = axis(w)
    if not clamp:                                             # (a fault for the tests of the tests: zeros behind the edge)
        x = np.pad(x, ((0, 1), (0, 1), (0, 0)))
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = x[y0][:, x0] + (x[y0][:, x1] - x[y0][:, x0]) * fx
    bot = x[y1][:, x0] + (x[y1][:, x1] - x[y1][:, x0]) * fx
    return top + (bot - top) * fy


def upsample2(x, dtype, clamp=True):
    """-> (words [2H][2W][C], exact values)."""
    x = np.asarray(x, np.float64)
    if not in_type(x, dtype):
        raise NotDyadic("upsample2: an input T does not hold")
    q = quantum(x)
    if x.size and np.abs(x).max() / q >= 2.0 ** 21:           # differences and quarter steps stay inside 24 bits
        raise NotDyadic("upsample2: input range beyond 2^21 quanta")
    exact = upsample2_exact(x, clamp)
    return rne(exact, dtype), exact


def maxpool2(x, dtype):
    x = np.asarray(x, np.float64)
    if not in_type(x, dtype):
        raise NotDyadic("maxpool2: an input T does not hold")
    h, w, c = x.shape
    exact = x.reshape(h // 2, 2, w // 2, 2, c).max(axis=(1, 3))
    return rne(exact, dtype), exact


# ---- convolution ------------------------------------------------------------------------------------------------------------
def activation(v, act, slope):
    if act == 1:
        return np.maximum(v, 0.0)
    if act == 2:
        return np.maximum(v, v * slope)                       # kernel_common.h: fmaxf(v, v * slope), slope in [0, 1]
    return v


def conv_sums(x, w, taps):
    """sum over taps and input channels of x w, "same" zero padding: x [H][W][cin], w [taps][cin][cout] -> [H][W][cout]."""
    h, wd, cin = x.shape
    cout = w.shape[2]
    if taps == 1:
        return x.reshape(-1, cin).dot(w[0]).reshape(h, wd, cout)
    xp = np.zeros((h + 2, wd + 2, cin))
    xp[1:h + 1, 1:wd + 1] = x
    y = np.zeros((h, wd, cout))
    for t in range(9):
        dy, dx = divmod(t, 3)
        y += xp[dy:dy + h, dx:dx + wd].reshape(-1, cin).dot(w[t]).reshape(h, wd, cout)
    return y


def conv(x, w, bias, taps=9, act=1, slope=0.25, res=None, pool=False, upsample=False, out_head=False, dtype=BF16, clamp=True):
    """One convolution launch.  x: [H][W][cin] values of T ([H/2][W/2][cin] with `upsample`: expanded and rounded to T first),
    w: [taps][cin][cout], bias [cout], res [H][W][cout] values of T or None.  -> dict(words, exact, budget_bits): the words
    stored ([H/2][W/2][cout] with `pool`; f16 with out_head), the exact values they round, log2 of the largest A / q'."""
    x, w, bias = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64)
    if not in_type(x, dtype) or (res is not None and not in_type(res, dtype)):
        raise NotDyadic("conv: an activation T does not hold")
    if upsample:
        words, _ = upsample2(x, dtype, clamp)
        x = to_float(words, dtype)
    qp = quantum(x) * quantum(w)
    others = [bias] + ([np.asarray(res, np.float64)] if res is not None else [])
    if quantum(*others) < qp:
        raise NotDyadic("conv: bias or residual finer than the products' quantum")
    a = conv_sums(np.abs(x), np.abs(w), taps) + np.abs(bias)
    v = conv_sums(x, w, taps) + bias
    if res is not None:
        a = a + np.abs(res)
        v = v + res
    bits = check_budget(a.max(), qp, "conv")
    v = activation(v, act, slope)
    if pool:
        h, wd, c = v.shape
        v = v.reshape(h // 2, 2, wd // 2, 2, c).max(axis=(1, 3))
    out_type = F16 if out_head else dtype
    return dict(words=rne(v, out_type), exact=v, budget_bits=bits, out_type=out_type)


def flow_block(x, w1, b1, w2, b2, act1=1, act2=1, slope=0.25, upsample=False, pool=False, out_head=False, residual=False,
               dtype=BF16, clamp=True):
    """conv A, act1, T, conv B, [+ x], act2, [pool]: two `conv`s with the intermediate rounded to T (zero outside the image).
    -> conv B's dict, with budget_a / budget_b and the intermediate's words."""
    a = conv(x, w1, b1, 9, act1, slope, None, False, upsample, False, dtype, clamp)
    mid = to_float(a["words"], dtype)
    b = conv(mid, w2, b2, 9, act2, slope, np.asarray(x, np.float64) if residual else None, pool, False, out_head, dtype)
    b.update(budget_a=a["budget_bits"], budget_b=b["budget_bits"], mid_words=a["words"], mid_exact=a["exact"])
    return b


# ---- warp -------------------------------------------------------------------------------------------------------------------
def lr_slot_table(dtype):
    """x / 255 - 0.5 of the 256 byte values as T: (words, alt) -- words: RNE of the float64 value; alt: the other accepted
    word where the four f32 evaluations a correct kernel may use (multiply by f32(1 / 255) unfused or fused, f32 division,
    the exact value) do not round to one word, else the same word."""
    b = np.arange(256)
    f = b.astype(np.float32)
    r255 = np.float32(1.0) / np.float32(255.0)
    unfused = (f * r255 - np.float32(0.5)).astype(np.float64)
    fused = (b.astype(np.float64) * np.float64(r255) - 0.5).astype(np.float32).astype(np.float64)      # one rounding
    divided = (f / np.float32(255.0) - np.float32(0.5)).astype(np.float64)
    exact = b / 255.0 - 0.5
    cands = np.stack([rne_any(c, dtype) for c in (exact, unfused, fused, divided)])
    words = cands[0]
    alt = words.copy()
    for c in cands[1:]:
        differs = c != words
        if (differs & (alt != words) & (alt != c)).any():
            raise AssertionError("three words for one byte")
        alt[differs] = c[differs]
    if (np.abs(alt.astype(np.int32) - words.astype(np.int32)) > 1).any():
        raise AssertionError("the accepted words are not neighbours")
    return words, alt


def warp(state, flow, frame, H, W, PW, pad_top, pad_left, dtype, clamp_to=2):
    """warpQuarter's definition.  state: f16 values [4H][4W][4] (multiples of 2^-9 in [-0.5, 0.5]), flow: f16 values
    [PH][PW][32] (multiples of 1/8), frame u8 [H][W][4].  -> dict(records, records_alt: words [H][W][64]; pre_warp: f16 words
    [4H][4W][4]; bgrx: u8 [4H][4W][4]; exact: the warped values [4H][4W][3])."""
    state, flow = np.asarray(state, np.float64), np.asarray(flow, np.float64)
    hh, ww = 4 * H, 4 * W
    if not in_type(state, F16) or not in_type(flow, F16):
        raise NotDyadic("warp: state and flow are f16 tensors")
    if quantum(flow) < 1.0 / 8 or quantum(state) < 2.0 ** -9 or np.abs(state).max() > 0.5:
        raise NotDyadic("warp: flows are multiples of 1/8, states multiples of 2^-9 in [-0.5, 0.5]")
    if np.abs(flow).max() >= 2.0 ** 15:
        raise NotDyadic("warp: a flow beyond 2^15 (the query would lose eighths in f32)")
    head = flow[pad_top:pad_top + H, pad_left:pad_left + W].reshape(H, W, 4, 4, 2)
    field = head.transpose(0, 2, 1, 3, 4).reshape(hh, ww, 2)          # depth-to-space(4): flow[4h+i, 4w+j, k]
    gy, gx = np.meshgrid(np.arange(hh, dtype=np.float64), np.arange(ww, dtype=np.float64), indexing="ij")
    qy, qx = gy - field[..., 0], gx - field[..., 1]

    def axis(q, size):
        fl = np.minimum(np.maximum(0.0, np.floor(q)), size - clamp_to)
        return fl.astype(np.int64), np.clip(q - fl, 0.0, 1.0)

    y0, ay = axis(qy, hh)
    x0, ax = axis(qx, ww)
    y1, x1 = y0 + 1, x0 + 1
    img = state[..., :3]
    if clamp_to != 2:                                                  # (a fault for the tests of the tests: zeros behind the edge)
        img = np.pad(img, ((0, 1), (0, 1), (0, 0)))
    ax, ay = ax[..., None], ay[..., None]
    top = ax * (img[y0, x1] - img[y0, x0]) + img[y0, x0]
    bot = ax * (img[y1, x1] - img[y1, x0]) + img[y1, x0]
    v = ay * (bot - top) + top                                         # <= 15 fractional bits: exact in f32 and float64
    slots = rne(v, dtype)                                              # [4H][4W][3]
    pre = np.zeros((hh, ww, 4), np.uint16)
    pre[..., :3] = rne(v, F16)
    records = np.zeros((H, W, 64), np.uint16)
    blocks = slots.reshape(H, 4, W, 4, 3).transpose(0, 2, 1, 3, 4)    # [h][w][i][j][c]
    for i in range(4):
        records[..., i * 16:i * 16 + 12] = blocks[:, :, i].reshape(H, W, 12)
    alt = records.copy()
    lr, lr_alt = lr_slot_table(dtype)
    bgr = np.asarray(frame)[..., :3]
    records[..., 12:15] = lr[bgr]
    alt[..., 12:15] = lr_alt[bgr]
    stored = to_float(slots, dtype).astype(np.float32)                 # the byte is made from the slot AS STORED
    byte = np.trunc(np.clip((stored + np.float32(0.5)) * np.float32(255.0), np.float32(0.0), np.float32(255.0)))
    bgrx = np.zeros((hh, ww, 4), np.uint8)
    bgrx[..., :3] = byte.astype(np.uint8)
    return dict(records=records, records_alt=alt, pre_warp=pre, bgrx=bgrx, exact=v)
