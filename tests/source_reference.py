"""The source stage in numpy, in integers only (docs/source_stage.md is the prose): the triangle scaler that brings a
source of any size to the model's input, and the masked pass-through of the source over the upscaled frame.  The HIP
kernels (csrc/source_kernels.hip) and the C++ table builder (buildScaleAxis) must give these bytes exactly.

Images are ``[H, W, 4]`` uint8, byte order B, G, R, X; X is ignored on input and written 0."""

import struct
import zlib

import numpy as np

MAX_TAPS = 33
AXIS_MIN, AXIS_MAX, RATIO_MAX = 2, 8192, 16


def axis_table(n: int, m: int):
    """One axis, ``n`` source samples -> ``m`` destination samples: ``(start [m], count [m], taps [m, MAX_TAPS])``.

    Raw weight of source index s for destination index d, with D = 2 max(n, m):
    ``w = max(0, D - |(2s+1) m - (2d+1) n|)`` -- a triangle at the pixel centres, widened by n / m when downscaling;
    taps outside [0, n) are dropped.  ``q = floor(4096 w / S)`` with S the row's sum of w; the remainder 4096 - sum(q)
    goes to the tap with the largest w, the first on a tie."""
    assert n >= 1 and m >= 1 and n <= RATIO_MAX * m and m <= RATIO_MAX * n, (n, m)
    big = 2 * max(n, m)
    s = np.arange(n, dtype=np.int64)
    start = np.zeros(m, np.int64)
    count = np.zeros(m, np.int64)
    taps = np.zeros((m, MAX_TAPS), np.int64)
    for d in range(m):
        w = np.maximum(0, big - np.abs((2 * s + 1) * m - (2 * d + 1) * n))
        nz = np.flatnonzero(w)
        lo, hi = int(nz[0]), int(nz[-1]) + 1
        assert hi - lo == nz.size and nz.size <= MAX_TAPS           # (one run, by the shape of the triangle)
        w = w[lo:hi]
        q = w * 4096 // int(w.sum())
        q[int(np.argmax(w))] += 4096 - int(q.sum())                  # (argmax: the first of the largest)
        start[d], count[d] = lo, hi - lo
        taps[d, :hi - lo] = q
    return start, count, taps


def _apply_axis(table, x):
    """sum over taps of q * x along axis 0 of ``x`` (int64): [n, ...] -> [m, ...]."""
    start, count, taps = table
    out = np.zeros((start.size,) + x.shape[1:], np.int64)
    last = x.shape[0] - 1
    for t in range(int(count.max())):
        q = taps[:, t].reshape((-1,) + (1,) * (x.ndim - 1))
        out += q * x[np.minimum(start + t, last)]                    # (past a row's count the tap is 0)
    return out


def scale(src: np.ndarray, mh: int, mw: int) -> np.ndarray:
    """``src [H, W, 4]`` -> ``[mh, mw, 4]``: out = (sum over y, x of qy qx src + 2^23) >> 24 per channel, in 32 unsigned
    bits (asserted), no rounding between the axes, no clipping; X = 0."""
    h, w = src.shape[:2]
    v = _apply_axis(axis_table(h, mh), src[..., :3].astype(np.int64))                    # [mh, W, 3], <= 255 * 4096
    assert int(v.max(initial=0)) < 1 << 20
    acc = _apply_axis(axis_table(w, mw), v.transpose(1, 0, 2)).transpose(1, 0, 2) + (1 << 23)
    assert int(acc.max(initial=0)) < 1 << 32
    out = np.zeros((mh, mw, 4), np.uint8)
    out[..., :3] = acc >> 24
    return out


def scale_float(src: np.ndarray, mh: int, mw: int) -> np.ndarray:
    """The same triangle filter with its coefficients unquantised, in float64, not rounded: ``[mh, mw, 3]``."""
    def matrix(n, m):
        big = 2 * max(n, m)
        s, d = np.arange(n, dtype=np.int64)[None, :], np.arange(m, dtype=np.int64)[:, None]
        wgt = np.maximum(0, big - np.abs((2 * s + 1) * m - (2 * d + 1) * n)).astype(np.float64)
        return wgt / wgt.sum(1, keepdims=True)
    h, w = src.shape[:2]
    x = src[..., :3].astype(np.float64)
    return np.einsum("dh,hwc,ew->dec", matrix(h, mh), x, matrix(w, mw), optimize=True)


def texel(i: np.ndarray, size: int, out_size: int) -> np.ndarray:
    """The texel of a ``size``-wide texture under the centre of output pixel i (point sampling)."""
    return (2 * i.astype(np.int64) + 1) * size // (2 * out_size)


def blend(gen: np.ndarray, src: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """The source drawn over ``gen [OH, OW, 4]`` through the mask, each texture of its own size: a = 765 - (Rm + Gm +
    Bm), out = (src a + gen (765 - a) + 382) // 765 for B, G, R and X = 0; pixels with a == 0 keep gen's four bytes."""
    oh, ow = gen.shape[:2]
    ys, xs = np.arange(oh), np.arange(ow)
    m = mask[texel(ys, mask.shape[0], oh)[:, None], texel(xs, mask.shape[1], ow)[None, :]]
    s = src[texel(ys, src.shape[0], oh)[:, None], texel(xs, src.shape[1], ow)[None, :]]
    a = 765 - m[..., :3].astype(np.int64).sum(-1)
    mixed = np.zeros_like(gen)
    mixed[..., :3] = (s[..., :3].astype(np.int64) * a[..., None] + gen[..., :3].astype(np.int64) * (765 - a[..., None]) + 382) // 765
    return np.where((a == 0)[..., None], gen, mixed)


def read_png_palette_1bit(path: str) -> np.ndarray:
    """A non-interlaced 1-bit palette PNG (the reference's mask.png) as a BGRX ``[H, W, 4]`` image, X = 255."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        size, = struct.unpack(">I", data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        chunks[kind] = chunks.get(kind, b"") + data[pos + 8:pos + 8 + size]
        pos += 12 + size
    w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", chunks[b"IHDR"])
    assert (depth, colour, interlace) == (1, 3, 0)
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8)
    pitch = (w + 7) // 8
    rows = raw.reshape(h, pitch + 1)
    lines = np.zeros((h, pitch), np.uint8)
    for y in range(h):                                               # PNG filters on whole bytes (bpp = 1)
        f, cur = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = lines[y - 1].astype(np.int64) if y else np.zeros(pitch, np.int64)
        if f == 0:
            pass
        elif f == 2:
            cur = cur + up
        else:
            for x in range(pitch):
                a = int(cur[x - 1]) & 255 if x else 0
                b, c = int(up[x]), (int(up[x - 1]) if x else 0)
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) // 2
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (cur[x] + pred) & 255
        lines[y] = cur & 255
    index = np.unpackbits(lines, axis=1)[:, :w]
    palette = np.frombuffer(chunks[b"PLTE"], np.uint8).reshape(-1, 3)
    out = np.full((h, w, 4), 255, np.uint8)
    out[..., :3] = palette[index][..., ::-1]                         # RGB -> BGR
    return out
