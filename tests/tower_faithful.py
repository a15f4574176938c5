"""Rounding-faithful restatement of the generator tower (test infrastructure).

The oracle (oracle/ju_oracle.py) computes the tower in float64; the engine rounds at fixed
points.  This module restates the tower so that it rounds exactly where the kernels round
(tower_kernels.hip, tower8_kernels.hip, fp8_kernels.hip, engine.cpp's tower program), and
computes every sum in float64 -- the engine's only freedom is then its fp32 summation order:

16-bit tower (tower_resident_kernel; input: the engine's `gen_in`)
  * weights: BN folded in float64 from the float32 variables, rounded once to float32
    (model.cpp foldConv / O._fold_bn), then to the compute type, round to nearest even
    (floatToF16 / floatToBF16); biases float32;
  * layer 0 is generator/conv_1 (51 -> 64), then conv_1 / conv_2 of every block;
  * every layer: accumulator = bias + sum of products in fp32, (+ the 16-bit stream for a
    block's conv_2), activation in fp32 (ReLU: on the packed 16-bit value, which is the same
    number), stored as the compute type, RNE (pack4: v_cvt_pk_*_f32).

8-bit tower (tower8_resident_kernel, res_block_fp8_kernel, conv_tower_fp8_kernel; input: the
engine's `trunk_a`, generator/conv_1's fp16 output)
  * weights: the float32 fold, per output channel e4m3 with a power-of-two scale
    (fp8.h packFp8TowerWeights / O.fp8_quantize_weights);
  * block 0's e4m3 input: e4m3(clamp(x * 2^ex)) of the fp16 stream -- clamp [0, 448] for
    ReLU (it is the ReLU), [-448, 448] for LeakyReLU;
  * conv A: bias + products (exact: e4m3 x e4m3, power-of-two scales), activation,
    t8 = e4m3(clamp(t * 2^et));
  * conv B: bias + products + the fp16 stream, activation: the fp32 value v.  The stream
    is fp16(v), RNE; the NEXT block's e4m3 input is quantised from v itself, not from the
    rounded stream (o8 and o16 are both computed from v in every 8-bit epilogue).

Products of e4m3 operands and of 16-bit operands are exact in float64, and the float64
sums of one output element carry at most a rounding in the 53rd bit, so the restatement
is the exact tower up to the fp32 roundings it deliberately leaves out.
"""

import numpy as np

from helpers import O

BF16, F16 = "bf16", "fp16"


# -- roundings ----------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def to_bf16(x, truncate=False):
    """float -> fp32 -> bf16 (RNE, or truncation), back as float64."""
    u = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)).view(np.uint32).astype(np.uint64)
    if not truncate:
        u = u + 0x7fff + ((u >> 16) & 1)
    u = (u >> 16) << 16
    return (u & 0xffffffff).astype(np.uint32).view(np.float32).astype(np.float64)


def to_f16(x, truncate=False):
    """float -> fp32 -> fp16 (RNE, or truncation towards zero), back as float64."""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    h = x32.astype(np.float16)
    if truncate:   # one step towards zero wherever RNE rounded away from zero
        up = np.abs(h.astype(np.float32)) > np.abs(x32)
        h = np.where(up, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float64)


def to_stream(x, dtype, truncate=False):
    return to_bf16(x, truncate) if dtype == BF16 else to_f16(x, truncate)


def ulp(x, dtype):
    """Spacing of the stream type at |x| (its subnormal spacing below the smallest normal)."""
    a = np.abs(np.asarray(x, np.float64))
    mant, emin = (7, -126) if dtype == BF16 else (10, -14)
    _, e = np.frexp(a)
    return np.exp2(np.maximum(np.where(a > 0, e - 1, emin), emin) - mant)


def e4m3(x, exponent, leaky):
    """The value of the e4m3 byte the kernels store for x: e4m3(clamp(x * 2^e)) * 2^-e."""
    lo = -448.0 if leaky else 0.0
    return O.e4m3_round(np.clip(np.asarray(x, np.float64) * 2.0 ** exponent, lo, 448.0)) * 2.0 ** -exponent


def act(x, leaky, slope):
    return np.maximum(x, x * slope) if leaky else np.maximum(x, 0.0)


# -- the convolution ----------------------------------------------------------------------------------------
# A mutant is (kind, layer, arg): the restatement with one deliberate kernel bug in one layer, for the tests that
# show the trunk comparison's bounds catch such bugs.  Kinds:
#   "halo_row"  output row `arg` (a 16-row region edge) reads the input row above it as zero
#   "halo_col"  output column `arg` (a 32-column region edge) reads the input column left of it as zero
#   "last_row"  the layer's last output row is never written (stays zero)
#   "k_slice"   input channels 8 arg .. 8 arg + 7 of the centre tap are left out
#   "tap"       tap (0, 0) is left out
#   "truncate"  the stream store truncates instead of rounding to nearest even
MUTANTS = ("halo_row", "halo_col", "last_row", "k_slice", "tap", "truncate")


def conv3x3(x, k, bias, accumulate="f64", mutant=None):
    """SAME 3x3 convolution + bias, as im2col + one matmul per band of about 32k output pixels.
    accumulate="f64": float64 sums (exact for the operands here); "f32": float32 sums in BLAS
    order over the taps in reverse -- a summation order other than the restatement's, standing
    in for the MFMA order."""
    h, w, cin = x.shape
    kk = np.asarray(k, np.float64).reshape(9 * cin, -1)
    xp = np.zeros((h + 2, w + 2, cin), np.float64)
    xp[1:h + 1, 1:w + 1] = x
    kind, arg = (mutant[0], mutant[2]) if mutant else (None, None)
    rows = max(1, 32768 // w)
    out = np.empty((h, w, kk.shape[1]), np.float64)
    if accumulate == "f32":
        order = np.arange(9 * cin).reshape(9, cin)[::-1].ravel()
        kk32 = kk[order].astype(np.float32)
    for r0 in range(0, h, rows):
        r1 = min(h, r0 + rows)
        cols = np.empty((r1 - r0, w, 9, cin), np.float64)
        for a in range(3):
            for b in range(3):
                cols[:, :, a * 3 + b] = xp[r0 + a:r1 + a, b:b + w]
        if kind == "halo_row" and r0 <= arg < r1:
            cols[arg - r0, :, 0:3] = 0.0
        elif kind == "halo_col":
            cols[:, arg, 0::3] = 0.0
        elif kind == "k_slice":
            cols[:, :, 4, 8 * arg:8 * arg + 8] = 0.0
        elif kind == "tap":
            cols[:, :, 0] = 0.0
        cols = cols.reshape((r1 - r0) * w, 9 * cin)
        if accumulate == "f32":
            y = (cols[:, order].astype(np.float32) @ kk32 + np.asarray(bias, np.float32)).astype(np.float64)
        else:
            y = cols @ kk + bias
        out[r0:r1] = y.reshape(r1 - r0, w, -1)
    return out


def _mut(mutant, layer):
    return mutant if mutant is not None and mutant[1] == layer else None


def _store(v, layer, mutant, fn):
    m = _mut(mutant, layer)
    out = fn(v, m is not None and m[0] == "truncate")
    if m is not None and m[0] == "last_row":
        out[-1] = 0.0
    return out


# -- weights ------------------------------------------------------------------------------------------------
def fold(wts, conv, bn, eps, exact=False):
    """BN folded into the convolution: the engine's float32 fold (O._fold_bn), or (exact) the
    same algebra in float64 -- what O.res_block computes."""
    if not exact:
        k, b = O._fold_bn(wts, conv, bn, eps)
        return k.astype(np.float64), b.astype(np.float64)
    f8 = np.float64
    g = np.asarray(wts[bn + "/gamma"], f8)
    scale = g / np.sqrt(np.asarray(wts[bn + "/moving_variance"], f8) + f8(np.float32(eps)))
    bias = np.asarray(wts[bn + "/beta"], f8) - np.asarray(wts[bn + "/moving_mean"], f8) * scale
    return np.asarray(wts[conv + "/kernel"], f8) * scale, bias


# -- the two towers -----------------------------------------------------------------------------------------
def tower16(gen_in, wts, blocks, eps, dtype, leaky=False, slope=0.3, rounding=True, accumulate="f64",
            mutant=None):
    """The 16-bit resident tower: generator/conv_1 and `blocks` residual blocks.
    gen_in: [H, W, 51] in the reference channel order (helpers.gen_in_to_reference of the
    engine's `gen_in`).  rounding=False: float64 everywhere (weights folded in float64 too) --
    then this IS the oracle's generator/conv_1 + res_block chain.  Layers are numbered 0
    (conv_1), then 2 i + 1 / 2 i + 2 for block i's conv_1 / conv_2 (the kernel's order).
    Returns the trunk, [H, W, 64]."""
    slope = float(np.float32(slope))

    def weights(conv, bn):
        k, b = fold(wts, conv, bn, eps, exact=not rounding)
        return (to_stream(k, dtype) if rounding else k), b

    def store(v, layer):
        return _store(v, layer, mutant, (lambda y, t: to_stream(y, dtype, t)) if rounding else (lambda y, t: y))

    k, b = weights("generator/conv_1", "generator/bn_1")
    x = store(act(conv3x3(gen_in, k, b, accumulate, _mut(mutant, 0)), leaky, slope), 0)
    for i in range(blocks):
        n = f"generator/block_{i + 1}"
        k1, b1 = weights(n + "/conv_1", n + "/bn_1")
        k2, b2 = weights(n + "/conv_2", n + "/bn_2")
        t = store(act(conv3x3(x, k1, b1, accumulate, _mut(mutant, 2 * i + 1)), leaky, slope), 2 * i + 1)
        x = store(act(conv3x3(t, k2, b2, accumulate, _mut(mutant, 2 * i + 2)) + x, leaky, slope), 2 * i + 2)
    return x


def fp8_exponents(wts, blocks):
    """Per-tensor exponents of the 2 x blocks e4m3 conv inputs (generator/fp8_amax, else
    kFp8DefaultAmax): what engine.cpp's m_Fp8Exp holds."""
    amax = wts.get("generator/fp8_amax")
    return [O.fp8_activation_exponent(O.FP8_DEFAULT_AMAX if amax is None else float(np.float32(amax[j])))
            for j in range(2 * blocks)]


def tower8(trunk_a, wts, blocks, eps, leaky=False, slope=0.3, rounding=True, accumulate="f64", mutant=None):
    """The 8-bit tower from its fp16 input (the engine's `trunk_a`).  rounding=False: the
    stream stays float64 and nothing is rounded to fp32 (the e4m3 quantisation is the scheme
    itself and stays) -- then this IS the oracle's res_block_fp8 chain.  Layers: 2 i / 2 i + 1
    for block i's conv_1 / conv_2; a "truncate" mutant acts on the fp16 stream store of the
    layer's block.  Returns the trunk, [H, W, 64]."""
    slope = float(np.float32(slope))
    exps = fp8_exponents(wts, blocks)
    r32 = f32 if rounding else (lambda y: y)
    x = np.asarray(trunk_a, np.float64)
    v = x
    for i in range(blocks):
        n = f"generator/block_{i + 1}"
        k1, b1 = fold(wts, n + "/conv_1", n + "/bn_1", eps)
        k2, b2 = fold(wts, n + "/conv_2", n + "/bn_2", eps)
        x8 = e4m3(v, exps[2 * i], leaky)
        t = r32(act(conv3x3(x8, O.fp8_quantize_weights(k1), b1, accumulate, _mut(mutant, 2 * i)), leaky, slope))
        m = _mut(mutant, 2 * i)
        if m is not None and m[0] == "last_row":
            t[-1] = 0.0
        t8 = e4m3(t, exps[2 * i + 1], leaky)
        v = r32(act(conv3x3(t8, O.fp8_quantize_weights(k2), b2, accumulate, _mut(mutant, 2 * i + 1)) + x,
                    leaky, slope))
        m = next((mm for mm in (_mut(mutant, 2 * i), _mut(mutant, 2 * i + 1)) if mm and mm[0] == "truncate"), None)
        x = to_f16(v, m is not None) if rounding else v
        m = _mut(mutant, 2 * i + 1)
        if m is not None and m[0] == "last_row":
            x[-1] = 0.0
            v = v.copy()
            v[-1] = 0.0
    return x


# -- the comparison and its bounds --------------------------------------------------------------------------
def compare(got, ref, dtype):
    """The engine's trunk against the restatement, in units of the stream type's spacing at the
    larger of the two magnitudes, floored at 1/16 of the reference's RMS (below that the fp32
    summation error of a sum of many terms is not small relative to the result, and a
    near-zero element measured in its own spacing would count a cancellation as thousands of
    ulps).  Share of elements more than 1 unit off, the largest difference, and the mean signed
    difference (a one-sided store rounding shows there)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), (got.shape, ref.shape)
    floor = np.sqrt(np.mean(ref * ref)) / 16.0
    d = (got - ref) / ulp(np.maximum(np.maximum(np.abs(got), np.abs(ref)), floor), dtype)
    a = np.abs(d)
    return {"frac_gt1ulp": float(np.mean(a > 1.0)), "max_ulp": float(a.max()), "mean_ulp": float(d.mean()),
            "n": int(a.size)}


# Bounds of the trunk comparison: 1.4 x the worst value measured on MI355X (8-bit: 1.1-1.4 x; gpu_common.py's header).
# Summation-order differences do not stay where they arise: a flipped rounding of one element perturbs the 9 x 64
# outputs it feeds in the next layer, so two faithful towers that sum in different orders drift apart with depth,
# and a 24-block 16-bit tower has bounds of its own.  The 16-bit engine sits at the level of the float32-reordered
# restatement (test_tower_faithful_cpu.py).  The 8-bit engine's e4m3 matrix instruction does not return the
# correctly rounded sum of its 64 products (tools/probes/fp8_mfma_accumulation_probe.hip: off by up to ~2^-11 of the
# largest product), and where that flips an e4m3 rounding the step is 1/16 of one operand; so its bounds are held
# on towers of at most 2 blocks (both convolutions, both halo exchanges, the stream store), past which these flips
# spread over the whole trunk.
BOUNDS = {
    # (kind, 24 blocks): share > 1 unit, max units, |mean| units
    (BF16, False): dict(frac=0.0131, max=48.3, mean=0.0015),
    (F16, False): dict(frac=0.0498, max=70.0, mean=0.015),
    ("fp8", False): dict(frac=0.374, max=794.0, mean=0.08),
    (BF16, True): dict(frac=0.485, max=126.0, mean=0.0175),
    (F16, True): dict(frac=0.499, max=151.2, mean=0.0227),
}


def bounds(kind, blocks):
    """kind: "bf16" / "fp16" (the 16-bit towers: at most 5 blocks, or 24) or "fp8" (at most 2 blocks)."""
    if kind == "fp8":
        assert blocks <= 2, ("8-bit towers are compared at up to 2 blocks, not", blocks)
    else:
        assert blocks <= 5 or blocks == 24, ("no measured basis for a tower of", blocks, "blocks")
    return BOUNDS[(kind, blocks == 24)]


def within(st, kind, blocks):
    b = bounds(kind, blocks)
    return st["frac_gt1ulp"] <= b["frac"] and st["max_ulp"] <= b["max"] and abs(st["mean_ulp"]) <= b["mean"]
