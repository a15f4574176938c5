"""The temporal output filter alone (csrc/frame_kernels.hip: zero_words_kernel, temporal_reduce_kernel,
temporal_blend_kernel; the hook ju_debug_temporal): its definition in float64 on top of oracle.ju_oracle.temporal_filter,
the two helpers the GPU test checks a run with, and the table of cases both test files run.

The definition (`define`), for a state tensor s (f16, generator output minus brightness), pre_warp p (f16) and the six
words of the frame sums:

    b        = sum_c luma_c (S_c / (255 N) - 0.5)          N LR pixels; 0 without sums
    gen      = s + b
    filtered = ju_oracle.temporal_filter(gen, p, ...)
    state'   = filtered - b
    byte     = trunc(clip((filtered + 0.5) * 255, 0, 255))  saturated; the fed-back state is not
    sums     = per-window sums of the gate terms = temporal_mean * (3 window^2, or 3 HH WW for the global gate)

Blend from the accumulators a run returned (`gate_from_acc`, `blend`): the kernels do two things, a reduction into 32.32
fixed-point sums and a blend gated by them.  The gate is defined on the integers: mean = acc / 2^32 / denom, d = mean -
float64(threshold) in float64, c = sign(d) (sign(0) = 0) or tanh(gain d), the asymmetric-linear resize with the clamped
neighbour, the un-pad slice.  Every float64 step there is the kernel's own, so a hard gate decides as the kernel did and
no threshold has to be "far from everything".

Acceptance intervals (`intervals`): the stored types round, so a result is accepted when the byte lies in
[byte(r - e), byte(r + e)] and the f16 state between the f16 neighbours enclosing [r - b - e, r - b + e].  The bound e
on the blend arithmetic, per element, from the kernel's f32 operations (unit round-off u = 2^-24; contraction to FMA
only removes roundings; strength <= 1, so half = strength / 2 <= 0.5 is exact):

    m1 = half - c half            product u half, difference u |m1|               <= 1.5 u
    m2 = c half + 1 - half        product 0.5 u, sum 1.5 u, difference u           <= 3 u
    gen = s + b                   u |gen| + db     (no rounding and db = 0 without sums: an f16 value is exact in f32)
    r = p m1 + gen m2             |p| 1.5 u + |gen| 3 u + (u |gen| + db) + u |p| + u |gen| + u |r|
    state' = r - b                u (|r| + 0.5) + db
    byte   = (r + 0.5) * 255      u (|r| + 0.5) for the sum, the same again for the product, in units of r

    e = u (2.5 |p| + 5 |gen| + 3 |r| + 1) + 2 db + half |p - gen| dc

which is 22 u = 2^-19.5 for values up to 2 and 6.25 u = 2^-21.4 for values up to 0.5.  db, the f32 evaluation of b
(brightnessOf): the integer's conversion, 1 / N, the product, the division by 255 (4 u on a value <= 1), the subtraction
(0.5 u), then three weights rounded to f32 and three products (2 u on sum_c luma_c |m_c| <= 0.5) and two sums (2 u |b|
<= u): db = 7 u.  dc, the error of the gate value c the blend uses against `gate_from_acc`:

    windowed   src = (y + pad) / window in f32 has an error of u src (none for window 1), which the fraction inherits;
               the differences of gate cells are at most 2, and the lerps add 3 u per row and 5 u for the column:
                                                                            dc += u (2 (src_y + src_x) + 8)
    tanh gate  d rounded to f32 and the f32 product d gain each move the argument z by u |z|, and |z| tanh'(z) <= 0.45;
               tanhf itself is taken to be good to 4 ulp of a value below 1, 4 u:       dc += 5 u

The reduction's own tolerance (`reduce_tolerance`): 2^-16 of the window's sum of |term|, plus 2^-16 per term when the
sums are given.  A term costs 8 (L1) to 20 (L2, luma, the three-term sum, the wave's tree) roundings of 2^-24 relative,
and b's error of 7 u enters a term at most 11 times (L2: 2 |d| k^2 <= 2 * 2 * 3.1 at |d| <= 2, less 1 for L1); the
conversion to fixed point adds 2^-33 per pixel, which is 2^-19 of a pixel's terms at the most, because `build` keeps those
above 2^-14 (a 32.32 sum cannot be held to a relative bound on windows whose terms vanish).  2^-16 is 100 times the
roundings or more, and 8 times the fixed-point step.
"""

import numpy as np

from helpers import O

U = 2.0 ** -24
DB = 7 * U
SCALE = 2.0 ** 32
FLAG_L2, FLAG_LIMIT, FLAG_LUMA = 1, 2, 4


# ---- geometry --------------------------------------------------------------------------------------------------------
def geometry(h, w, window):
    """(HH, WW, GH, GW, pad_y, pad_x) of an LR frame of h x w: frame_moving_avg.py:211-218."""
    hh, ww = 4 * h, 4 * w
    if window == 0:
        return hh, ww, 1, 1, 0, 0
    gh, gw = (hh + window - 1) // window, (ww + window - 1) // window
    return hh, ww, gh, gw, (gh * window - hh) // 2, (gw * window - ww) // 2


def cell_index(h, w, window):
    """The gate cell of every HR pixel, [HH, WW]."""
    hh, ww, gh, gw, py, px = geometry(h, w, window)
    if window == 0:
        return np.zeros((hh, ww), np.int64)
    return ((np.arange(hh) + py) // window)[:, None] * gw + ((np.arange(ww) + px) // window)[None, :]


def brightness(sums, n_lr):
    """b from the six words of the frame sums (three 64-bit sums, low word first); 0 without them."""
    if sums is None:
        return 0.0
    s = np.asarray(sums, np.uint32).astype(np.uint64)
    total = [int(s[2 * c]) | (int(s[2 * c + 1]) << 32) for c in range(3)]
    return float(sum(O.BGR_LUMA[c] * (total[c] / (255.0 * n_lr) - 0.5) for c in range(3)))


# ---- the definition ----------------------------------------------------------------------------------------------------
def define(state, pre_warp, sums, h, w, run):
    """state, pre_warp: f16 [HH, WW, 4] (lane 3 unused).  run: strength, threshold, gain, window, l2, limit, luma."""
    hh, ww, gh, gw, _, _ = geometry(h, w, run["window"])
    b = brightness(sums, h * w)
    gen = state[..., :3].astype(np.float64) + b
    p = pre_warp[..., :3].astype(np.float64)
    tr = {}
    filtered = O.temporal_filter(gen, p, float(run["strength"]), float(np.float32(run["threshold"])), run["window"],
                                 float(run["gain"]), "L2" if run["l2"] else "L1", bool(run["limit"]), bool(run["luma"]), tr)
    denom = 3.0 * hh * ww if run["window"] == 0 else 3.0 * run["window"] ** 2
    mean = np.asarray(tr["temporal_mean"], np.float64).reshape(gh, gw)
    terms = 3 * np.bincount(cell_index(h, w, run["window"]).ravel(), minlength=gh * gw).reshape(gh, gw)
    return dict(b=b, gen=gen, p=np.clip(p, -0.5, 0.5) if run["limit"] else p, filtered=filtered, state=filtered - b,
                byte=to_byte(filtered), mean=mean, sums=mean * denom, terms=terms, denom=denom)


def to_byte(r):
    return np.trunc(np.clip((r + 0.5) * 255.0, 0.0, 255.0)).astype(np.uint8)


# ---- helper 1: the blend from a run's accumulators ---------------------------------------------------------------------
def gate_cells(acc, denom, run):
    d = np.asarray(acc, np.uint64).astype(np.float64) / SCALE / denom - np.float64(np.float32(run["threshold"]))
    return np.sign(d) if run["gain"] == 0 else np.tanh(d * np.float64(np.float32(run["gain"])))


def resize_axis(n_out, pad, window, n_cells):
    src = (np.arange(n_out) + pad) / np.float64(window)
    lo = np.floor(src).astype(np.int64)
    return lo, np.minimum(lo + 1, n_cells - 1), src - lo


def gate_from_acc(acc, h, w, run):
    """c for every HR pixel, [HH, WW, 1], from the integer accumulators (row-major window grid)."""
    hh, ww, gh, gw, py, px = geometry(h, w, run["window"])
    if run["window"] == 0:
        return np.full((hh, ww, 1), gate_cells(acc[:1], 3.0 * hh * ww, run)[0])
    cg = gate_cells(acc[:gh * gw], 3.0 * run["window"] ** 2, run).reshape(gh, gw)
    y0, y1, fy = resize_axis(hh, py, run["window"], gh)
    x0, x1, fx = resize_axis(ww, px, run["window"], gw)
    fy, fx = fy[:, None], fx[None, :]
    top = cg[y0][:, x0] + (cg[y0][:, x1] - cg[y0][:, x0]) * fx
    bot = cg[y1][:, x0] + (cg[y1][:, x1] - cg[y1][:, x0]) * fx
    return (top + (bot - top) * fy)[..., None]


def blend(d, c, run):
    half = float(run["strength"]) / 2
    return d["p"] * (half - c * half) + d["gen"] * (c * half + 1 - half)


# ---- helper 2: acceptance intervals -------------------------------------------------------------------------------------
def error_bound(d, r, h, w, run, has_sums):
    hh, ww, _, _, py, px = geometry(h, w, run["window"])
    dc = 5 * U if run["gain"] else 0.0
    if run["window"]:
        sy, sx = (np.arange(hh) + py) / run["window"], (np.arange(ww) + px) / run["window"]
        src = (sy[:, None] + sx[None, :] if run["window"] > 1 else np.zeros((hh, ww)))[..., None]
        dc = dc + U * (8 + 2 * src)
    half = float(run["strength"]) / 2
    return (U * (2.5 * np.abs(d["p"]) + 5 * np.abs(d["gen"]) + 3 * np.abs(r) + 1) + (2 * DB if has_sums else 0.0)
            + half * np.abs(d["p"] - d["gen"]) * dc)


def f16_floor(x):
    v = x.astype(np.float16)
    return np.where(v.astype(np.float64) > x, np.nextafter(v, np.float16(-np.inf)), v)


def f16_ceil(x):
    v = x.astype(np.float16)
    return np.where(v.astype(np.float64) < x, np.nextafter(v, np.float16(np.inf)), v)


def intervals(r, b, e):
    """(byte lo, byte hi, f16 state lo, f16 state hi), inclusive."""
    return to_byte(r - e), to_byte(r + e), f16_floor(r - b - e), f16_ceil(r - b + e)


def reduce_tolerance(d, has_sums):
    return 2.0 ** -16 * np.abs(d["sums"]) + (2.0 ** -16 * d["terms"] if has_sums else 0.0)


def is_hard_cut(acc, h, w, run):
    """The global sign gate that says "scene cut": the kernel leaves the tail's bytes and state alone."""
    hh, ww = 4 * h, 4 * w
    return run["window"] == 0 and run["gain"] == 0 and gate_cells(acc[:1], 3.0 * hh * ww, run)[0] > 0


def check_run(case, data, d, run, acc, out, state, out_before=None):
    """A run's results (acc: uint64 words, at least the grid; out: u8 [HH, WW, 4]; state: f16 [HH, WW, 4]) against the
    definition `d`: (failures, figures).  `out_before`: what `out` held before the run (a hard cut keeps it)."""
    h, w = case["h"], case["w"]
    hh, ww, gh, gw, _, _ = geometry(h, w, run["window"])
    has_sums = data["sums"] is not None
    fails, fig = [], {}
    acc = np.asarray(acc, np.uint64)
    got = acc[:gh * gw].astype(np.float64).reshape(gh, gw) / SCALE
    dev, tol = np.abs(got - d["sums"]), reduce_tolerance(d, has_sums)
    fig["acc_dev_over_tol"] = float(np.max(dev / np.maximum(tol, 1e-300))) if dev.any() else 0.0
    fig["acc_dev_rel"] = float(np.max(dev / np.maximum(np.abs(d["sums"]), 1e-300))) if dev.any() else 0.0
    if (dev > tol).any():
        k = int(np.argmax(dev - tol))
        fails.append(f"reduce: window {k} sum {got.ravel()[k]!r} != {d['sums'].ravel()[k]!r} (tolerance {tol.ravel()[k]:.3g})")
    if acc[gh * gw:].any():
        fails.append("reduce: a word behind the window grid is not zero")
    if is_hard_cut(acc, h, w, run):
        fig["hard_cut"] = 1
        if not np.array_equal(state.view(np.uint16), data["state"].view(np.uint16)):
            fails.append("hard cut: the state changed")
        if out_before is not None and not np.array_equal(out, out_before):
            fails.append("hard cut: the frame changed")
        return fails, fig
    r = blend(d, gate_from_acc(acc, h, w, run), run)
    e = error_bound(d, r, h, w, run, has_sums)
    blo, bhi, slo, shi = intervals(r, d["b"], e)
    byte, st = out[..., :3], state[..., :3]
    bad = (byte < blo) | (byte > bhi)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        fails.append(f"blend: {int(bad.sum())} bytes outside their interval, first at {i}: {int(byte[i])} not in "
                     f"[{int(blo[i])}, {int(bhi[i])}] (r = {r[i]!r})")
    bad = ~((st >= slo) & (st <= shi))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        fails.append(f"blend: {int(bad.sum())} state elements outside their interval, first at {i}: {float(st[i])!r} not "
                     f"in [{float(slo[i])!r}, {float(shi[i])!r}]")
    if out[..., 3].any():
        fails.append("blend: X is not 0")
    if state[..., 3].view(np.uint16).any():
        fails.append("blend: lane 3 of the state is not +0")
    fig["byte_off_centre"] = float(np.mean(byte != to_byte(r)))
    fig["state_off_centre"] = float(np.mean(st.view(np.uint16) != (r - d["b"]).astype(np.float16).view(np.uint16)))
    fig["byte_two_valued"] = float(np.mean(blo != bhi))
    return fails, fig


# ---- the case table --------------------------------------------------------------------------------------------------------
# kind: "plain" values within +-0.5, no sums; "wide" pre_warp out to +-1.5, no sums; "bright" / "dark": wide, with sums
# that give b near +0.3 / -0.2.  The modes (L1 / L2 x luma x limit x gain 0 / 25) are looped over inside a case.
STRENGTHS = (0.5, 1.0, 0.25)
LAYOUTS = ("dense", "padded", "bottom-up")
KINDS = ("plain", "wide", "bright", "dark")
GEOMETRIES = [
    # (h, w, windows)                                     HR size; what the windows give
    (1, 1, (0, 1, 3, 5)),                               # 4 x 4: 3 -> 2 x 2 cells, padding 2 (even); 5 -> one cell, padding 1 (odd)
    (3, 5, (0, 5, 7, 16, 24)),                          # 12 x 20: 5 -> padding 3 / 0; 7 -> 2 / 1; 16 -> GH = 1, GW = 2; 24 -> 1 x 1
    (5, 3, (16,)),                                      # 20 x 12: GH = 2, GW = 1
    (5, 7, (0, 3, 7, 24, 64)),                          # 20 x 28: 3 -> padding 1 / 2; 7 -> 1 / 0; 24 -> GH = 1; 64 -> 1 x 1
    (16, 16, (0, 1, 5, 16, 24, 64)),                    # 64 x 64: 1, 16, 64 -> no padding (64: the wave-uniform path); 5 -> 1; 24 -> 8
    (30, 48, (0, 3, 5, 7, 16, 24, 64)),                 # 120 x 192: 7 -> padding 6 / 4; 16 -> 8 / 0; 64 -> 8 / 0
]
MODES = [dict(l2=l2, luma=luma, limit=limit, gain=gain) for l2 in (0, 1) for luma in (0, 1) for limit in (0, 1) for gain in (0.0, 25.0)]
BIG = dict(name="363x362-w0-bright", h=363, w=362, window=0, kind="bright", strength=0.5, layout="padded", seed=999,
           modes=[dict(l2=0, luma=1, limit=0, gain=25.0)])    # 131406 LR pixels: HR pixels > 2048 * 256, a thread's second element
HUGE_WINDOW = dict(name="30x48-w4096-wide", h=30, w=48, window=4096, kind="wide", strength=0.5, layout="dense", seed=998,
                   modes=[dict(l2=0, luma=0, limit=0, gain=0.0), dict(l2=1, luma=1, limit=1, gain=25.0)])


def _cases():
    out, k = [], 0
    for h, w, windows in GEOMETRIES:
        for window in windows:
            kind = KINDS[k % 4]
            out.append(dict(name=f"{h}x{w}-w{window}-{kind}", h=h, w=w, window=window, kind=kind, strength=STRENGTHS[k % 3],
                            layout=LAYOUTS[(k // 3) % 3], seed=100 + k, modes=MODES))
            k += 1
    return out + [HUGE_WINDOW, BIG]


CASES = _cases()


def sums_words(h, w, target, rng):
    """Six words whose b is near `target`, the three channel means apart from each other."""
    n = h * w
    words = []
    for c, off in enumerate((0.06, 0.0, -0.05)):
        s = int(round(n * 255 * min(max(0.5 + target + off + rng.uniform(-0.01, 0.01), 0.0), 1.0)))
        words += [s & 0xFFFFFFFF, s >> 32]
    return np.array(words, np.uint32)


def build(case):
    """The inputs of a case: state, pre_warp (f16 [HH, WW, 4], lane 3 holds finite junk), sums (six u32 words or None).
    Still regions (pre_warp = gen + small noise) and unrelated regions alternate per gate window, so that windowed gates of
    both signs are neighbours; a single window is split into a still and an unrelated half."""
    h, w, window = case["h"], case["w"], case["window"]
    hh, ww, gh, gw, py, px = geometry(h, w, window)
    rng = np.random.default_rng(case["seed"])
    wide = case["kind"] != "plain"
    sums = sums_words(h, w, 0.3 if case["kind"] == "bright" else -0.2, rng) if case["kind"] in ("bright", "dark") else None
    b = brightness(sums, h * w)
    if gh * gw > 1:
        cy, cx = (np.arange(hh) + py) // window, (np.arange(ww) + px) // window
        unrelated = ((cy[:, None] + cx[None, :]) % 2 == 1)
    else:
        unrelated = np.broadcast_to(np.arange(ww)[None, :] >= (ww + 1) // 2, (hh, ww)).copy()
    g = rng.uniform(-0.46, 0.46, (hh, ww, 3))             # (the still noise stays inside the limit)
    if wide:                                             # 15 % of the pixels: the generator near an end of the range ...
        pushed = rng.random((hh, ww)) < 0.15
        sign = np.where(rng.random((hh, ww, 1)) < 0.5, -1.0, 1.0)
        g = np.where(pushed[..., None], sign * rng.uniform(0.3, 0.45, (hh, ww, 3)), g)
    state = np.zeros((hh, ww, 4), np.float16)
    state[..., :3] = (g - b).astype(np.float16)
    state[..., 3] = rng.uniform(-2, 2, (hh, ww)).astype(np.float16)
    gen = state[..., :3].astype(np.float64) + b
    # (still: noise of 0.01 .. 0.03 either way, never less -- a pixel's terms stay above 2^-14 in every mode, see the header)
    still = rng.uniform(0.01, 0.03, (hh, ww, 3)) * np.where(rng.random((hh, ww, 3)) < 0.5, -1.0, 1.0)
    amp = np.array([1.0, 0.6, 0.3])                      # the channels differ in size, so that the luma weights matter
    other = amp * rng.uniform(-0.5, 0.5, (hh, ww, 3))
    other = np.where(np.abs(other - gen) < 0.03 * amp, gen + np.where(other < gen, -0.03, 0.03) * amp, other)   # (the same floor)
    pw = np.where(unrelated[..., None], other, gen + amp * still)
    if wide:                                             # ... and pre_warp beyond it on the same side
        pw = np.where(pushed[..., None], sign * (0.5 + amp * rng.uniform(0.1, 1.0, (hh, ww, 3))), pw)
    pre = np.zeros((hh, ww, 4), np.float16)
    pre[..., :3] = pw.astype(np.float16)
    pre[..., 3] = rng.uniform(-2, 2, (hh, ww)).astype(np.float16)
    return dict(state=state, pre_warp=pre, sums=sums, b=b)


def window_sums(case, data, mode):
    """The gate statistic's per-window sums [GH, GW], without the gate: what the thresholds are chosen from."""
    p = data["pre_warp"][..., :3].astype(np.float64)
    if mode["limit"]:
        p = np.clip(p, -0.5, 0.5)
    t = data["state"][..., :3].astype(np.float64) + data["b"] - p
    t = t * t if mode["l2"] else np.abs(t)
    if mode["luma"]:
        k = O.BGR_LUMA * 3
        t = t * (k * k if mode["l2"] else k)
    _, _, gh, gw, _, _ = geometry(case["h"], case["w"], case["window"])
    idx = cell_index(case["h"], case["w"], case["window"]).ravel()
    return np.bincount(idx, t.sum(-1).ravel(), gh * gw).reshape(gh, gw)


def thresholds(case, data, mode):
    """The thresholds a mode of a case runs at, as f32 values.  Several cells: the middle of the widest gap of the cell
    means (below 1).  One cell: one threshold under its mean and one above (a hard gate: far; a tanh gate: 0.02 away, so
    that c is neither 1 nor -1)."""
    hh, ww, gh, gw, _, _ = geometry(case["h"], case["w"], case["window"])
    denom = 3.0 * hh * ww if case["window"] == 0 else 3.0 * case["window"] ** 2
    m = np.sort((window_sums(case, data, mode) / denom).ravel())
    if len(m) == 1:
        m = float(m[0])
        lo, hi = (m - 0.02, m + 0.02) if mode["gain"] else (m / 2, min(2 * m, (m + 1) / 2))
        if m - lo < 2.0 ** -11 or lo < 0:                # a small mean (a window far larger than the frame): 2^-10 away, or 0
            lo = max(m - 2.0 ** -10, 0.0)
        pair = (lo, max(hi, m + 2.0 ** -10)) if m - lo >= 2.0 ** -12 else (max(hi, m + 2.0 ** -10),)   # (no room under the mean)
        return [float(np.float32(t)) for t in pair]
    mids = 0.5 * (m[1:] + m[:-1])
    gaps = np.where(mids < 1.0, m[1:] - m[:-1], -1.0)
    return [float(np.float32(mids[int(np.argmax(gaps))]))]


def runs(case, data):
    """Every run of a case: the mode, strength, window and one of its thresholds.  With limit, strength 1 and a gate of
    -1 the result is the clamped pre_warp itself, exactly +-0.5 on every pixel that was out of range, and there byte(r - e)
    and byte(r + e) differ whatever e is: on data with such pixels the limit modes of a strength-1 case run at 0.5."""
    out = []
    for mode in case["modes"]:
        strength = 0.5 if mode["limit"] and case["kind"] != "plain" and case["strength"] == 1.0 else case["strength"]
        for thr in thresholds(case, data, mode):
            out.append(dict(mode, window=case["window"], strength=strength, threshold=thr))
    return out


def flags_of(run):
    return (FLAG_L2 if run["l2"] else 0) | (FLAG_LIMIT if run["limit"] else 0) | (FLAG_LUMA if run["luma"] else 0)
