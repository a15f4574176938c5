"""The temporal output filter without a GPU: the definition (tests/temporal_reference.py) against a per-pixel loop over
frame_moving_avg.py's graph; the conditions the GPU case table has to meet, on the definition alone; the sensitivity of
that table to subtly wrong kernels, written as mutants of a simulated kernel; the hook's refusals and its place among the
hooks."""

import ctypes as C
import math
import os
import re

import numpy as np

import temporal_reference as T
from helpers import O
from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 2.0 ** -12


# ---- 1. the definition against a per-pixel loop ---------------------------------------------------------------------------
def brute(gen, pre, run):
    """frame_moving_avg.py:156-302 node by node, one scalar at a time.  gen, pre: [HH, WW, 3] float64."""
    hh, ww, _ = gen.shape
    window, thr, gain, s = run["window"], float(np.float32(run["threshold"])), float(run["gain"]), float(run["strength"])
    luma = [3 * 0.1140, 3 * 0.5870, 3 * 0.2989]
    gain_coef = 1.0 if gain == 0 else gain
    p = [[[min(max(v, -0.5), 0.5) if run["limit"] else v for v in px] for px in row] for row in pre.tolist()]
    g = gen.tolist()
    diff = [[[0.0] * 3 for _ in range(ww)] for _ in range(hh)]
    for y in range(hh):
        for x in range(ww):
            for c in range(3):
                d = g[y][x][c] - p[y][x][c]
                diff[y][x][c] = d * d if run["l2"] else abs(d)

    def weight(c):
        k = 1.0
        if run["luma"]:
            k = luma[c] * luma[c] if run["l2"] else luma[c]
        return k

    def gate(v):                                        # Add(-threshold * gain_coef), then Sign or Tanh
        z = v - thr * gain_coef
        if gain == 0:
            return (z > 0) - (z < 0)
        return math.tanh(z)

    if window == 0:
        total = sum(diff[y][x][c] * weight(c) * gain_coef for y in range(hh) for x in range(ww) for c in range(3))
        cond = [[gate(total / (3 * hh * ww))] * ww for _ in range(hh)]
    else:
        oh, ow = (hh + window - 1) // window * window, (ww + window - 1) // window * window
        pad_y, pad_x = (oh - hh) // 2, (ow - ww) // 2    # [(x - y) // 2, x - y - (x - y) // 2]: the smaller part leads
        gh, gw = oh // window, ow // window
        cells = [[0.0] * gw for _ in range(gh)]
        for cy in range(gh):                             # Conv, strides = window, kernel = 1 / 3 / window / window
            for cx in range(gw):
                acc = 0.0
                for ky in range(window):
                    for kx in range(window):
                        y, x = cy * window + ky - pad_y, cx * window + kx - pad_x
                        if 0 <= y < hh and 0 <= x < ww:   # (zero padding)
                            for c in range(3):
                                acc += diff[y][x][c] * weight(c)
                cells[cy][cx] = gate(acc / 3 / window / window * gain_coef)
        cond = [[0.0] * ww for _ in range(hh)]
        for y in range(hh):                              # Resize linear / asymmetric by `window`, then Slice
            for x in range(ww):
                sy, sx = (y + pad_y) / window, (x + pad_x) / window
                y0, x0 = int(sy), int(sx)
                y1, x1 = min(y0 + 1, gh - 1), min(x0 + 1, gw - 1)
                fy, fx = sy - y0, sx - x0
                top = cells[y0][x0] + (cells[y0][x1] - cells[y0][x0]) * fx
                bot = cells[y1][x0] + (cells[y1][x1] - cells[y1][x0]) * fx
                cond[y][x] = top + (bot - top) * fy
    out = np.zeros((hh, ww, 3))
    for y in range(hh):
        for x in range(ww):
            m1 = cond[y][x] * (-s / 2) + s / 2
            m2 = cond[y][x] * (s / 2) + (1 - s / 2)
            for c in range(3):
                out[y, x, c] = p[y][x][c] * m1 + g[y][x][c] * m2
    return out, cond


def test_the_definition_equals_a_per_pixel_loop_over_the_reference_graph():
    for k, (h, w, window) in enumerate([(1, 1, 0), (1, 1, 3), (1, 1, 5), (2, 3, 5), (2, 3, 7), (3, 2, 7), (3, 5, 16), (3, 5, 3), (2, 2, 1),
                                        (2, 2, 24)]):
        case = dict(h=h, w=w, window=window, kind=T.KINDS[k % 4], seed=k, strength=T.STRENGTHS[k % 3], modes=T.MODES)
        data = T.build(case)
        for run in T.runs(case, data):
            d = T.define(data["state"], data["pre_warp"], data["sums"], h, w, run)
            want, cond = brute(d["gen"], data["pre_warp"][..., :3].astype(np.float64), run)
            assert np.abs(d["filtered"] - want).max() <= 1e-12, (case, run)
            # the second helper's gate, from the definition's own sums as integers, is the loop's gate too
            acc = np.floor(d["sums"].ravel() * T.SCALE + 0.5).astype(np.uint64)
            c = T.gate_from_acc(acc, h, w, run)[..., 0]
            assert np.abs(c - np.array(cond)).max() <= 1e-6, (case, run)
            assert np.allclose(d["sums"], T.window_sums(case, data, run), rtol=1e-12, atol=1e-15)


def test_the_byte_saturates_and_the_state_does_not():
    r = np.array([0.7, 0.525, 0.5, 0.4999, 0.0, -0.5, -0.52, -0.7])
    assert T.to_byte(r).tolist() == [255, 255, 255, 254, 127, 0, 0, 0]
    assert O.postprocess(r).tolist() == T.to_byte(r).tolist()
    lo, hi, slo, shi = T.intervals(np.array([0.25, 1.0]), 0.3, np.array([2.0 ** -20, 2.0 ** -20]))
    assert lo.tolist() == hi.tolist() == [191, 255]
    assert slo[0] < np.float16(-0.05) <= shi[0] and float(shi[1]) >= 0.7 + 2.0 ** -20 > float(slo[1])
    assert float(shi[0]) - float(slo[0]) <= 2 * 2.0 ** -15   # (two steps of f16 near 0.05 at the most)


# ---- 2. the conditions on the GPU case table -------------------------------------------------------------------------------
def claims(case, data, run):
    """What a run of the table says it exercises, by the rule of the table."""
    _, _, gh, gw, _, _ = T.geometry(case["h"], case["w"], case["window"])
    several, hard = gh * gw > 1, run["gain"] == 0
    out = set()
    if several and hard:
        out.add("both gate signs")
        if case["window"] > 1:
            out.add("interpolation between unlike cells")
    if case["kind"] != "plain" and case["h"] * case["w"] >= 15:      # (a 4 x 4 frame has two or three pixels out of range)
        if run["limit"]:
            out.add("limit changes the result")
        elif hard and case["window"] in (0, 16, 24, 64, 4096):         # (a gate of -1 gives pre_warp the whole strength; in a
            # window of a few pixels one pixel out of range is a scene cut by itself, and the generator's value passes)
            out.add("bytes saturate at both ends")
    if run["luma"]:
        out.add("luma changes the sums")
    return out


def test_every_case_meets_the_conditions_it_is_run_under():
    seen = set()
    n_runs = 0
    windows, pads = set(), set()
    for case in T.CASES:
        data = T.build(case)
        _, _, gh, gw, _, _ = T.geometry(case["h"], case["w"], case["window"])
        windows.add(case["window"])
        if case["window"]:
            pads.add((gh * case["window"] - 4 * case["h"], gw * case["window"] - 4 * case["w"], gh == 1, gw == 1))
        cut_seen = []
        for run in T.runs(case, data):
            n_runs += 1
            d = T.define(data["state"], data["pre_warp"], data["sums"], case["h"], case["w"], run)
            what = (case["name"], run)
            thr = float(np.float32(run["threshold"]))
            assert 0.0 <= thr <= 1.0, what
            assert np.abs(d["mean"] - thr).min() >= MARGIN, what
            acc = np.floor(d["sums"].ravel() * T.SCALE + 0.5).astype(np.uint64)
            hard_cut = T.is_hard_cut(acc, case["h"], case["w"], run)
            cut_seen.append(bool(hard_cut))
            c = T.gate_from_acc(acc, case["h"], case["w"], run)
            r = T.blend(d, c, run)
            assert np.abs(r - d["filtered"]).max() <= 1e-9, what     # the helper's blend is the definition's
            e = T.error_bound(d, r, case["h"], case["w"], run, data["sums"] is not None)
            assert e.max() <= 2.0 ** -16, what                        # far below a step of the byte or of f16 near 1
            lo, hi, _, _ = T.intervals(r, d["b"], e)
            assert np.mean(lo != hi) <= 0.01, what
            got = claims(case, data, run)
            seen |= got
            cells = T.gate_cells(acc, d["denom"], run)
            raw = (d["filtered"] + 0.5) * 255
            if "both gate signs" in got:
                assert (cells > 0).any() and (cells < 0).any(), what
            if "interpolation between unlike cells" in got:
                assert ((c > -1) & (c < 1)).any(), what
            through = run["gain"] == 0 and (cells > 0).all()         # every gate says "cut": the generator's output passes through
            if "bytes saturate at both ends" in got and not through:
                assert (raw >= 256).any() and (raw < 0).any(), what
            if "limit changes the result" in got and not through:
                other = T.define(data["state"], data["pre_warp"], data["sums"], case["h"], case["w"], dict(run, limit=0))
                assert not np.array_equal(other["byte"], d["byte"]), what
            if "luma changes the sums" in got:
                plain = T.window_sums(case, data, dict(run, luma=0))
                assert (np.abs(plain - d["sums"]) > 10 * T.reduce_tolerance(d, data["sums"] is not None)).any(), what
        if case["window"] == 0 and any(m["gain"] == 0 for m in case["modes"]):
            assert True in cut_seen and False in cut_seen, case["name"]      # the hard cut and its opposite
    assert seen == {"both gate signs", "interpolation between unlike cells", "bytes saturate at both ends",
                    "limit changes the result", "luma changes the sums"}
    assert windows >= {0, 1, 3, 5, 7, 16, 24, 64, 4096}
    assert any(p[:2] == (0, 0) for p in pads)                                 # no padding
    assert any(p[0] % 2 == 0 and p[0] > 0 for p in pads) and any(p[1] % 2 == 0 and p[1] > 0 for p in pads)   # even
    assert any(p[0] % 2 == 1 for p in pads) and any(p[1] % 2 == 1 for p in pads)                              # odd, each axis
    assert any(p[2] and not p[3] for p in pads) and any(p[3] and not p[2] for p in pads)                      # GH = 1, GW = 1 alone
    assert {c["strength"] for c in T.CASES} == {0.25, 0.5, 1.0} and {c["layout"] for c in T.CASES} == set(T.LAYOUTS)
    big = T.BIG
    assert big["h"] * big["w"] > 131072 and 16 * big["h"] * big["w"] > 2048 * 256 and len(big["modes"]) == 1 and big["window"] == 0
    assert n_runs >= 400


# ---- 3. sensitivity: mutants of a simulated kernel ----------------------------------------------------------------------------
MUTANTS = ["pad trailing first", "divisor by the real area", "neighbour not clamped", "luma B and R swapped", "luma once under L2",
           "limit in the blend only", "limit in the gate only", "byte wrapped", "no brightness in the gate", "last partial wave dropped"]
REDUCE_MUTANTS = {"luma B and R swapped", "luma once under L2", "no brightness in the gate", "last partial wave dropped"}


def simulate(case, data, run, mutant=None):
    """The three kernels in float64 with exact roundings at the end (acc: 32.32; byte; f16): (acc, out, state)."""
    h, w, window = case["h"], case["w"], run["window"]
    hh, ww, gh, gw, py, px = T.geometry(h, w, window)
    if mutant == "pad trailing first" and window:
        py, px = gh * window - hh - py, gw * window - ww - px
    b = data["b"]
    st = data["state"][..., :3].astype(np.float64)
    pre = data["pre_warp"][..., :3].astype(np.float64)
    gen = st + b
    limited = np.clip(pre, -0.5, 0.5)
    p_gate = limited if run["limit"] and mutant != "limit in the blend only" else pre
    p_blend = limited if run["limit"] and mutant != "limit in the gate only" else pre
    t = (st if mutant == "no brightness in the gate" else gen) - p_gate
    t = t * t if run["l2"] else np.abs(t)
    if run["luma"]:
        k = O.BGR_LUMA * 3
        if mutant == "luma B and R swapped":
            k = k[::-1]
        t = t * (k * k if run["l2"] and mutant != "luma once under L2" else k)
    per_pixel = t.sum(-1).ravel()
    if mutant == "last partial wave dropped" and per_pixel.size % 64:
        per_pixel[per_pixel.size // 64 * 64:] = 0.0
    if window:
        idx = (((np.arange(hh) + py) // window)[:, None] * gw + ((np.arange(ww) + px) // window)[None, :]).ravel()
    else:
        idx = np.zeros(hh * ww, np.int64)
    acc = np.floor(np.bincount(idx, per_pixel, gh * gw) * T.SCALE + 0.5).astype(np.uint64)
    denom = np.full(gh * gw, 3.0 * hh * ww if window == 0 else 3.0 * window * window)
    if mutant == "divisor by the real area" and window:
        denom = 3.0 * np.maximum(np.bincount(idx, minlength=gh * gw), 1)
    cells = T.gate_cells(acc, denom, run).reshape(gh, gw)
    if window:
        if mutant == "neighbour not clamped":            # the cell behind the last one: a sum of 0
            outside = T.gate_cells(np.zeros(1, np.uint64), denom[:1], run)[0]
            cells = np.pad(cells, ((0, 1), (0, 1)), constant_values=outside)
        y0, y1, fy = T.resize_axis(hh, py, window, cells.shape[0])
        x0, x1, fx = T.resize_axis(ww, px, window, cells.shape[1])
        fy, fx = fy[:, None], fx[None, :]
        top = cells[y0][:, x0] + (cells[y0][:, x1] - cells[y0][:, x0]) * fx
        bot = cells[y1][:, x0] + (cells[y1][:, x1] - cells[y1][:, x0]) * fx
        c = (top + (bot - top) * fy)[..., None]
    else:
        c = np.full((hh, ww, 1), cells[0, 0])
    out = np.full((hh, ww, 4), 0x5A, np.uint8)
    state = data["state"].copy()
    if window == 0 and run["gain"] == 0 and cells[0, 0] > 0:
        return acc, out, state, out.copy()
    half = float(run["strength"]) / 2
    r = p_blend * (half - c * half) + gen * (c * half + 1 - half)
    if mutant == "byte wrapped":
        out[..., :3] = (np.trunc((r + 0.5) * 255).astype(np.int64) & 0xFF).astype(np.uint8)
    else:
        out[..., :3] = T.to_byte(r)
    out[..., 3] = 0
    state[..., :3] = (r - b).astype(np.float16)
    state[..., 3] = 0
    return acc, out, state, np.full((hh, ww, 4), 0x5A, np.uint8)


def test_the_table_catches_every_mutant_and_passes_the_faithful_kernel():
    caught = {m: [] for m in MUTANTS}
    for case in T.CASES:
        data = T.build(case)
        for run in T.runs(case, data):
            d = T.define(data["state"], data["pre_warp"], data["sums"], case["h"], case["w"], run)
            acc, out, state, before = simulate(case, data, run)
            fails, fig = T.check_run(case, data, d, run, acc, out, state, before)
            assert not fails, (case["name"], run, fails)
            assert fig["acc_dev_over_tol"] <= 0.125                # (the definition's sums, a fixed-point step per pixel apart)
            if case is T.BIG or case is T.HUGE_WINDOW:
                continue
            for m in MUTANTS:
                if len(caught[m]) >= 3:                            # (three witnesses each are enough to name)
                    continue
                acc, out, state, before = simulate(case, data, run, m)
                fails, _ = T.check_run(case, data, d, run, acc, out, state, before)
                if m in REDUCE_MUTANTS:
                    fails = [f for f in fails if f.startswith("reduce")]      # these are the accumulator tolerance's to catch
                if fails:
                    caught[m].append((case["name"], fails[0][:60]))
    assert all(caught[m] for m in MUTANTS), {m: v for m, v in caught.items() if not v}


# ---- 4. the hook ----------------------------------------------------------------------------------------------------------------
def refusal(lib, **kw):
    a = dict(state=0x1000, pre_warp=0x2000, out=0x3000, stride=64, sums=None, width=4, height=4, strength=0.5, threshold=0.1,
             gain=0.0, window=0, flags=0, acc=None, capacity=0)
    a.update(kw)
    rc = lib.ju_debug_temporal(a["state"], a["pre_warp"], a["out"], a["stride"], a["sums"], a["width"], a["height"], a["strength"],
                               a["threshold"], a["gain"], a["window"], a["flags"], a["acc"], a["capacity"])
    return rc, lib.ju_last_error().decode() if rc else ""


def test_the_hook_refuses_bad_arguments_before_any_device_call(hip_library):
    words = (C.c_uint64 * 4)()
    loader = {"strength": "temporal filter strength/threshold must be in [0, 1]",
              "threshold": "temporal filter strength/threshold must be in [0, 1]",
              "window": "temporal filter window must be in 0..4096", "gain": "temporal filter gain must be in [0, 1e6]"}
    cases = [(dict(state=None), "null buffer"), (dict(pre_warp=None), "null buffer"), (dict(out=None), "null buffer"),
             (dict(state=0x1004), "8-byte aligned"), (dict(pre_warp=0x2002), "8-byte aligned"),
             (dict(out=0x3002), "multiples of 4"), (dict(stride=66), "multiples of 4"), (dict(stride=-62), "multiples of 4"),
             (dict(sums=0x4002), "multiples of 4"),
             (dict(width=0), "1 .. 8192"), (dict(height=0), "1 .. 8192"), (dict(width=8193), "1 .. 8192"), (dict(height=1 << 40), "1 .. 8192"),
             (dict(strength=1.5), loader["strength"]), (dict(strength=-0.1), loader["strength"]),
             (dict(strength=float("nan")), loader["strength"]), (dict(threshold=1.01), loader["threshold"]),
             (dict(threshold=-1.0), loader["threshold"]), (dict(window=-1), loader["window"]), (dict(window=4097), loader["window"]),
             (dict(gain=-1.0), loader["gain"]), (dict(gain=2e6), loader["gain"]), (dict(gain=float("nan")), loader["gain"]),
             (dict(flags=8), "unknown temporal flag bits"), (dict(flags=0x80000001), "unknown temporal flag bits"),
             (dict(acc=words, capacity=0), "capacity"), (dict(acc=None, capacity=4), "capacity"),
             (dict(acc=words, capacity=3, window=2), "capacity")]        # 4 x 4 LR at window 2: 8 x 8 cells
    for kw, text in cases:
        rc, msg = refusal(hip_library, **kw)
        assert rc == 1 and msg.startswith("std::invalid_argument: ju_debug_temporal: ") and text in msg, (kw, rc, msg)
    model_cpp = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "model.cpp")).read()
    for text in set(loader.values()):
        assert '"' + text + '"' in model_cpp                         # the loader's wording


def test_the_hook_is_a_hook_and_nothing_the_product_exports(hip_library, product_library):
    header = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    assert re.search(r"JU_API\s+int\s+ju_debug_temporal\s*\(", test_header) and "ju_debug_temporal" not in header
    assert "ju_debug_temporal" in R.HOOK_SYMBOLS and "ju_debug_temporal" not in R.PRODUCT_SYMBOLS
    assert hasattr(hip_library, "ju_debug_temporal") and not hasattr(product_library, "ju_debug_temporal")
    assert (T.FLAG_L2, T.FLAG_LIMIT, T.FLAG_LUMA) == (1, 2, 4)
