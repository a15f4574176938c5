"""The exact tests without a GPU (docs/exact_tests.md): the definitions (tests/exact_reference.py) against the oracle's
float64 primitives on dyadic inputs; the rounding against hand-made cases; every case of the GPU tables
(tests/exact_cases.py) held to the dyadic condition -- a table that would test inexact arithmetic fails here; what the
tables cover; the hooks' refusals and their place among the hooks."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import exact_cases as K
import exact_reference as E
from helpers import O
from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the definitions against the oracle ---------------------------------------------------------------------------------------
def test_the_convolution_is_the_oracles_on_dyadic_inputs():
    rng = np.random.default_rng(1)
    for taps, cin, cout, h, w in [(9, 16, 32, 5, 7), (1, 32, 32, 3, 4), (9, 64, 32, 2, 2)]:
        x = rng.integers(-8, 9, (h, w, cin)).astype(np.float64)
        wt = rng.integers(-2, 3, (taps, cin, cout)).astype(np.float64)
        bias = rng.integers(-4, 5, cout).astype(np.float64)
        k = 3 if taps == 9 else 1
        want = O.conv2d_same(x, wt.reshape(k, k, cin, cout), bias)
        for act, f in ((0, lambda v: v), (1, O.relu), (2, lambda v: O.leaky_relu(v, 0.25))):
            got = E.conv(x, wt, bias, taps, act, 0.25, dtype=E.BF16)
            assert np.array_equal(got["exact"], f(want))
            res = rng.integers(-8, 9, (h, w, cout)).astype(np.float64)
            assert np.array_equal(E.conv(x, wt, bias, taps, act, 0.25, res=res, dtype=E.F16)["exact"], f(want + res))
        if h % 2 == 0 and w % 2 == 0:
            assert np.array_equal(E.conv(x, wt, bias, taps, 1, pool=True, dtype=E.F16)["exact"], O.max_pool_2x2(O.relu(want)))


def test_resampling_is_the_oracles():
    rng = np.random.default_rng(2)
    for h, w in [(1, 1), (2, 2), (5, 7), (6, 10)]:
        x = rng.integers(-255, 256, (h, w, 8)).astype(np.float64)
        assert np.array_equal(E.upsample2_exact(x), O.resize_bilinear_tf1(x, 2))
        if h % 2 == 0:
            assert np.array_equal(E.maxpool2(x, E.BF16)[1], O.max_pool_2x2(x))
    # the fused expansion: the oracle's upsampling, rounded to T, then the oracle's convolution
    x = rng.integers(-255, 256, (3, 4, 64)).astype(np.float64)
    wt = rng.integers(-1, 2, (9, 64, 32)).astype(np.float64)
    up = E.to_float(E.rne(O.resize_bilinear_tf1(x, 2), E.BF16), E.BF16)
    assert not np.array_equal(up, O.resize_bilinear_tf1(x, 2))                 # (it rounds)
    got = E.conv(x, wt, np.zeros(32), 9, 0, upsample=True, dtype=E.BF16)
    assert np.array_equal(got["exact"], O.conv2d_same(up, wt.reshape(3, 3, 64, 32)))


def test_the_flow_block_is_two_convolutions_with_the_intermediate_in_t():
    rng = np.random.default_rng(3)
    x = rng.integers(-4, 5, (5, 7, 64)).astype(np.float64)
    w1, w2 = (rng.integers(-2, 3, (9, 64, 64)).astype(np.float64) for _ in range(2))
    b1, b2 = (rng.integers(-4, 5, 64).astype(np.float64) for _ in range(2))
    got = E.flow_block(x, w1, b1, w2, b2, 2, 2, 0.25, residual=True, dtype=E.BF16)
    mid = O.leaky_relu(O.conv2d_same(x, w1.reshape(3, 3, 64, 64), b1), 0.25)
    mid_t = E.to_float(E.rne(mid, E.BF16), E.BF16)
    assert not np.array_equal(mid_t, mid)
    assert np.array_equal(got["exact"], O.leaky_relu(O.conv2d_same(mid_t, w2.reshape(3, 3, 64, 64), b2) + x, 0.25))


def test_the_warp_is_the_oracles_dense_image_warp():
    for case in K.WARP_CASES:
        d, ref = K.warp_reference(case, E.BF16)
        H, W = case["H"], case["W"]
        want = O.dense_image_warp(d["state"][..., :3], d["field"])
        assert np.array_equal(ref["exact"], want), case["name"]
        # the records: slot i * 16 + j * 3 + c = HR pixel (4 h + i, 4 w + j), 12 .. 14 of quarter 0 the LR pixel, else 0
        rec = ref["records"].reshape(H, W, 4, 16)
        hr = E.rne(want, E.BF16).reshape(H, 4, W, 4, 3).transpose(0, 2, 1, 3, 4).reshape(H, W, 4, 12)
        assert np.array_equal(rec[..., :12], hr)
        assert not rec[:, :, 1:, 12:].any() and not rec[:, :, 0, 15].any()
        lr = E.rne_any(O.preprocess(d["frame"][..., :3]), E.BF16)
        assert np.array_equal(rec[:, :, 0, 12:15], lr)
        assert np.array_equal(ref["bgrx"][..., :3], O.postprocess(E.to_float(E.rne(want, E.BF16), E.BF16).astype(np.float32)))
        assert not ref["bgrx"][..., 3].any() and not ref["pre_warp"][..., 3].any()


def test_the_lr_slots_accept_two_words_at_one_byte_in_bf16_and_none_in_f16():
    w, alt = E.lr_slot_table(E.BF16)
    assert np.flatnonzero(w != alt).size == 1
    w, alt = E.lr_slot_table(E.F16)
    assert np.array_equal(w, alt)
    assert E.to_float(w[[0, 255]], E.F16).tolist() == [-0.5, 0.5]


# ---- 2. the rounding ------------------------------------------------------------------------------------------------------------
def test_rne_on_hand_made_cases():
    bf = lambda v: E.to_float(E.rne(np.array(v, np.float64), E.BF16), E.BF16).tolist()
    fh = lambda v: E.to_float(E.rne(np.array(v, np.float64), E.F16), E.F16).tolist()
    # bf16 holds 8 significant bits: 257 is the first integer it cannot, and the ties go to the even neighbour both ways
    assert bf([256, 257, 258, 259, 260, 261, 263]) == [256, 256, 258, 260, 260, 260, 264]
    assert bf([-257, -259, 257.5, 258.875, 1.00390625, 1.01171875]) == [-256, -260, 258, 258, 1.0, 1.015625]
    # f16 holds 11: 2049 is the first
    assert fh([2048, 2049, 2050, 2051, 2053, -2049, -2051, 0.25, 2049.5]) == [2048, 2048, 2050, 2052, 2052, -2048, -2052, 0.25, 2050]
    assert E.rne(np.array([0.0, -0.0, 1.0, -2.0]), E.BF16).tolist() == [0, 0x8000, 0x3F80, 0xC000]
    assert E.rne(np.array([0.0, -0.0, 1.0, -2.0]), E.F16).tolist() == [0, 0x8000, 0x3C00, 0xC000]
    assert E.fold_zero(np.array([0x8000, 0, 0x8001], np.uint16))[0].tolist() == [0, 0, 0x8001]
    # both roundings of arbitrary float64 agree with the bit formula wherever f32 holds the value
    v = np.random.default_rng(4).integers(-2 ** 20, 2 ** 20, 4096) / 64.0
    for dt in K.DTYPES:
        assert np.array_equal(E.rne_any(v, dt), E.rne(v, dt))
    assert E.rounding_counts(np.array([256.0, 257.0, 258.5, 259.0]), E.BF16) == (3, 2)
    with pytest.raises(E.NotDyadic):
        E.rne(np.array([0.1]), E.BF16)                                          # (f32 does not hold it)
    with pytest.raises(E.NotDyadic):
        E.rne(np.array([65520.0]), E.F16)


def test_the_condition_refuses_what_is_not_dyadic():
    x = np.full((4, 4, 64), 8.0)
    w = np.full((9, 64, 32), 2.0)
    assert E.conv(x, w, np.zeros(32), dtype=E.BF16)["budget_bits"] < 14
    with pytest.raises(E.NotDyadic):
        E.conv(x * 128, w, np.zeros(32), dtype=E.BF16)                          # 576 x 2048 = 2^20.2
    with pytest.raises(E.NotDyadic):
        E.conv(x + 0.001, w, np.zeros(32), dtype=E.BF16)                        # T does not hold the input
    with pytest.raises(E.NotDyadic):
        E.conv(x, w, np.full(32, 0.5), dtype=E.BF16)                            # a bias finer than the products
    with pytest.raises(E.NotDyadic):
        E.conv(np.full((4, 4, 64), 128.0), np.full((9, 64, 32), 64.0), np.zeros(32), act=0, dtype=E.F16)   # beyond 65504
    st = np.zeros((8, 8, 4))
    fl = np.zeros((2, 2, 32))
    fr = np.zeros((2, 2, 4), np.uint8)
    E.warp(st, fl, fr, 2, 2, 2, 0, 0, E.F16)
    with pytest.raises(E.NotDyadic):
        E.warp(st, fl + 1 / 16, fr, 2, 2, 2, 0, 0, E.F16)
    with pytest.raises(E.NotDyadic):
        E.warp(st + 0.75, fl, fr, 2, 2, 2, 0, 0, E.F16)


# ---- 3. the case tables -----------------------------------------------------------------------------------------------------------
def counts(refs):
    c = t = 0
    for r in refs:
        a, b = E.rounding_counts(r["exact"], r["out_type"])
        c, t = c + a, t + b
    return c, t


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_NAMES.get)
def test_every_convolution_case_is_dyadic(dtype):
    worst = 0.0
    for case in K.CONV_CASES + K.SPLITK_CASES + K.TOWER_CASES:
        c = t = 0
        for si in range(len(case["shapes"])):
            _, refs = K.conv_reference(case, si, K.act_of(case, si), dtype)    # (raises NotDyadic)
            worst = max(worst, max(r["budget_bits"] for r in refs))
            a, b = counts(refs)
            c, t = c + a, t + b
        if dtype in case["rounds"]:
            assert c > 0 and t > 0, (case["name"], c, t)
    assert worst < E.BUDGET_BITS


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_NAMES.get)
def test_every_flow_block_case_is_dyadic(dtype):
    for case in K.FB_CASES:
        c = t = 0
        for k, (th, shape, items) in enumerate(K.fb_runs(case)):
            _, refs = K.fb_reference(case, shape, items, case["acts"][k % len(case["acts"])], dtype)
            assert max(max(r["budget_a"], r["budget_b"]) for r in refs) < E.BUDGET_BITS
            a, b = counts(refs)
            c, t = c + a, t + b
            if case["wide"] and dtype == E.BF16:                                # the expanded tile itself rounds in T
                x = K.fb_inputs(case, shape, items, case["acts"][k % len(case["acts"])])["x"][0]
                assert E.rounding_counts(E.upsample2_exact(x), dtype)[0] > 0
        if dtype in case["rounds"]:
            assert c > 0 and t > 0, (case["name"], c, t)


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.DTYPE_NAMES.get)
def test_every_resample_and_warp_case_is_dyadic(dtype):
    for case in K.RESAMPLE_CASES:
        c = t = 0
        for size in case["sizes"]:
            _, outs = K.resample_reference(case, size, dtype)
            a, b = counts([dict(exact=o[1], out_type=dtype) for o in outs])
            c, t = c + a, t + b
        if dtype in case["rounds"]:
            assert c > 0 and t > 0, case["name"]
    for case in K.WARP_CASES:
        d, ref = K.warp_reference(case, dtype)
        if case["field"] == "fractions":
            assert min(E.rounding_counts(ref["exact"], dtype)) > 0 and min(E.rounding_counts(ref["exact"], E.F16)) > 0


def test_the_tables_cover_what_they_claim():
    conv = K.CONV_CASES
    has = lambda cases, **kw: any(all(c[k] == v for k, v in kw.items()) for c in cases)
    for taps, cin in [(9, 64), (9, 32), (9, 16), (1, 64), (1, 32)]:
        for nb in (1, 2):
            for rw in (1, 2):
                assert has(conv, taps=taps, cin=cin, nb=nb, rw=rw)
    assert any(c["res"] and c["res_pad"] for c in conv) and has(conv, out_head=True) and has(conv, pool=True, rw=2)
    for cin in (64, 128):
        for rw in (1, 2):
            assert has(conv, upsample=True, cin=cin, rw=rw)
    for cin in (128, 256):
        for stages in (0, 1, 2):
            assert has(conv, cin=cin, nb=1, plan=dict(conv_stages=stages))
    assert {c["items"] for c in conv} >= {1, 3, 8} and all(c["gap"] > 0 for c in conv if c["items"] > 1)
    assert any(c["in_pad"] and c["out_pad"] for c in conv) and any(not c["in_pad"] and not c["out_pad"] for c in conv)
    assert has(conv, cin=16, cin_real=12)
    assert sum(c["amp"] == 255 and c["upsample"] for c in conv) >= 1
    sk = K.SPLITK_CASES
    for cin in (128, 256):
        for cout in (32, 128, 256):
            assert has(sk, cin=cin, cout=cout)
    assert has(sk, cin=128, pool=True) and {c["items"] for c in sk} >= {1, 8}
    rows = {c["plan"].get("splitk_rows") for c in sk if c["shapes"] == [(35, 34)]}
    assert rows == {2, 6, 16, 18, 34}
    assert {c["plan"].get("splitk_blocks") for c in sk} >= {1, 2}
    tw = K.TOWER_CASES
    assert {c["res"] for c in tw} == {False, True} and all(c["shapes"] == [(2, 2), (9, 33), (16, 64)] and c["acts"] == (1, 2) for c in tw)
    fb = K.FB_CASES
    for cin, cmid, ups, pool, kind, heights in K.FB_SHAPES:
        mine = [c for c in fb if (c["cin"], c["cmid"], c["upsample"], c["pool"], c["out_head"], c["residual"]) ==
                (cin, cmid, ups, pool, kind == 1, kind == 2)]
        assert mine and any(set(c["heights"]) == set(heights) for c in mine)
        assert any(items == 3 for c in mine for _, _, items in K.fb_runs(c)) or kind == 2
        if ups:
            assert any(c["wide"] for c in mine)
    assert {(c["form"], c["tower"]) for c in fb if c["residual"]} == {(f, t) for f in ("res_block_pipe", "res_block", "flow_block")
                                                                       for t in (False, True)}
    assert all(c["amp"] == 4 for c in fb if c["residual"])
    # the launcher's table and the kernels' tile constants are what this file's are
    src = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "flow_kernels.hip")).read()
    table = re.findall(r"^\tJU_FB_CASE\((\d+), (\d+), (true|false), (true|false), (\d)\)", src, flags=re.M)
    assert [(int(a), int(b), c == "true", d == "true", int(e)) for a, b, c, d, e in table] == [s[:5] for s in K.FB_SHAPES]
    assert re.search(r"constexpr int kFbMid = 14;", src)
    common = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "flow_block_common.h")).read()
    assert re.search(r"constexpr int kFbOutW = %d;" % K.FB_TW, common)
    # shapes: 2 x 2, below a tile with odd sizes, a tile and one more, two tiles
    assert K.shapes_for(32, 8, False) == [(2, 2), (3, 7), (9, 33), (16, 64)] and K.shapes_for(30, 14, False)[2:] == [(15, 31), (28, 60)]
    assert all(h % 2 == 0 and w % 2 == 0 for th in (2, 4, 6, 8, 20) for h, w in K.shapes_for(30, th, True))
    rs = K.RESAMPLE_CASES
    assert {(c["op"], c["C"], c["items"]) for c in rs} >= {(0, 32, 1), (0, 32, 3), (0, 256, 1), (0, 256, 3), (1, 32, 1), (1, 256, 1)}
    wp = K.WARP_CASES
    assert {(c["H"], c["W"]) for c in wp} == set(K.WARP_SIZES) and {c["field"] for c in wp} == set(K.WARP_FIELDS)
    for size in K.WARP_SIZES:
        mine = [c for c in wp if (c["H"], c["W"]) == size]
        assert {c["pads"] for c in mine} == {(0, 0), (3, 5)} and {c["tower_pitch"] for c in mine} == {False, True}
        assert {c["pre_warp"] for c in mine} == {False, True} and any(c["out_u8"] is None for c in mine)
    u8 = [c["out_u8"] for c in wp if c["out_u8"] is not None]
    align = lambda pad, off: min((16 * 2 + pad) & -(16 * 2 + pad), off & -off if off else 16, 16)    # (of every row, W = 2)
    assert {align(p, o) for p, o, _ in u8} == {16, 8, 4} and any(f for _, _, f in u8)
    assert any(c["pw_extra"] > 0 for c in wp)
    big = K.warp_inputs(next(c for c in wp if c["H"] == 17))
    assert set(big["frame"][..., :3].ravel().tolist()) == set(range(256))
    st = np.abs(big["state"])
    assert 0.05 < np.mean(st == 0.5) < 0.4


def test_the_warp_fields_reach_what_they_are_named_for():
    for case in K.WARP_CASES:
        d = K.warp_inputs(case)
        hh, ww = 4 * case["H"], 4 * case["W"]
        gy, gx = np.meshgrid(np.arange(hh), np.arange(ww), indexing="ij")
        qy, qx = gy - d["field"][..., 0], gx - d["field"][..., 1]
        if case["field"] == "corners-and-beyond" and case["H"] > 2:
            for ty, tx in [(0, 0), (hh - 1, ww - 1), (0, ww - 1), (hh - 1, 0)]:
                assert ((qy == ty) & (qx == tx)).any()
            assert (qy < 0).any() and (qy > hh - 1).any() and (qx < 0).any() and (qx > ww - 1).any()
        if case["field"] == "last-rows-and-columns" and case["H"] > 2:
            assert {hh - 2, hh - 1} <= set(qy.ravel().tolist()) and {ww - 2, ww - 1} <= set(qx.ravel().tolist())
        if case["field"].startswith("far"):
            amp = float(case["field"].split("-")[1])
            assert np.abs(d["field"]).min() >= amp - 1 and (d["field"] > 0).any() and (d["field"] < 0).any()


# ---- 4. the reference bites: the faults the GPU comparison has to catch ---------------------------------------------------------
def test_the_tables_tell_the_faulty_definitions_from_the_right_ones():
    # a neighbour that is not clamped, a clamp to size - 1, a rounding half away from zero: each changes words of the table
    case = next(c for c in K.CONV_CASES if c["name"] == "conv-ups-c64-rw1")
    d, refs = K.conv_reference(case, 1, K.act_of(case, 1), E.BF16)
    wrong = E.conv(d["x"][0], d["w"], d["bias"], 9, K.act_of(case, 1), K.SLOPE, upsample=True, dtype=E.BF16, clamp=False)
    assert not np.array_equal(wrong["words"], refs[0]["words"])
    wcase = next(c for c in K.WARP_CASES if c["field"] == "last-rows-and-columns" and c["H"] == 3)
    _, right = K.warp_reference(wcase, E.F16)
    _, wrong = K.warp_reference(wcase, E.F16, clamp_to=1)
    assert not np.array_equal(right["records"], wrong["records"])
    v = refs[0]["exact"]
    away = E.to_float(E.rne(v, E.BF16), E.BF16)
    assert E.rounding_counts(v, E.BF16)[1] > 0 and np.array_equal(E.rne(away, E.BF16), refs[0]["words"])


# ---- 5. the hooks -----------------------------------------------------------------------------------------------------------------
HOOKS = ("ju_debug_conv", "ju_debug_flow_block", "ju_debug_resample", "ju_debug_warp")


def test_the_hooks_are_hooks_and_nothing_the_product_exports(hip_library, product_library):
    header = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    for name in HOOKS:
        assert re.search(r"JU_API\s+int\s+%s\s*\(" % name, test_header) and name not in header
        assert name in R.HOOK_SYMBOLS and name not in R.PRODUCT_SYMBOLS
        assert hasattr(hip_library, name) and not hasattr(product_library, name)
    # the structs are the header's: field for field, in order
    for struct, cls in (("ju_debug_plan", R.JuDebugPlan), ("ju_debug_conv_args", R.JuDebugConv), ("ju_debug_flow_block_args", R.JuDebugFlowBlock),
                        ("ju_debug_resample_args", R.JuDebugResample), ("ju_debug_warp_args", R.JuDebugWarp)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), test_header, flags=re.S).group(1)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)\s*(?:,|$)", re.sub(r"^\s*(const\s+)?(\w+\s+)+?(?=\*?\w+\s*(,|$))", "", decl.strip()))]
        mine = [("in" if n == "inp" else n) for n, _ in cls._fields_]
        assert names == mine, (struct, names, mine)


def conv_args(**kw):
    w = np.zeros(9 * 64 * 64, np.float32)
    a = R.JuDebugConv()
    a.kernel, a.dtype, a.inp, a.out, a.res = 0, E.BF16, 0x10000, 0x20000, None
    a.H, a.W, a.cin, a.cin_real, a.cout, a.taps, a.relu, a.slope = 4, 4, 64, 64, 64, 9, 1, 0.25
    a.nb, a.rw, a.items = 1, 1, 1
    a.plan = R.JuDebugPlan(0, 0, -1, 0, 0, 0, 0)
    a._keep = w
    a.weights = a.bias = w.ctypes.data
    for k, v in kw.items():
        if k.startswith("plan_") and k not in ("plan_text", "plan_capacity"):
            setattr(a.plan, k[5:], v)
        else:
            setattr(a, k, v)
    return a


def refused(lib, fn, args, hook):
    rc = getattr(lib, fn)(C.byref(args)) if args is not None else getattr(lib, fn)(None)
    msg = lib.ju_last_error().decode() if rc else ""
    assert rc == 1 and msg.startswith("std::invalid_argument: %s: " % hook), (rc, msg)
    return msg


def test_the_conv_hook_refuses_bad_arguments_before_any_device_call(hip_library):
    lib = hip_library
    assert "null arguments" in refused(lib, "ju_debug_conv", None, "ju_debug_conv")
    text = C.create_string_buffer(16)
    cases = [(dict(dtype=2), "dtype"), (dict(kernel=3), "kernel must be"), (dict(inp=None), "null buffer"), (dict(out=None), "null buffer"),
             (dict(weights=None), "null buffer"), (dict(bias=None), "null buffer"), (dict(inp=0x10008), "16-byte aligned"),
             (dict(res=0x30002), "16-byte aligned"), (dict(H=0), "1 .. 4096"), (dict(W=4097), "1 .. 4096"), (dict(cin_real=65), "cin_real"),
             (dict(cin_real=0), "cin_real"), (dict(relu=3), "activation"), (dict(relu=2, slope=1.5), "slope"),
             (dict(relu=2, slope=float("nan")), "slope"), (dict(items=0), "items"), (dict(items=9), "items"),
             (dict(cin=24, cin_real=24), "multiple of 16"), (dict(cout=48), "multiple of 16"), (dict(nb=3), "multiple of 16"),
             (dict(rw=0), "multiple of 16"), (dict(nb=2, cout=96), "multiple of 16"), (dict(taps=3), "unsupported shape"),
             (dict(taps=1, cin=16, cin_real=16), "unsupported shape"), (dict(pool=1), "fused max-pool"), (dict(pool=1, rw=2, H=5), "fused max-pool"),
             (dict(pool=1, rw=2, res=0x30000), "fused max-pool"), (dict(pool=1, rw=2, out_head=1), "fused max-pool"),
             (dict(upsample=1, nb=2), "fused upsampling"), (dict(upsample=1, W=5), "fused upsampling"),
             (dict(upsample=1, cin=32, cin_real=32), "fused upsampling"), (dict(upsample=1, taps=1), "fused upsampling"),
             (dict(items=2, res=0x30000, in_item_bytes=4096, out_item_bytes=4096), "takes no residual"),
             (dict(in_pitch=3), "input pitch"), (dict(out_pitch=2), "output pitch"), (dict(res_pitch=1, res=0x30000), "residual pitch"),
             (dict(pool=1, rw=2, out_pitch=1), "output pitch"), (dict(items=2, in_item_bytes=2047, out_item_bytes=2048), "input item stride"),
             (dict(items=2, in_item_bytes=2048, out_item_bytes=2040), "output item stride"),
             (dict(items=2, in_item_bytes=2056, out_item_bytes=2048), "input item stride"),
             (dict(plan_conv_stages=3), "plan field"), (dict(plan_splitk_rows=-2), "plan field"), (dict(plan_res_block=3), "plan field"),
             (dict(plan_text=C.cast(text, C.c_void_p), plan_capacity=0), "go together"), (dict(plan_capacity=8), "go together"),
             (dict(kernel=1), "split-K conv: unsupported layer"), (dict(kernel=1, cin=128, cin_real=128, res=0x30000), "split-K conv"),
             (dict(kernel=1, cin=256, cin_real=256, pool=1), "split-K conv"), (dict(kernel=1, cin=128, cin_real=128, nb=2), "split-K conv"),
             (dict(kernel=1, cin=128, cin_real=128, taps=1), "split-K conv"), (dict(kernel=1, cin=128, cin_real=128, H=256, W=256), "split-K conv"),
             (dict(kernel=2), "tower kernel"), (dict(kernel=2, nb=2, in_pitch=34, out_pitch=34, cout=128), "tower kernel"),
             (dict(kernel=2, nb=2, in_pitch=34, out_pitch=36), "tower kernel"),
             (dict(kernel=2, nb=2, in_pitch=34, out_pitch=34, res=0x30000, res_pitch=35), "tower kernel"),
             (dict(kernel=2, nb=2, in_pitch=34, out_pitch=34, items=2, in_item_bytes=1 << 20, out_item_bytes=1 << 20), "tower kernel")]
    for kw, text_ in cases:
        msg = refused(lib, "ju_debug_conv", conv_args(**kw), "ju_debug_conv")
        assert text_ in msg, (kw, msg)
    # the launchers' own wording
    for src, texts in (("conv_kernels.hip", ["conv: cin must be a multiple of 16, cout of 32*nb", "conv: unsupported shape",
                                            "conv: fused max-pool needs rw = 2, even H and W, 16-bit output",
                                            "conv: fused upsampling needs 3x3, cin % 64 == 0, nb = 1, even H and W",
                                            "launchConv: a look-ahead launch (items > 1) takes no residual"]),
                       ("splitk_kernels.hip", ["split-K conv: unsupported layer"])):
        code = open(os.path.join(ROOT, "joshupscale_amd", "csrc", src)).read()
        api = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "c_api.cpp")).read()
        for t in texts:
            assert '"' + t + '"' in code and '"' + t + '"' in api


def fb_args(**kw):
    w = np.zeros(9 * 64 * 64, np.float32)
    a = R.JuDebugFlowBlock()
    a.dtype, a.inp, a.out = E.F16, 0x10000, 0x20000
    a.H, a.W, a.cin, a.cin_real, a.cmid, a.pool, a.act1, a.act2, a.slope, a.items = 4, 4, 32, 32, 64, 1, 1, 1, 0.25, 1
    a.plan = R.JuDebugPlan(0, 0, -1, 0, 0, 0, 0)
    a._keep = w
    a.weights1 = a.weights2 = a.bias1 = a.bias2 = w.ctypes.data
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_other_hooks_refuse_bad_arguments_before_any_device_call(hip_library):
    lib = hip_library
    for fn in HOOKS[1:]:
        assert "null arguments" in refused(lib, fn, None, fn)
    cases = [(dict(dtype=-1), "dtype"), (dict(inp=None), "null buffer"), (dict(weights2=None), "null buffer"), (dict(bias1=None), "null buffer"),
             (dict(out=0x20004), "16-byte aligned"), (dict(H=0), "1 .. 4096"), (dict(act1=3), "activation"), (dict(act2=2, slope=-0.5), "slope"),
             (dict(items=0), "items"), (dict(items=9), "more look-ahead frames than kFlowBatchMax"),
             (dict(items=2, residual=1, cin=64, cin_real=64, pool=0), "the residual form has no look-ahead launch"),
             (dict(H=5), "fused max-pool needs even H and W"), (dict(cin=128, cin_real=128, pool=0, upsample=1, W=6, H=3), "fused upsampling needs even"),
             (dict(pool=0), "unsupported shape"), (dict(cmid=32), "unsupported shape"), (dict(out_head=1), "unsupported shape"),
             (dict(cin=64, cin_real=64, cmid=64, pool=0), "unsupported shape"), (dict(cin=64, cin_real=64, pool=0, residual=1, out_head=1), "unsupported shape"),
             (dict(cin_real=33), "cin_real"), (dict(in_pitch=3), "input pitch"), (dict(out_pitch=1), "output pitch"),
             (dict(items=2, in_item_bytes=1000, out_item_bytes=4096), "input item stride"),
             (dict(items=2, in_item_bytes=4096, out_item_bytes=8), "output item stride"), (dict(plan_capacity=4), "go together")]
    for kw, text in cases:
        msg = refused(lib, "ju_debug_flow_block", fb_args(**kw), "ju_debug_flow_block")
        assert text in msg, (kw, msg)
    code = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "flow_kernels.hip")).read()
    for t in ("flow block: more look-ahead frames than kFlowBatchMax", "flow block: the residual form has no look-ahead launch",
              "flow block: fused upsampling needs even H and W", "flow block: fused max-pool needs even H and W", "flow block: unsupported shape"):
        assert '"' + t + '"' in code
    rs = lambda **kw: R.JuDebugResample(**{**dict(op=0, dtype=E.F16, inp=0x10000, out=0x20000, H=2, W=2, C=32, items=1), **kw})
    for kw, text in [(dict(op=2), "op must be"), (dict(dtype=3), "dtype"), (dict(inp=None), "null buffer"), (dict(out=0x20008), "16-byte aligned"),
                     (dict(W=0), "1 .. 4096"), (dict(C=12), "multiple of 8"), (dict(C=0), "multiple of 8"), (dict(items=9), "items"),
                     (dict(op=1, H=3), "even H and W"), (dict(op=1, items=2), "one item")]:
        assert text in refused(lib, "ju_debug_resample", rs(**kw), "ju_debug_resample"), kw
    wp = lambda **kw: R.JuDebugWarp(**{**dict(dtype=E.BF16, state=0x10000, flow=0x20000, frame=0x30000, frame_stride=16, out=0x40000, out_pitch=0,
                                              H=4, W=4, PW=4, pad_top=0, pad_left=0, sums=None, pre_warp_out=None, out_u8=None, out_stride=0), **kw})
    for kw, text in [(dict(dtype=2), "dtype"), (dict(state=None), "null buffer"), (dict(flow=None), "null buffer"), (dict(frame=None), "null buffer"),
                     (dict(out=None), "null buffer"), (dict(H=0), "1 .. 4096"), (dict(pad_left=1), "PW at least"), (dict(pad_top=-1), "pads"),
                     (dict(out_pitch=3), "output pitch"), (dict(state=0x10004), "8-byte aligned"), (dict(pre_warp_out=0x50002), "8-byte aligned"),
                     (dict(flow=0x20008), "16-byte aligned"), (dict(out=0x40008), "16-byte aligned"), (dict(frame=0x30002), "LR frame"),
                     (dict(frame_stride=18), "LR frame"), (dict(frame_stride=12), "LR frame"), (dict(frame_stride=-12), "LR frame"),
                     (dict(sums=0x60002), "sums"), (dict(out_u8=0x70002, out_stride=64), "warp_pack: the frame output must be 4-byte aligned"),
                     (dict(out_u8=0x70000, out_stride=66), "warp_pack: the frame output must be 4-byte aligned"),
                     (dict(out_u8=0x70000, out_stride=60), "below its row"), (dict(out_u8=0x70000, out_stride=-60), "below its row")]:
        assert text in refused(lib, "ju_debug_warp", wp(**kw), "ju_debug_warp"), kw
    assert '"warp_pack: the frame output must be 4-byte aligned"' in open(os.path.join(ROOT, "joshupscale_amd", "csrc", "frame_kernels.hip")).read()
