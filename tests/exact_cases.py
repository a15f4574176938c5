"""The case tables of the exact tests (docs/exact_tests.md), their inputs and their references -- imported by the GPU tests
(test_gpu_exact_conv.py, test_gpu_exact_warp.py) and by test_exact_cpu.py, which holds every case to the dyadic condition
on a machine without a GPU: a table that would test inexact arithmetic fails there.

Inputs unless a case says otherwise: integer activations in -8 .. 8, integer weights in -2 .. 2, integer bias in -4 .. 4,
ReLU and LeakyReLU(0.25) alternating over a case's shapes.  "wide" cases: activations in -255 .. 255, weights in -1 .. 1
(thinned so that the budget holds): the x2 expansion itself rounds in T there.

Shapes per kernel form, from the tile of the form (tw columns x th rows): 2 x 2; a frame smaller than one tile with odd
sizes; one row and one column more than a tile; exactly two tiles each way -- even sizes only where pool or upsampling
demand them."""

import functools
import zlib

import numpy as np

import exact_reference as E

DTYPES = (E.F16, E.BF16)
DTYPE_NAMES = {E.F16: "fp16", E.BF16: "bf16"}
SLOPE = 0.25


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def tower_pitch(w):
    return (w + 31) // 32 * 32 + 2


def tower_rows(h):
    return (h + 7) // 8 * 8 + 2


def shapes_for(tw, th, even):
    """The four shapes of a form whose tile is tw columns x th rows."""
    if even:
        small = (max(2, min(4, th - 2)), 6)
        return [(2, 2), small, (th + 2, tw + 2), (2 * th, 2 * tw)]
    return [(2, 2), (max(1, min(3, th - 1)), 7), (th + 1, tw + 1), (2 * th, 2 * tw)]


# ---- convolutions: launchConv / launchConvSplitK / launchConvTower ------------------------------------------------------------
def conv_case(name, kernel=0, taps=9, cin=64, cout=64, nb=1, rw=1, **kw):
    c = dict(name=name, kernel=kernel, taps=taps, cin=cin, cin_real=cin, cout=cout, nb=nb, rw=rw, acts=(1, 2), res=False, res_pad=0,
             out_head=False, pool=False, upsample=False, items=1, in_pad=0, out_pad=0, gap=0, amp=8, wamp=2, density=1.0,
             plan={}, expect={}, tower=False, rounds=(E.BF16,), shapes=None)
    c.update(kw)
    if c["shapes"] is None:
        c["shapes"] = shapes_for(32, 4 * rw, c["pool"] or c["upsample"])
    return c


def _conv_cases():
    cases = []
    for taps, cin in [(9, 64), (9, 32), (9, 16), (1, 64), (1, 32)]:
        for nb in (1, 2):
            for rw in (1, 2):
                # (a 1 x 1 convolution of 32 channels sums 32 small terms: too few to need the rounding)
                rounds = (E.BF16,) if taps == 9 else ()
                cases.append(conv_case("conv-t%d-c%d-nb%d-rw%d" % (taps, cin, nb, rw), taps=taps, cin=cin, nb=nb, rw=rw, rounds=rounds,
                                       in_pad=3 if nb == 2 else 0, out_pad=5 if rw == 2 else 0))
    cases += [
        conv_case("conv-res-own-pitch-nb2-rw2", nb=2, rw=2, res=True, res_pad=3, out_pad=1),
        conv_case("conv-res-c32", cin=32, res=True, res_pad=5, in_pad=2),
        conv_case("conv-head-rw1", cout=32, out_head=True, acts=(0, 2), rounds=()),
        conv_case("conv-head-rw2", cout=32, rw=2, out_head=True, acts=(0, 2), out_pad=2, rounds=()),
        conv_case("conv-pool-c16", cin=16, cout=32, rw=2, pool=True),
        conv_case("conv-pool-c64-nb2", nb=2, rw=2, pool=True, in_pad=1, out_pad=3),
        conv_case("conv-real-cin-12-of-16", cin=16, cin_real=12, cout=32),
        conv_case("conv-real-cin-12-of-16-nb2", cin=16, cin_real=12, cout=64, nb=2, rw=2),
    ]
    for cin in (64, 128):
        for rw in (1, 2):
            cases.append(conv_case("conv-ups-c%d-rw%d" % (cin, rw), cin=cin, cout=32, rw=rw, upsample=True, in_pad=rw - 1, out_pad=2 - rw))
    cases += [
        conv_case("conv-ups-wide-c64-rw1", cout=32, upsample=True, amp=255, wamp=1, density=0.5, rounds=DTYPES),
        conv_case("conv-ups-wide-c128-rw2", cin=128, cout=32, rw=2, upsample=True, amp=255, wamp=1, density=0.25, rounds=DTYPES),
    ]
    for cin in (128, 256):
        for stages in (0, 1, 2):
            for rw in ((1, 2) if stages == 2 else (1 + stages % 2,)):
                cases.append(conv_case("conv-c%d-stages%d-rw%d" % (cin, stages, rw), cin=cin, cout=32, rw=rw, plan=dict(conv_stages=stages),
                                       expect=dict(stages=stages), in_pad=stages))
    for items in (3, 8):
        cases.append(conv_case("conv-items%d" % items, cin=32, cout=32, items=items, gap=16 * items, shapes=[(2, 2), (5, 33)]))
        cases.append(conv_case("conv-items%d-pool-pitched" % items, cin=16, cout=32, rw=2, pool=True, items=items, gap=48, in_pad=1,
                               out_pad=2, shapes=[(2, 2), (10, 34)]))
    cases.append(conv_case("conv-items3-ups", cin=64, cout=32, upsample=True, items=3, gap=32, shapes=[(2, 2), (6, 34)]))
    cases.append(conv_case("conv-items3-c128-stages2", cin=128, cout=32, items=3, gap=16, plan=dict(conv_stages=2), expect=dict(stages=2),
                           shapes=[(5, 33)]))
    return cases


def _splitk_cases():
    cases = []
    # the launcher's own plan on the four shapes of a 32 x 6 tile (its rule gives a small frame 2-row tiles: both occur)
    for cin in (128, 256):
        for cout in (32, 128, 256):
            heavy = cin * cout >= 128 * 256
            cases.append(conv_case("splitk-c%d-o%d" % (cin, cout), kernel=1, cin=cin, cout=cout,
                                   shapes=[(2, 2), (3, 7), (7, 33)] + ([] if heavy else [(12, 64)]),
                                   plan=dict(splitk_rows=6), expect=dict(rows=6, blocks=1)))
    cases += [
        conv_case("splitk-c128-o32-own-plan", kernel=1, cin=128, cout=32, shapes=[(3, 7), (7, 33)], in_pad=2, out_pad=1),
        conv_case("splitk-pool-c128-o32", kernel=1, cin=128, cout=32, pool=True, plan=dict(splitk_rows=6), expect=dict(rows=6, blocks=1),
                  shapes=shapes_for(32, 6, True)),
        conv_case("splitk-pool-c128-o128-blocks2", kernel=1, cin=128, cout=128, pool=True, plan=dict(splitk_rows=4, splitk_blocks=2),
                  expect=dict(rows=4, blocks=2), shapes=[(2, 2), (6, 34)], out_pad=3),
        conv_case("splitk-items8", kernel=1, cin=128, cout=32, items=8, gap=64, shapes=[(2, 2), (7, 33)], plan=dict(splitk_rows=6),
                  expect=dict(rows=6, blocks=1, items=8)),
        conv_case("splitk-items8-own-plan-pool", kernel=1, cin=128, cout=64, items=8, gap=16, pool=True, shapes=[(6, 34)],
                  expect=dict(items=8)),
    ]
    # forced rows on a 35 x 34 frame: one frame, one reference per dtype, every plan its bytes
    for rows in (2, 6, 16, 18, 34):
        cases.append(conv_case("splitk-c256-o256-rows%d" % rows, kernel=1, cin=256, cout=256, shapes=[(35, 34)], acts=(2,),
                               plan=dict(splitk_rows=rows), expect=dict(rows=rows, blocks=1), data="splitk-c256-o256-35x34"))
        for blocks in (1, 2):
            cases.append(conv_case("splitk-c128-o128-rows%d-blocks%d" % (rows, blocks), kernel=1, cin=128, cout=128, shapes=[(35, 34)],
                                   acts=(1,), plan=dict(splitk_rows=rows, splitk_blocks=blocks), expect=dict(rows=rows, blocks=blocks),
                                   data="splitk-c128-o128-35x34"))
    return cases


def _tower_cases():
    cases = []
    for res in (False, True):
        cases.append(conv_case("tower%s" % ("-res" if res else ""), kernel=2, nb=2, rw=2, res=res, tower=True,
                               shapes=[(2, 2), (9, 33), (16, 64)]))
    return cases


CONV_CASES = _conv_cases()
SPLITK_CASES = _splitk_cases()
TOWER_CASES = _tower_cases()


def draw_weights(rng, taps, cin_real, cout, wamp, density):
    w = rng.integers(-wamp, wamp + 1, (taps, cin_real, cout)).astype(np.float64)
    if density < 1.0:
        w *= rng.random((taps, cin_real, cout)) < density
    return w


def conv_inputs(case, shape, act):
    """The host tensors of one launch of a conv case: x [items][inH][inW][cin], w [taps][cin_real][cout], bias, res or None."""
    h, w = shape
    rng = rng_of(case.get("data", case["name"]), shape, act)
    ih, iw = (h // 2, w // 2) if case["upsample"] else (h, w)
    x = rng.integers(-case["amp"], case["amp"] + 1, (case["items"], ih, iw, case["cin"])).astype(np.float64)
    wts = draw_weights(rng, case["taps"], case["cin_real"], case["cout"], case["wamp"], case["density"])
    bias = rng.integers(-4, 5, case["cout"]).astype(np.float64)
    res = rng.integers(-case["amp"], case["amp"] + 1, (h, w, case["cout"])).astype(np.float64) if case["res"] else None
    return dict(x=x, w=wts, bias=bias, res=res)


@functools.lru_cache(maxsize=64)
def _conv_reference(data_key, shape_index, act, dtype):
    case = next(c for c in CONV_CASES + SPLITK_CASES + TOWER_CASES if c.get("data", c["name"]) == data_key)
    shape = case["shapes"][shape_index]
    d = conv_inputs(case, shape, act)
    wp = np.zeros((case["taps"], case["cin"], case["cout"]))
    wp[:, :case["cin_real"]] = d["w"]                      # (the packer's cinMap: the padded channels weigh nothing)
    outs = [E.conv(d["x"][i], wp, d["bias"], case["taps"], act, SLOPE, d["res"], case["pool"], case["upsample"], case["out_head"],
                   dtype) for i in range(case["items"])]
    return d, outs


def conv_reference(case, shape_index, act, dtype):
    """(inputs, [E.conv's dict per item]); cached, shared by the cases that name one `data` (the plans of one frame)."""
    return _conv_reference(case.get("data", case["name"]), shape_index, act, dtype)


def act_of(case, shape_index):
    return case["acts"][shape_index % len(case["acts"])]


# ---- flow blocks: launchFlowBlock ---------------------------------------------------------------------------------------------
# the launcher's table (flow_kernels.hip JU_FB_CASE): cin, cmid, upsample, pool, kind 0 plain / 1 flow head / 2 residual,
# and the tile heights the launcher tries for the shape (those that fit LDS are in the plan text's `heights=`)
FB_SHAPES = [
    (16, 32, False, True, 0, (20, 18, 10, 6)),
    (32, 64, False, True, 0, (20, 18, 10, 6)),
    (64, 128, False, True, 0, (6, 4, 2)),
    (256, 128, True, False, 0, (6, 4, 2)),
    (256, 128, False, False, 0, (6, 4, 2)),
    (128, 64, True, False, 0, (20, 18, 10, 6)),
    (128, 64, False, False, 0, (20, 18, 10, 6)),
    (64, 32, True, False, 1, (20, 18, 10, 6)),
    (64, 32, False, False, 1, (20, 18, 10, 6)),
    (64, 64, False, False, 2, (14, 6)),
]
FB_TW = 30                                                 # kFbOutW


def fb_case(name, cin, cmid, ups, pool, kind, heights, **kw):
    c = dict(name=name, cin=cin, cin_real=12 if cin == 16 else cin, cmid=cmid, upsample=ups, pool=pool, out_head=kind == 1,
             residual=kind == 2, heights=heights, all_heights=heights, amp=4 if kind == 2 else 8, wamp=2, density1=1.0, density2=1.0, acts=(1, 2),
             plan={}, tower=False, wide=False, rounds=(E.BF16,) if kind != 1 else ())
    c.update(kw)
    return c


def _fb_cases():
    cases = []
    for cin, cmid, ups, pool, kind, heights in FB_SHAPES:
        name = "fb-%d-%d%s%s%s" % (cin, cmid, "-ups" if ups else "", "-pool" if pool else "", ("", "-head", "-res")[kind])
        if kind == 2:
            for tower in (False, True):
                t = "-tower" if tower else ""
                cases.append(fb_case(name + "-pipe" + t, cin, cmid, ups, pool, kind, heights, acts=(1,), tower=tower, form="res_block_pipe"))
                cases.append(fb_case(name + "-plain-by-plan" + t, cin, cmid, ups, pool, kind, heights, acts=(1,), plan=dict(res_block=1),
                                     tower=tower, form="res_block"))
                cases.append(fb_case(name + "-plain-by-lrelu" + t, cin, cmid, ups, pool, kind, heights, acts=(2,), tower=tower,
                                     form="res_block"))
                cases.append(fb_case(name + "-tile" + t, cin, cmid, ups, pool, kind, heights, plan=dict(res_block=2), tower=tower,
                                     form="flow_block"))
        else:
            # (conv B of the widest blocks sums 1152 products of conv A's outputs, whose quantum the x2 expansion and the
            # LeakyReLU have divided by 16: its weights are thinned until the budget holds -- test_exact_cpu.py decides)
            thin = {(256, 128, True): 0.2, (256, 128, False): 0.7, (128, 64, True): 0.6}.get((cin, cmid, ups), 1.0)
            cases.append(fb_case(name, cin, cmid, ups, pool, kind, heights, form="flow_block", density2=thin))
            if ups:
                cases.append(fb_case(name + "-wide", cin, cmid, ups, pool, kind, heights[-1:], all_heights=heights, amp=255, wamp=1, density1=16.0 / cin,
                                     density2=4.0 / cmid, wide=True, form="flow_block", rounds=DTYPES if kind != 1 else (E.BF16,)))
    return cases


FB_CASES = _fb_cases()


def fb_shapes(case, th):
    return shapes_for(FB_TW, th, case["upsample"] or case["pool"])


def fb_runs(case):
    """(tile height, shape, items) of every launch of a case: each height on its four shapes with one item, and on the
    tile-plus-one shape with three (the residual form has no look-ahead launch)."""
    runs = []
    for th in case["heights"]:
        shapes = fb_shapes(case, th)
        if case["wide"]:
            shapes = shapes[1:3]
        for s in shapes:
            runs.append((th, s, 1))
        if not case["residual"] and not case["wide"]:
            runs.append((th, shapes[2], 3))
    return runs


def fb_inputs(case, shape, items, act):
    h, w = shape
    rng = rng_of(case["name"].replace("-tower", ""), shape, items, act)
    ih, iw = (h // 2, w // 2) if case["upsample"] else (h, w)
    x = rng.integers(-case["amp"], case["amp"] + 1, (items, ih, iw, case["cin"])).astype(np.float64)
    w1 = draw_weights(rng, 9, case["cin_real"], case["cmid"], case["wamp"], case["density1"])
    w2 = draw_weights(rng, 9, case["cmid"], case["cmid"], case["wamp"], case["density2"])
    b1 = rng.integers(-4, 5, case["cmid"]).astype(np.float64)
    b2 = rng.integers(-4, 5, case["cmid"]).astype(np.float64)
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2)


@functools.lru_cache(maxsize=64)
def _fb_reference(name, shape, items, act, dtype):
    case = next(c for c in FB_CASES if c["name"] == name)
    d = fb_inputs(case, shape, items, act)
    w1 = np.zeros((9, case["cin"], case["cmid"]))
    w1[:, :case["cin_real"]] = d["w1"]
    outs = [E.flow_block(d["x"][i], w1, d["b1"], d["w2"], d["b2"], act, act, SLOPE, case["upsample"], case["pool"], case["out_head"],
                         case["residual"], dtype) for i in range(items)]
    return d, outs


def fb_reference(case, shape, items, act, dtype):
    return _fb_reference(case["name"], tuple(shape), items, act, dtype)


# ---- upsample2 / maxpool2 -----------------------------------------------------------------------------------------------------
RESAMPLE_CASES = []
for _op, _sizes in ((0, [(1, 1), (2, 2), (5, 7), (6, 10)]), (1, [(2, 2), (6, 10)])):
    for _c in (32, 256):
        for _items in ((1, 3) if _op == 0 else (1,)):
            RESAMPLE_CASES.append(dict(name="%s-c%d-items%d" % (("upsample2", "maxpool2")[_op], _c, _items), op=_op, C=_c, items=_items,
                                       sizes=_sizes, amp=8, rounds=()))
RESAMPLE_CASES.append(dict(name="upsample2-wide", op=0, C=32, items=1, sizes=[(5, 7), (6, 10)], amp=255, rounds=(E.BF16,)))


def resample_inputs(case, size):
    rng = rng_of(case["name"], size)
    return rng.integers(-case["amp"], case["amp"] + 1, (case["items"], size[0], size[1], case["C"])).astype(np.float64)


def resample_reference(case, size, dtype):
    x = resample_inputs(case, size)
    f = E.upsample2 if case["op"] == 0 else E.maxpool2
    return x, [f(x[i], dtype) for i in range(case["items"])]


# ---- warp ---------------------------------------------------------------------------------------------------------------------
WARP_SIZES = [(2, 2), (3, 5), (17, 33)]
WARP_FIELDS = ["zero", "integers", "fractions", "corners-and-beyond", "last-rows-and-columns", "far-40", "far-1000"]
# out_u8: None, or (extra bytes per row, byte offset of row 0 from a 16-byte boundary, bottom-up); with 16 W bytes per row
# a pitch that is a multiple of 16 / 8 / 4 keeps every row 16- / 8- / 4-byte aligned
WARP_CONFIGS = [
    dict(pads=(0, 0), pw_extra=0, tower_pitch=False, pre_warp=False, out_u8=None),
    dict(pads=(3, 5), pw_extra=2, tower_pitch=True, pre_warp=True, out_u8=(0, 0, False)),
    dict(pads=(0, 0), pw_extra=3, tower_pitch=False, pre_warp=True, out_u8=(8, 0, False)),
    dict(pads=(3, 5), pw_extra=0, tower_pitch=True, pre_warp=False, out_u8=(4, 4, False)),
    dict(pads=(3, 5), pw_extra=1, tower_pitch=False, pre_warp=True, out_u8=(16, 0, True)),
    dict(pads=(0, 0), pw_extra=0, tower_pitch=True, pre_warp=False, out_u8=(0, 8, False)),
    dict(pads=(3, 5), pw_extra=4, tower_pitch=False, pre_warp=False, out_u8=None),
]
WARP_CASES = [dict(name="warp-%dx%d-%s" % (h, w, f), H=h, W=w, field=f, **WARP_CONFIGS[(k + 3 * i) % len(WARP_CONFIGS)])
              for i, (h, w) in enumerate(WARP_SIZES) for k, f in enumerate(WARP_FIELDS)]


def warp_field(kind, H, W, rng):
    """The HR flow field [4H][4W][2] (dy, dx) of a kind: multiples of 1/8 that f16 holds."""
    hh, ww = 4 * H, 4 * W
    gy, gx = np.meshgrid(np.arange(hh, dtype=np.float64), np.arange(ww, dtype=np.float64), indexing="ij")
    if kind == "zero":
        return np.zeros((hh, ww, 2))
    if kind == "integers":
        return rng.integers(-3, 4, (hh, ww, 2)).astype(np.float64)
    if kind == "fractions":
        return rng.integers(-24, 25, (hh, ww, 2)) / 8.0
    if kind in ("corners-and-beyond", "last-rows-and-columns"):
        if kind == "corners-and-beyond":              # every sample sent to a corner, onto an edge or beyond one, in turn
            ty = np.array([0.0, hh - 1.0, -1.5, hh + 0.5, 0.0, hh - 1.0, -7.0, hh + 6.0])
            tx = np.array([0.0, ww - 1.0, ww + 0.5, -1.5, ww - 1.0, 0.0, 0.25, ww - 1.25])
        else:                                         # exactly on rows / columns size - 2 and size - 1, and just around them
            ty = np.array([hh - 2.0, hh - 1.0, hh - 2.0, hh - 1.5, hh - 2.125, hh - 1.0, hh - 0.875, hh - 2.0])
            tx = np.array([ww - 2.0, ww - 1.0, ww - 1.0, ww - 2.0, ww - 1.0, ww - 2.125, ww - 2.0, ww - 0.875])
        k = rng.integers(0, 8, (hh, ww))
        return np.stack([gy - ty[k], gx - tx[k]], -1)  # query = position - flow = the target
    amp = 40.0 if kind == "far-40" else 1000.0
    f = rng.choice([-amp, amp], (hh, ww, 2)) + (rng.integers(-4, 5, (hh, ww, 2)) / 8.0 if amp < 512 else rng.integers(-2, 3, (hh, ww, 2)) / 2.0)
    return f


def warp_inputs(case):
    H, W = case["H"], case["W"]
    rng = rng_of(case["name"])
    pt, pl = case["pads"]
    PW = W + pl + case["pw_extra"]
    PH = H + pt + 2
    field = warp_field(case["field"], H, W, rng)
    flow = rng.integers(-8, 9, (PH, PW, 32)) / 8.0                       # (the padding: other values, never read)
    flow[pt:pt + H, pl:pl + W] = field.reshape(H, 4, W, 4, 2).transpose(0, 2, 1, 3, 4).reshape(H, W, 32)
    state = rng.integers(-256, 257, (4 * H, 4 * W, 4)) / 512.0
    edge = rng.random((4 * H, 4 * W, 4))
    state[edge < 0.1] = 0.5
    state[edge > 0.9] = -0.5
    frame = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    if H * W * 3 >= 256:                                                  # every byte value where the frame has room
        flat = frame[..., :3].reshape(-1)
        flat[:256] = np.arange(256, dtype=np.uint8)
        frame[..., :3] = flat.reshape(H, W, 3)
    return dict(state=state, flow=flow, frame=frame, PW=PW, PH=PH, field=field)


def warp_reference(case, dtype, **fault):
    d = warp_inputs(case)
    return d, E.warp(d["state"], d["flow"], d["frame"], case["H"], case["W"], d["PW"], case["pads"][0], case["pads"][1], dtype, **fault)
