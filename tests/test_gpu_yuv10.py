"""10-bit 4:2:0 frame I/O on the GPU (P010 / I010; csrc/colour_kernels.hip, engine_frames.cpp): the three conversion kernels
alone against the numpy definition (tests/yuv10_reference.py), byte for byte; 10-bit inputs against a twin fed the
decoded frame; 10-bit outputs against the definition applied to the runtime's own f16 state (or, for the models whose
state is not the frame, to the twin's 8-bit frame); every format pair, location and call; look-ahead passes against a
twin driven frame by frame; the refused calls."""

import ctypes as C
import dataclasses

import numpy as np
import pytest

import yuv10_reference as T
import yuv_reference as Y
from flowfree_common import flow_free
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_yuv import CSS, SIZES, DevPlane, torch_dev
from test_gpu_yuv_lookahead import HostPlane

pytestmark = pytest.mark.gpu

BGRX, I420, NV12, P010, I010 = 0, 1, 2, 3, 4
TEN = (P010, I010)
ALL = (BGRX, I420, NV12, P010, I010)
NAMES = {BGRX: "bgrx", I420: "i420", NV12: "nv12", P010: "p010", I010: "i010"}


def as_bytes(a):
    """A uint16 (or uint8) plane as its bytes [rows][row bytes] -- what DevPlane / HostPlane hold and compare."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def words_of(fmt, y, u, v):
    """The caller's planes of 8- or 10-bit samples in the given format."""
    if fmt in TEN:
        return T.to_words(fmt, y, u, v)
    return [y, u, v] if fmt == I420 else [y, Y.to_nv12(u, v)]


def blank_planes(fmt, h, w):
    if fmt == BGRX:
        return [np.zeros((h, w, 4), np.uint8)]
    dt = np.uint16 if fmt in TEN else np.uint8
    if fmt in (NV12, P010):
        return [np.zeros((h, w), dt), np.zeros((h // 2, w), dt)]
    return [np.zeros((h, w), dt), np.zeros((h // 2, w // 2), dt), np.zeros((h // 2, w // 2), dt)]


def state_of(rt, h, w):
    """The runtime's recurrent state as float16 [4h][4w][4] (ju_read_tensor widens it to float32, exactly)."""
    s32 = rt.read_tensor("state").reshape(4 * h, 4 * w, 4)
    s16 = s32.astype(np.float16)
    assert np.array_equal(s16.astype(np.float32), s32)
    return s16


def expect_planes(fmt, cs, frame, state):
    """What a runtime writes for an output of the format: from its 8-bit frame, or -- a 10-bit format with a state
    given -- from the state."""
    if fmt == BGRX:
        return [frame]
    if fmt in TEN:
        p = T.p_from_state(state) if state is not None else T.p_from_u8(frame)
        return words_of(fmt, *T.encode10(p, cs))
    return words_of(fmt, *Y.encode(frame, cs))


def decoded(fmt, cs, planes):
    """The BGRX frame the network consumes for the caller's planes."""
    if fmt == BGRX:
        return planes[0]
    if fmt in TEN:
        return T.decode10(*T.from_words(fmt, planes), cs)
    return Y.decode(planes[0], *((planes[1], planes[2]) if fmt == I420 else Y.from_nv12(planes[1])), cs)


def source(frame, fmt, cs):
    """The planes of one input frame of a BGRX clip in the given format."""
    if fmt == BGRX:
        return [frame]
    if fmt in TEN:
        return words_of(fmt, *T.encode10(T.p_from_u8(frame), cs))
    return words_of(fmt, *Y.encode(frame, cs))


def blob_of(cfg, wts=None):
    return M.serialize(cfg, wts if wts is not None else M.make_seeded_weights(cfg))


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------
LAYOUTS = {"dense": dict(pad=0, offset=0, flip=False), "padded": dict(pad=32, offset=0, flip=False),
           "bottom-up": dict(pad=16, offset=0, flip=True), "offset-2": dict(pad=6, offset=2, flip=False),
           "offset-6": dict(pad=10, offset=6, flip=False), "padded-bottom-up": dict(pad=6, offset=2, flip=True)}


def run_debug10(op, fmt, cs, w, h, image_ptr, image_stride, planes):
    lib = R.load_library(True)
    ptrs = (C.c_void_p * 3)(*([p.ptr for p in planes] + [None] * (3 - len(planes))))
    strides = (C.c_ssize_t * 3)(*([p.stride for p in planes] + [0] * (3 - len(planes))))
    rc = lib.ju_debug_yuv10(op, fmt, cs, w, h, image_ptr, image_stride, ptrs, strides)
    assert rc == 0, lib.ju_last_error()


def content10(kind, h, w, rng):
    shapes = ((h, w), (h // 2, w // 2), (h // 2, w // 2))
    if kind in ("random", "junk"):
        return [rng.integers(0, 1024, s, dtype=np.uint16) for s in shapes]
    if kind == "zero":
        return [np.zeros(s, np.uint16) for s in shapes]
    if kind == "full":
        return [np.full(s, 1023, np.uint16) for s in shapes]
    cb = (np.indices(shapes[1]).sum(0) % 2 * 1023).astype(np.uint16)    # extreme chroma in a checkerboard of cells
    return [rng.integers(0, 1024, shapes[0], dtype=np.uint16), cb, (1023 - cb).astype(np.uint16)]


def with_junk(fmt, planes, rng):
    """Random bits where the format ignores them: P010's low 6, I010's high 6."""
    shift = 0 if fmt == P010 else 10
    return [p | (rng.integers(0, 64, p.shape, dtype=np.uint16) << shift) for p in planes]


def random_state(h, w, rng):
    """f16 [h][w][4] in -0.5 .. 0.5 with the values the sample formula has to get exactly right sprinkled in."""
    s = rng.uniform(-0.5, 0.5, (h, w, 4)).astype(np.float16)
    special = np.array([0.5, -0.5, 0.0, -0.0, 6e-8, -6e-8, 3e-5, -3e-5, 6.1e-5, 0.49976, -0.49976, 0.75, -0.75, 2.0, -3.0],
                       np.float16)
    flat = s.reshape(-1)
    where = rng.choice(flat.size, min(flat.size, 4 * special.size), replace=False)
    flat[where] = special[np.arange(where.size) % special.size]
    return s


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("fmt", TEN, ids=["p010", "i010"])
def test_kernels_equal_the_numpy_definition(fmt, layout):
    torch, dev = torch_dev()
    rng = np.random.default_rng(7)
    lay = LAYOUTS[layout]
    img_lay = dict(pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
    for (h, w) in SIZES:
        for cs in CSS:
            for kind in ("random", "zero", "full", "extreme", "junk"):
                y, u, v = content10(kind, h, w, rng)
                held = words_of(fmt, y, u, v)
                if kind == "junk":
                    held = with_junk(fmt, held, rng)
                # decode: planes -> BGRX
                src = [DevPlane(as_bytes(p), **lay) for p in held]
                out = DevPlane(np.zeros((h, w, 4), np.uint8), **img_lay)
                run_debug10(0, fmt, cs, w, h, out.ptr, out.stride, src)
                out.check(T.decode10(y, u, v, cs))
                for p, d in zip(src, held):
                    p.check(as_bytes(d))                        # (inputs untouched)
                if kind == "junk":
                    continue
                # encode from a u8 frame (X random: ignored) -> planes
                bgrx = rng.integers(0, 256, (h, w, 4), dtype=np.uint8) if kind == "random" else T.decode10(y, u, v, cs)
                inb = DevPlane(bgrx, **img_lay)
                want = words_of(fmt, *T.encode10(T.p_from_u8(bgrx), cs))
                dst = [DevPlane(as_bytes(np.zeros_like(p)), **lay) for p in want]
                run_debug10(1, fmt, cs, w, h, inb.ptr, inb.stride, dst)
                for p, e in zip(dst, want):
                    p.check(as_bytes(e))
                # encode from an f16 tensor -> planes
                if kind == "random":
                    state = random_state(h, w, rng)
                elif kind == "zero":
                    state = np.full((h, w, 4), -0.5, np.float16)
                elif kind == "full":
                    state = np.full((h, w, 4), 0.5, np.float16)
                else:
                    state = (bgrx.astype(np.float32) / 255.0 - 0.5).astype(np.float16)
                d_state = torch.from_numpy(state).to(dev)
                assert d_state.data_ptr() % 16 == 0
                want = words_of(fmt, *T.encode10(T.p_from_state(state), cs))
                dst = [DevPlane(as_bytes(np.zeros_like(p)), **lay) for p in want]
                run_debug10(2, fmt, cs, w, h, d_state.data_ptr(), 0, dst)
                for p, e in zip(dst, want):
                    p.check(as_bytes(e))
                assert np.array_equal(d_state.cpu().numpy().view(np.uint16), state.view(np.uint16))


def test_items_kernel_decodes_8_and_10_bit_items_in_one_launch():
    """ju_debug_yuv_items with the four YUV formats mixed: per item the definition's frame and the guards intact."""
    lib = R.load_library(True)
    rng = np.random.default_rng(21)
    names = sorted(LAYOUTS)
    for (h, w) in [(46, 30), (18, 100)]:
        fmts, css, outs, srcs, want = [], [], [], [], []
        for i in range(8):
            fmt = (P010, I420, I010, NV12)[i % 4]
            lay = LAYOUTS[names[i % len(names)]]
            if fmt in TEN:
                y, u, v = content10("random", h, w, rng)
                held = with_junk(fmt, words_of(fmt, y, u, v), rng)
            else:
                y, u, v = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
                held = words_of(fmt, y, u, v)
            fmts.append(fmt)
            css.append(CSS[i % 4])
            want.append(decoded(fmt, css[-1], held))
            srcs.append([DevPlane(as_bytes(p), **lay) for p in held])
            outs.append(DevPlane(np.zeros((h, w, 4), np.uint8), pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"]))
        ptrs, strides = [], []
        for planes in srcs:
            ptrs += [p.ptr for p in planes] + [None] * (3 - len(planes))
            strides += [p.stride for p in planes] + [0] * (3 - len(planes))
        rc = lib.ju_debug_yuv_items(8, (C.c_int * 8)(*fmts), (C.c_int * 8)(*css), w, h,
                                    (C.c_void_p * 8)(*[o.ptr for o in outs]), (C.c_ssize_t * 8)(*[o.stride for o in outs]),
                                    (C.c_void_p * 24)(*ptrs), (C.c_ssize_t * 24)(*strides))
        assert rc == 0, lib.ju_last_error()
        for o, e in zip(outs, want):
            o.check(e)


# ---- 2. 10-bit inputs -------------------------------------------------------------------------------------------------
SMALL = [pytest.param(R.DTYPE_BF16, id="bf16"), pytest.param(R.DTYPE_F16, id="fp16"), pytest.param(R.DTYPE_FP8, id="fp8")]


@pytest.mark.parametrize("dtype", SMALL)
@pytest.mark.parametrize("fmt", TEN, ids=["p010", "i010"])
def test_10_bit_input_equals_process_of_the_decoded_frame(fmt, dtype):
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED if fmt == P010 else Y.CS_BT601_FULL
    rng = np.random.default_rng(3)
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        for t, f in enumerate(M.synthetic_frames(5, h, w, seed=3, kind="smooth")):
            held = source(f, fmt, cs)
            if t % 2:
                held = with_junk(fmt, held, rng)
            got = np.zeros((4 * h, 4 * w, 4), np.uint8)
            a.process_frame(R.host_frame(fmt, held, cs), R.host_frame(R.FMT_BGRX, [got]))
            want = b.process_image(decoded(fmt, cs, held))
            assert np.array_equal(got, want), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


# ---- 3. 10-bit outputs: which source, and its bytes ---------------------------------------------------------------
def check_output_from_state(blob, dtype, frames, fmt, cs):
    cfg, _ = M.deserialize(blob)
    h, w = cfg.frame_height, cfg.frame_width
    with R.Runtime(blob, 0, dtype) as rt:
        assert rt.stat("hbd_from_state") == 1
        for t, f in enumerate(frames):
            got = blank_planes(fmt, 4 * h, 4 * w)
            rt.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(fmt, got, cs))
            want = expect_planes(fmt, cs, None, state_of(rt, h, w))
            for g, e in zip(got, want):
                assert np.array_equal(g, e), t


@pytest.mark.parametrize("dtype", SMALL)
@pytest.mark.parametrize("fmt", TEN, ids=["p010", "i010"])
def test_output_is_encoded_from_the_state(fmt, dtype):
    cfg = small_config()
    frames = M.synthetic_frames(4, cfg.frame_height, cfg.frame_width, seed=8, kind="smooth")
    check_output_from_state(blob_of(cfg), dtype, frames, fmt, Y.CS_BT709_LIMITED if fmt == P010 else Y.CS_BT601_FULL)


@pytest.mark.parametrize("variant", ["lrelu", "temporal-still", "temporal-moving", "temporal-window3"])
def test_output_from_the_state_of_other_models(variant):
    """A LeakyReLU model and the temporal filter (which blends the state in place): a still clip keeps the filter's
    gate on the blending side, noise frames on the other."""
    if variant == "lrelu":
        cfg = small_config(flow_activation="lrelu", gen_activation="lrelu", gen_negative_slope=0.2)
    elif variant == "temporal-window3":
        cfg = small_config(temporal_strength=0.25, temporal_window=3)
    else:
        cfg = small_config(temporal_strength=0.25, temporal_threshold=0.5)
    h, w = cfg.frame_height, cfg.frame_width
    if variant == "temporal-still":
        frames = [M.synthetic_frames(1, h, w, seed=5, kind="smooth")[0]] * 4
    elif variant == "temporal-moving":
        frames = M.synthetic_frames(4, h, w, seed=5, kind="noise")
    else:
        frames = M.synthetic_frames(4, h, w, seed=5, kind="smooth")
    check_output_from_state(blob_of(cfg), R.DTYPE_F16, frames, P010, Y.CS_BT709_LIMITED)
    check_output_from_state(blob_of(cfg), R.DTYPE_BF16, frames, I010, Y.CS_BT601_LIMITED)


def bgrx_to(rt, frame, fmt, cs):
    """One step of `rt` on the BGRX frame (both runtimes of a comparison consume the SAME frame), output planes in fmt."""
    cfg_h, cfg_w = frame.shape[:2]
    got = blank_planes(fmt, 4 * cfg_h, 4 * cfg_w)
    rt.process_frame(R.host_frame(R.FMT_BGRX, [frame]), R.host_frame(fmt, got, cs))
    return got


def y10_against_y8(y10, y8):
    """The relation of test_10_bit_luma_lies_around_4_times_the_8_bit_luma, as (min, max) of Y10 - 4 Y8."""
    d = y10.astype(np.int64) - 4 * y8.astype(np.int64)
    return int(d.min()), int(d.max())


def test_flow_free_model_encodes_from_its_scratch_state():
    """A flow-free model has no readable state (ju_read_tensor refuses the name), but its tail writes the frame in
    float into the scratch state all the same, and that is what the encode reads: "hbd_from_state" is 1, the luma keeps
    the relation to the 8-bit luma derived below and uses all four values of its two extra bits."""
    cfg, wts = flow_free(small_config())
    blob = blob_of(cfg, wts)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        assert not a.recurrent and a.stat("hbd_from_state") == 1
        for f in M.synthetic_frames(3, h, w, seed=6, kind="smooth"):
            (y10, uv10), (y8, uv8) = bgrx_to(a, f, P010, cs), bgrx_to(b, f, NV12, cs)
            assert (y10 & 63 == 0).all() and (uv10 & 63 == 0).all()
            lo, hi = y10_against_y8(y10 >> 6, y8)
            print("flow-free Y10 - 4 Y8:", lo, hi)
            assert -2 <= lo and hi <= 6
            assert set(np.unique((y10 >> 6) % 4)) == {0, 1, 2, 3}
            assert np.abs((uv10 >> 6).astype(np.int64) - 4 * uv8.astype(np.int64)).max() <= 8


@pytest.mark.parametrize("variant", ["brightness", "output-flow"])
@pytest.mark.parametrize("fmt", TEN, ids=["p010", "i010"])
def test_models_whose_state_is_not_the_frame_encode_from_the_8_bit_frame(fmt, variant):
    if variant == "brightness":
        cfg = small_config(normalize_brightness=True)
        blob = blob_of(cfg)
    else:
        cfg = small_config()
        blob = M.serialize(*M.output_flow(cfg, M.make_seeded_weights(cfg)))
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT601_LIMITED if fmt == P010 else Y.CS_BT709_FULL
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        assert a.stat("hbd_from_state") == 0
        for t, f in enumerate(M.synthetic_frames(4, h, w, seed=11, kind="smooth")):
            got = blank_planes(fmt, 4 * h, 4 * w)
            a.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(fmt, got, cs))
            frame = b.process_image(f)
            for g, e in zip(got, expect_planes(fmt, cs, frame, None)):
                assert np.array_equal(g, e), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


# ---- 4. a relation that a wrong source cannot meet ---------------------------------------------------------------------
def test_10_bit_luma_lies_around_4_times_the_8_bit_luma():
    """Plain model, limited range: with Y8 from an NV12 twin, -2 <= Y10 - 4 Y8 <= 6 everywhere, and Y10 % 4 takes all
    four values (an encode from 257 x u8 would leave most pixels on few of them and could not be told apart by the
    byte comparison of the tests above alone, which take the state as given).

    Derivation, t = r + 0.5 with r the tail's f32 output: the 8-bit frame is u8 = floor(255 t).  The state holds r
    rounded to f16 (spacing at most 2^-12 below 0.5, error at most 2^-13), P = floor(65536 (s + 0.5)), so P / 257 lies
    within 255 x 2^-13 = 0.031 (the rounding) + 0.004 (65536 / 257 = 255.004 against 255) of 255 t, less up to
    1 / 257 for the floor: P / 257 - u8 is in [-0.035, 1.035].  The real-valued lumas 64 + 876 Y' then differ by
    876 / 255 times a weighted mean of that: [-0.12, 3.56].  The 10-bit rounding adds +-0.5 and 4 x the 8-bit
    rounding +-2: [-2.62, 6.06], integers in -2 .. 6."""
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    for cs in (Y.CS_BT709_LIMITED, Y.CS_BT601_LIMITED):
        with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
            for f in M.synthetic_frames(4, h, w, seed=14, kind="smooth"):
                (y10, _, _), (y8, _) = bgrx_to(a, f, I010, cs), bgrx_to(b, f, NV12, cs)
                lo, hi = y10_against_y8(y10, y8)
                print("Y10 - 4 Y8:", lo, hi, "values of Y10 % 4:", np.bincount(y10.reshape(-1) % 4, minlength=4))
                assert -2 <= lo and hi <= 6, (lo, hi)
                assert set(np.unique(y10 % 4)) == {0, 1, 2, 3}
                assert int(y10.max()) <= 1023


# ---- 5. every new pair of formats, locations, calls ----------------------------------------------------------------
NEW_PAIRS = [(i, o) for i in ALL for o in ALL if i in TEN or o in TEN]


def dev_copy(arr, dev, flip):
    """A device copy of a host plane, described top-down or bottom-up: (tensor, pointer, byte stride)."""
    import torch
    data = np.ascontiguousarray(arr[::-1] if flip else arr)
    t = torch.from_numpy(as_bytes(data).copy()).to(dev)
    pitch = data.strides[0]
    ptr = t.data_ptr() + (data.shape[0] - 1) * pitch if flip else t.data_ptr()
    return t, ptr, (-pitch if flip else pitch)


def dev_back(t, like, flip):
    got = t.cpu().numpy().reshape(like.shape[0], -1).view(like.dtype).reshape(like.shape)
    return got[::-1] if flip else got


def test_all_16_new_format_pairs_on_host_device_and_mixed_frames():
    assert len(NEW_PAIRS) == 16
    torch, dev = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(3, h, w, seed=4, kind="smooth")
    for k, (fin, fout) in enumerate(NEW_PAIRS):
        cin, cout = CSS[k % 4], CSS[(k + 1) % 4]
        for loc_in, loc_out in (("host", "host"), ("device", "device"), ("host", "device"), ("device", "host")):
            flip = (k + len(loc_in)) % 2 == 1
            with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
                for t, f in enumerate(frames):
                    held = source(f, fin, cin)
                    blank = blank_planes(fout, 4 * h, 4 * w)
                    keep = []
                    if loc_in == "host":
                        vin = [np.ascontiguousarray(p[::-1])[::-1] if flip else p for p in held]
                        keep.append(vin)
                        f_in = R.host_frame(fin, vin, cin)
                    else:
                        d_in = [dev_copy(p, dev, flip) for p in held]
                        f_in = R.device_frame(fin, w, h, [x[1] for x in d_in], [x[2] for x in d_in], cin)
                    if loc_out == "host":
                        f_out = R.host_frame(fout, [p[::-1] for p in blank] if flip else blank, cout)
                    else:
                        d_out = [dev_copy(p, dev, flip) for p in blank]
                        f_out = R.device_frame(fout, 4 * w, 4 * h, [x[1] for x in d_out], [x[2] for x in d_out], cout)
                    torch.cuda.synchronize()
                    a.process_frame(f_in, f_out)
                    if loc_out == "host":
                        got = [p[::-1] if flip else p for p in blank]
                    else:
                        got = [dev_back(x[0], p, flip) for x, p in zip(d_out, blank)]
                    frame = b.process_image(decoded(fin, cin, held))
                    want = expect_planes(fout, cout, frame, state_of(b, h, w))
                    for g, e in zip(got, want):
                        assert np.array_equal(g, e), (NAMES[fin], NAMES[fout], loc_in, loc_out, t)
                assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))


def test_mixed_calls_on_one_runtime():
    """ju_process, 8-bit and 10-bit ju_process_frame, and ju_enqueue_frame + ju_synchronize on device planes, on one
    stream: every frame equals the all-BGRX twin's composed with the numpy conversions."""
    torch, dev = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT601_LIMITED
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        for t, f in enumerate(M.synthetic_frames(8, h, w, seed=12, kind="smooth")):
            mode = t % 4
            fin, fout = [(BGRX, BGRX), (P010, I010), (NV12, NV12), (I010, P010)][mode]
            held = source(f, fin, cs)
            frame = b.process_image(decoded(fin, cs, held))
            want = expect_planes(fout, cs, frame, state_of(b, h, w))
            if mode == 0:
                got = [a.process_image(held[0])]
            elif mode in (1, 2):
                got = blank_planes(fout, 4 * h, 4 * w)
                a.process_frame(R.host_frame(fin, held, cs), R.host_frame(fout, got, cs))
            else:
                d_in = [dev_copy(p, dev, False) for p in held]
                blank = blank_planes(fout, 4 * h, 4 * w)
                d_out = [dev_copy(p, dev, False) for p in blank]
                torch.cuda.synchronize()
                a.enqueue_frame(R.device_frame(fin, w, h, [x[1] for x in d_in], colorspace=cs),
                                R.device_frame(fout, 4 * w, 4 * h, [x[1] for x in d_out], colorspace=cs))
                a.synchronize()
                got = [dev_back(x[0], p, False) for x, p in zip(d_out, blank)]
            for g, e in zip(got, want):
                assert np.array_equal(g, e), t


# ---- 6. look-ahead passes -----------------------------------------------------------------------------------------------
HOST_LAYOUTS = {"plain": dict(pad=0, flip=False), "padded": dict(pad=24, flip=False), "bottom-up": dict(pad=8, flip=True)}


class Side:
    """One side of a frame call: its planes in host or device memory with guard bytes around them."""

    def __init__(self, fmt, cs, loc, layout, planes, w, h):
        lay = dict(HOST_LAYOUTS[layout], offset=0)
        if fmt == BGRX:
            lay["pad"] *= 4
        cls = HostPlane if loc == "host" else DevPlane
        self.planes = [cls(as_bytes(p) if fmt != BGRX else p, **lay) for p in planes]
        self.frame = R._frame(fmt, cs, R.LOC_CPU if loc == "host" else R.LOC_DEVICE, w, h,
                              [p.ptr for p in self.planes], [p.stride for p in self.planes])

    def check(self, want):
        for p, e in zip(self.planes, want):
            p.check(as_bytes(e) if e.ndim == 2 else e)


@dataclasses.dataclass
class Spec:
    fin: int
    cin: int
    lin: str = "host"
    layin: str = "plain"
    fout: int = P010
    cout: int = Y.CS_BT709_LIMITED
    lout: str = "host"
    layout: str = "plain"


def twin_bytes(blob, dtype, frames, specs):
    """What ju_process_frame, called frame by frame on plain host frames, writes; + the state and the history."""
    cfg, _ = M.deserialize(blob)
    h, w = cfg.frame_height, cfg.frame_width
    want = []
    with R.Runtime(blob, 0, dtype) as rt:
        for f, s in zip(frames, specs):
            pout = blank_planes(s.fout, 4 * h, 4 * w)
            pin = source(f, s.fin, s.cin)                       # (kept alive: the frame holds raw pointers)
            rt.process_frame(R.host_frame(s.fin, pin, s.cin), R.host_frame(s.fout, pout, s.cout))
            want.append(pout)
        tensors = [rt.read_tensor(n).copy() for n in ("state", "flow_in")] if rt.recurrent else None
    return want, tensors


def make_sides(frames, specs, h, w):
    ins = [Side(s.fin, s.cin, s.lin, s.layin, source(f, s.fin, s.cin), w, h) for f, s in zip(frames, specs)]
    outs = [Side(s.fout, s.cout, s.lout, s.layout, blank_planes(s.fout, 4 * h, 4 * w), 4 * w, 4 * h) for s in specs]
    torch_dev()[0].cuda.synchronize()
    return ins, outs


def run_calls(rt, ins, outs, want, lengths):
    t = 0
    for k in lengths:
        rt.process_frames([x.frame for x in ins[t:t + k]], [x.frame for x in outs[t:t + k]])
        for i in range(t, t + k):
            outs[i].check(want[i])
        t += k


def tensors_equal(rt, tensors):
    return all(np.array_equal(rt.read_tensor(n), e) for n, e in zip(("state", "flow_in"), tensors))


@pytest.mark.parametrize("loc", ["host", "device"])
@pytest.mark.parametrize("fmt", TEN, ids=["p010", "i010"])
def test_passes_of_10_bit_frames_give_the_frame_by_frame_bytes(fmt, loc):
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    n = 13
    frames = M.synthetic_frames(n, h, w, seed=97, kind="smooth")
    lays = ["plain", "padded", "bottom-up"]
    specs = [Spec(fmt, CSS[t % 4], loc, lays[t % 3], fmt, CSS[(t + 1) % 4], loc, lays[(t + 2) % 3]) for t in range(n)]
    want, tensors = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        run_calls(rt, ins, outs, want, (8, 3, 2))
        assert tensors_equal(rt, tensors)
        assert rt.stat("lookahead_yuv_frames") == n and rt.stat("lookahead_frames") == n
        assert rt.stat("lookahead_host_frames") == (n if loc == "host" else 0) and rt.stat("fallbacks") == 0
        for i in ins:                                           # (inputs and their guards untouched)
            i.check([p._rows(p.host) for p in i.planes])
        # the same buffers again: captured at the second use, replayed at the third, same bytes
        for _ in range(2):
            rt.reset()
            run_calls(rt, ins, outs, want, (8, 3, 2))
        assert rt.stat("graph_replays") >= 3


def test_passes_mixing_8_and_10_bit_frames_and_locations():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    kinds = [Spec(P010, 2, "host", "padded", I010, 0, "host", "bottom-up"),
             Spec(NV12, 1, "device", "bottom-up", P010, 3, "device", "padded"),
             Spec(I010, 0, "device", "plain", NV12, 2, "host", "plain"),
             Spec(BGRX, 0, "host", "plain", I010, 1, "device", "bottom-up"),
             Spec(I420, 3, "host", "bottom-up", BGRX, 0, "host", "padded"),
             Spec(P010, 1, "device", "padded", BGRX, 0, "device", "plain")]
    specs = kinds + kinds[::-1]
    frames = M.synthetic_frames(len(specs), h, w, seed=19, kind="smooth")
    for dtype in (R.DTYPE_BF16, R.DTYPE_FP8):
        want, tensors = twin_bytes(blob, dtype, frames, specs)
        ins, outs = make_sides(frames, specs, h, w)
        with R.Runtime(blob, 0, dtype) as rt:
            run_calls(rt, ins, outs, want, (7, 5))
            assert tensors_equal(rt, tensors)
            assert rt.stat("lookahead_frames") == 12 and rt.stat("lookahead_yuv_frames") == 12
            assert rt.stat("fallbacks") == 0


def test_a_pass_that_is_run_again_gives_the_same_planes():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    specs = [Spec(P010, 2, "host", "bottom-up", P010, 2, "host", "padded") for _ in range(5)] + \
            [Spec(I010, 1, "device", "padded", I010, 3, "device", "plain") for _ in range(4)]
    frames = M.synthetic_frames(len(specs), h, w, seed=7, kind="smooth")
    want, tensors = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        assert lib.ju_debug_set(b"pass_rerun", 1) == 0
        try:
            run_calls(rt, ins, outs, want, (5, 4))
        finally:
            lib.ju_debug_set(b"pass_rerun", 0)
        assert rt.stat("lookahead_frames") == 0 and rt.stat("lookahead_yuv_frames") == 0 and rt.stat("fallbacks") == 0
        assert tensors_equal(rt, tensors)


def test_a_10_bit_plane_over_an_earlier_input_plane_starts_a_new_pass():
    """Frame 1's output Y plane (P010, 2 bytes per sample) lies over frame 0's input Y plane: frame 0 runs on its own and
    frames 1-3 as a pass, with the bytes of the frame-by-frame calls on the same buffers."""
    torch, dev = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    frames = M.synthetic_frames(4, h, w, seed=61, kind="smooth")
    src = [source(f, P010, cs) for f in frames]

    def run(call):
        arena = torch.zeros(2 * 16 * h * w, dtype=torch.uint8, device=dev)
        arena[: 2 * h * w] = torch.from_numpy(as_bytes(src[0][0]).reshape(-1).copy()).to(dev)
        d_in = [[torch.from_numpy(as_bytes(p).copy()).to(dev) for p in s] for s in src]
        d_out = [[torch.zeros(as_bytes(p).shape, dtype=torch.uint8, device=dev) for p in blank_planes(P010, 4 * h, 4 * w)]
                 for _ in frames]
        ins = [R.device_frame(P010, w, h, [arena, d_in[0][1]], colorspace=cs)] + \
              [R.device_frame(P010, w, h, d_in[t], colorspace=cs) for t in (1, 2, 3)]
        outs = [R.device_frame(P010, 4 * w, 4 * h, d_out[0], colorspace=cs),
                R.device_frame(P010, 4 * w, 4 * h, [arena, d_out[1][1]], colorspace=cs)] + \
               [R.device_frame(P010, 4 * w, 4 * h, d_out[t], colorspace=cs) for t in (2, 3)]
        torch.cuda.synchronize()
        with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
            call(rt, ins, outs)
            stats = (rt.stat("lookahead_frames"), rt.stat("lookahead_yuv_frames"))
            state = rt.read_tensor("state").copy()
        return [arena.cpu().numpy()] + [p.cpu().numpy() for planes in d_out for p in planes], state, stats

    def one_by_one(rt, ins, outs):
        for a, b in zip(ins, outs):
            rt.process_frame(a, b)

    want, want_state, _ = run(one_by_one)
    got, state, stats = run(lambda rt, ins, outs: rt.process_frames(ins, outs))
    assert all(np.array_equal(g, e) for g, e in zip(got, want)) and np.array_equal(state, want_state)
    assert stats == (3, 3)


def test_a_flow_free_models_pass_encodes_each_frames_own_state():
    """One scratch state that every frame of the pass overwrites: the encode of frame i runs in front of frame i + 1."""
    cfg, wts = flow_free(small_config())
    blob = blob_of(cfg, wts)
    h, w = cfg.frame_height, cfg.frame_width
    specs = [Spec(P010 if t % 2 else I010, 2, "host" if t < 4 else "device", "plain", P010 if t % 3 else I010, 2,
                  "host" if t < 4 else "device", "bottom-up") for t in range(8)]
    frames = M.synthetic_frames(8, h, w, seed=3, kind="noise")
    want, _ = twin_bytes(blob, R.DTYPE_F16, frames, specs)
    for i in range(7):
        assert not np.array_equal(want[i][0], want[i + 1][0])
    ins, outs = make_sides(frames, specs, h, w)
    with R.Runtime(blob, 0, R.DTYPE_F16) as rt:
        for _ in range(3):                                      # eager, captured, replayed
            run_calls(rt, ins, outs, want, (8,))
        assert rt.stat("lookahead_yuv_frames") == 24 and rt.stat("lookahead_frames") == 24


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_runtime_unchanged():
    torch, dev = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    frames = M.synthetic_frames(4, h, w, seed=2, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        held = source(frames[0], P010, cs)
        good_in = R.host_frame(P010, held, cs)
        pout = blank_planes(I010, 4 * h, 4 * w)
        good_out = R.host_frame(I010, pout, cs)

        def bad(frame, **kw):
            f = R.JuFrame()
            C.memmove(C.addressof(f), C.addressof(frame), C.sizeof(f))
            for k, val in kw.items():
                if k == "plane":
                    f.planes[val[0]] = val[1]
                elif k == "stride":
                    f.strides[val[0]] = val[1]
                else:
                    setattr(f, k, val)
            return f
        cases = {
            "odd pointer": (bad(good_in, plane=(0, good_in.planes[0] + 1)), good_out, "multiples of 2"),
            "odd stride": (bad(good_in, stride=(1, 2 * w + 1)), good_out, "multiples of 2"),
            "odd output stride": (good_in, bad(good_out, stride=(2, 4 * w + 1)), "multiples of 2"),
            "short stride": (bad(good_in, stride=(0, 2 * w - 2)), good_out, "stride"),
            "8-bit stride for a 10-bit plane": (bad(good_in, stride=(0, w)), good_out, "stride"),
            "NULL plane": (bad(good_in, plane=(1, None)), good_out, "NULL"),
            "NULL third plane": (good_in, bad(good_out, plane=(2, None)), "NULL"),
            "odd size": (bad(good_in, width=w - 1), good_out, "even"),
            "graphics resource": (bad(good_in, location=R.LOC_GRAPHICS_RESOURCE), good_out, "graphics"),
            "unknown format": (bad(good_in, format=7), good_out, "format"),
            "unknown format 5": (good_in, bad(good_out, format=5), "format"),
        }
        for name, (fi, fo, words) in cases.items():
            with pytest.raises(R.JoshUpscaleError) as e:
                a.process_frame(fi, fo)
            assert e.value.code == 1 and words in e.value.message, (name, e.value.message)
            assert "JU_" not in e.value.message
        with pytest.raises(R.JoshUpscaleError) as e:            # a host frame handed to ju_enqueue_frame
            a.enqueue_frame(good_in, good_out)
        assert e.value.code == 1 and "device" in e.value.message
        # a bad frame in the middle of a ju_process_frames call is named by its index
        held_all = [source(f, P010, cs) for f in frames]        # (kept alive: the frames hold raw pointers)
        ins = [R.host_frame(P010, p, cs) for p in held_all]
        keep = [blank_planes(I010, 4 * h, 4 * w) for _ in frames]
        outs = [R.host_frame(I010, p, cs) for p in keep]
        with pytest.raises(R.JoshUpscaleError) as e:
            a.process_frames([ins[0], ins[1], bad(ins[2], stride=(0, 2 * w + 1)), ins[3]], outs)
        assert e.value.code == 1 and "frame 2" in e.value.message and "multiples of 2" in e.value.message
        assert all((p == 0).all() for planes in keep for p in planes) and (pout[0] == 0).all()
        # nothing ran: the stream goes on as its twin's
        for f in frames:
            got = a.process_yuv(*source(f, I010, cs), R.FMT_I010, cs)
            frame = b.process_image(decoded(I010, cs, source(f, I010, cs)))
            for g, e2 in zip(got, expect_planes(I010, cs, frame, state_of(b, h, w))):
                assert np.array_equal(g, e2)
        del held, held_all


# ---- 8. full size -----------------------------------------------------------------------------------------------------
def test_full_size_device_p010_in_and_out():
    """psp-quality bf16, 480 x 270 -> 1920 x 1080, device P010 planes both ways, the encode from the state."""
    torch, dev = torch_dev()
    cfg = M.PRESETS["psp-quality"]
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        assert a.stat("hbd_from_state") == 1
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=9, kind="smooth")):
            held = source(f, P010, cs)
            d_in = [torch.from_numpy(p.view(np.int16)).to(dev) for p in held]
            blank = blank_planes(P010, 4 * h, 4 * w)
            d_out = [torch.zeros(p.shape, dtype=torch.int16, device=dev) for p in blank]
            torch.cuda.synchronize()
            a.process_frame(R.device_frame(P010, w, h, d_in, colorspace=cs),
                            R.device_frame(P010, 4 * w, 4 * h, d_out, colorspace=cs))
            got = [d.cpu().numpy().view(np.uint16) for d in d_out]
            frame8 = b.process_image(decoded(P010, cs, held))
            want = expect_planes(P010, cs, None, state_of(a, h, w))
            for g, e in zip(got, want):
                assert np.array_equal(g, e), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t
            lo, hi = y10_against_y8(got[0] >> 6, Y.encode(frame8, cs)[0])    # (the relation derived above)
            assert -2 <= lo and hi <= 6, (lo, hi)
