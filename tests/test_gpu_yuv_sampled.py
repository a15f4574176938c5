"""4:2:2 and 4:4:4 frame I/O on the GPU (YUY2, UYVY, I422, P210, I210, I444, I410; csrc/colour_kernels.hip, engine_frames.cpp):
the conversion kernels alone against the numpy definition (tests/yuv_sampled_reference.py), byte for byte; inputs
against a twin fed the decoded frame; outputs against the definition applied to the twin's frame or to the runtime's own
f16 state; formats, locations and layouts on both sides; look-ahead passes against a twin driven frame by frame; the
source stage; odd geometry; the refused calls."""

import ctypes as C
import dataclasses

import numpy as np
import pytest

import source_reference as SRC
import yuv10_reference as T
import yuv_reference as Y
import yuv_sampled_reference as S
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_yuv import CSS, DevPlane, torch_dev
from test_gpu_yuv import LAYOUTS as LAYOUTS8
from test_gpu_yuv10 import LAYOUTS as LAYOUTS10
from test_gpu_yuv10 import Side, as_bytes, blob_of, random_state, state_of, tensors_equal

pytestmark = pytest.mark.gpu

BGRX, I420, NV12, P010, I010 = 0, 1, 2, 3, 4
YUY2, UYVY, I422, P210, I210, I444, I410 = S.NEW_FORMATS
NEW = S.NEW_FORMATS
NEW10 = (P210, I210, I410)
NAMES = dict(S.FORMAT_NAMES)
NAMES[BGRX] = "bgrx"
name_of = lambda f: NAMES[f]  # noqa: E731


def blank(fmt, h, w):
    return [np.zeros((h, w, 4), np.uint8)] if fmt == BGRX else S.blank_planes(fmt, h, w)


def decoded(fmt, cs, planes):
    """The BGRX frame the network consumes for the caller's planes."""
    return planes[0] if fmt == BGRX else S.decode_planes(fmt, cs, planes)


def expect(fmt, cs, frame, state):
    """What a runtime writes for an output of the format: from its 8-bit frame, or -- a 10-bit format with a state
    given -- from the state."""
    return [frame] if fmt == BGRX else S.encode_planes(fmt, cs, frame=frame, state=state)


def source(frame, fmt, cs):
    """The planes of one input frame of a BGRX clip in the given format."""
    return [frame] if fmt == BGRX else S.encode_planes(fmt, cs, frame=frame)


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, e) for g, e in zip(got, want))


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------
SIZES = {422: [(2, 2), (1, 2), (23, 30), (18, 100), (64, 1920)],
         444: [(2, 2), (1, 1), (23, 30), (23, 17), (3, 33), (18, 100), (64, 1920)]}
KINDS = ("random", "zero", "full", "extreme", "junk")
KERNEL_CASES = [(f, lay) for f in NEW for lay in sorted(LAYOUTS10 if f in S.DEEP else LAYOUTS8)]


def run_debug(op, fmt, cs, w, h, image_ptr, image_stride, planes):
    lib = R.load_library(True)
    ptrs = (C.c_void_p * 3)(*([p.ptr for p in planes] + [None] * (3 - len(planes))))
    strides = (C.c_ssize_t * 3)(*([p.stride for p in planes] + [0] * (3 - len(planes))))
    rc = lib.ju_debug_yuv_sampled(op, fmt, cs, w, h, image_ptr, image_stride, ptrs, strides)
    assert rc == 0, lib.ju_last_error()


def content(kind, fmt, h, w, rng):
    """(y, u, v) samples of a frame of the format."""
    top, dt = (1024, np.uint16) if fmt in S.DEEP else (256, np.uint8)
    cshape = S.chroma_shape(S.SAMPLING[fmt], h, w)
    shapes = ((h, w), cshape, cshape)
    if kind in ("random", "junk"):
        return [rng.integers(0, top, s, dtype=dt) for s in shapes]
    if kind == "zero":
        return [np.zeros(s, dt) for s in shapes]
    if kind == "full":
        return [np.full(s, top - 1, dt) for s in shapes]
    cb = (np.indices(cshape).sum(0) % 2 * (top - 1)).astype(dt)   # extreme chroma in a checkerboard of samples
    return [rng.integers(0, top, shapes[0], dtype=dt), cb, ((top - 1) - cb).astype(dt)]


def with_junk(fmt, planes, rng):
    """Random bits where a 10-bit format ignores them: P210's low 6, I210's and I410's high 6."""
    shift = 0 if fmt == P210 else 10
    return [p | (rng.integers(0, 64, p.shape, dtype=np.uint16) << shift) for p in planes]


@pytest.mark.parametrize("fmt,layout", KERNEL_CASES, ids=[f"{NAMES[f]}-{lay}" for f, lay in KERNEL_CASES])
def test_kernels_equal_the_numpy_definition(fmt, layout):
    torch, dev = torch_dev()
    rng = np.random.default_rng(7 + fmt)
    deep = fmt in S.DEEP
    sampling = S.SAMPLING[fmt]
    lay = (LAYOUTS10 if deep else LAYOUTS8)[layout]
    img_lay = dict(pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
    for n, (h, w) in enumerate(SIZES[sampling]):
        # every colour space on random content, the other contents in one colour space each (all four over the sizes)
        cases = [("random", cs) for cs in CSS] + [(kind, CSS[(n + i) % 4]) for i, kind in enumerate(KINDS[1:])]
        for kind, cs in cases:
            if kind == "junk" and not deep:
                continue                                        # (an 8-bit format ignores no bits)
            y, u, v = content(kind, fmt, h, w, rng)
            held = S.to_words(fmt, y, u, v)
            if kind == "junk":
                held = with_junk(fmt, held, rng)
            # decode: planes -> BGRX
            src = [DevPlane(as_bytes(p), **lay) for p in held]
            out = DevPlane(np.zeros((h, w, 4), np.uint8), **img_lay)
            run_debug(0, fmt, cs, w, h, out.ptr, out.stride, src)
            out.check(S.decode(y, u, v, cs, sampling, deep))
            for p, d in zip(src, held):
                p.check(as_bytes(d))                            # (inputs untouched)
            if kind == "junk":
                continue
            # encode from a u8 frame (X random: ignored) -> planes
            bgrx = rng.integers(0, 256, (h, w, 4), dtype=np.uint8) if kind == "random" else \
                S.decode(y, u, v, cs, sampling, deep)
            inb = DevPlane(bgrx, **img_lay)
            want = S.encode_planes(fmt, cs, frame=bgrx)
            dst = [DevPlane(as_bytes(np.zeros_like(p)), **lay) for p in want]
            run_debug(1, fmt, cs, w, h, inb.ptr, inb.stride, dst)
            for p, e in zip(dst, want):
                p.check(as_bytes(e))
            inb.check(bgrx)
            if not deep:
                continue
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
            want = S.encode_planes(fmt, cs, state=state)
            dst = [DevPlane(as_bytes(np.zeros_like(p)), **lay) for p in want]
            run_debug(2, fmt, cs, w, h, d_state.data_ptr(), 0, dst)
            for p, e in zip(dst, want):
                p.check(as_bytes(e))
            assert np.array_equal(d_state.cpu().numpy().view(np.uint16), state.view(np.uint16))


# ---- 2. the items kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [(YUY2, I420, P210, I444, I010, I410, NV12, UYVY), (I422, P010, I210, I444, I410, UYVY, NV12, P210)],
                         ids=["a", "b"])
def test_items_kernel_decodes_every_sampling_and_depth_in_one_launch(mix):
    lib = R.load_library(True)
    rng = np.random.default_rng(21)
    names8, names10 = sorted(LAYOUTS8), sorted(LAYOUTS10)
    for (h, w) in [(46, 30), (18, 100)]:
        fmts, css, outs, srcs, want, held_all = [], [], [], [], [], []
        for i, fmt in enumerate(mix):
            deep = fmt in S.DEEP
            lay = LAYOUTS10[names10[i % len(names10)]] if deep else LAYOUTS8[names8[i % len(names8)]]
            held = S.to_words(fmt, *content("random", fmt, h, w, rng))
            if deep:
                shift = 0 if fmt in (P010, P210) else 10
                held = [p | (rng.integers(0, 64, p.shape, dtype=np.uint16) << shift) for p in held]
            fmts.append(fmt)
            css.append(CSS[i % 4])
            held_all.append(held)
            want.append(S.decode_planes(fmt, css[-1], held))
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
        for i, (o, e) in enumerate(zip(outs, want)):
            o.check(e)
            # per item the single kernel's bytes (the new formats; the 4:2:0 ones are held to theirs by the existing tests)
            if fmts[i] in NEW:
                single = DevPlane(np.zeros((h, w, 4), np.uint8))
                run_debug(0, fmts[i], css[i], w, h, single.ptr, single.stride, srcs[i])
                single.check(e)
            for p, d in zip(srcs[i], held_all[i]):
                p.check(as_bytes(d))


# ---- 3. inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [pytest.param(R.DTYPE_F16, id="fp16"), pytest.param(R.DTYPE_BF16, id="bf16")])
@pytest.mark.parametrize("fmt", NEW, ids=name_of)
def test_input_equals_process_of_the_decoded_frame(fmt, dtype):
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = CSS[fmt % 4]
    rng = np.random.default_rng(3)
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=3, kind="smooth")):
            held = source(f, fmt, cs)
            if t % 2 and fmt in NEW10:
                held = with_junk(fmt, held, rng)
            got = np.zeros((4 * h, 4 * w, 4), np.uint8)
            a.process_frame(R.host_frame(fmt, held, cs), R.host_frame(R.FMT_BGRX, [got]))
            want = b.process_image(decoded(fmt, cs, held))
            assert np.array_equal(got, want), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


# ---- 4. outputs: which source, and its bytes -------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NEW, ids=name_of)
def test_output_equals_the_definition(fmt):
    """8-bit formats: the definition applied to the twin's BGRX output; 10-bit formats: to the runtime's own f16 state."""
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = CSS[(fmt + 1) % 4]
    dtype = R.DTYPE_F16 if fmt % 2 else R.DTYPE_BF16
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        assert a.stat("hbd_from_state") == 1
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=8, kind="smooth")):
            got = blank(fmt, 4 * h, 4 * w)
            a.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(fmt, got, cs))
            frame = b.process_image(f)
            want = expect(fmt, cs, frame, state_of(a, h, w) if fmt in NEW10 else None)
            assert same(got, want), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


@pytest.mark.parametrize("variant", ["brightness", "output-flow"])
@pytest.mark.parametrize("fmt", NEW10, ids=name_of)
def test_models_whose_state_is_not_the_frame_encode_from_the_8_bit_frame(fmt, variant):
    if variant == "brightness":
        cfg = small_config(normalize_brightness=True)
        blob = blob_of(cfg)
    else:
        cfg = small_config()
        blob = M.serialize(*M.output_flow(cfg, M.make_seeded_weights(cfg)))
    h, w = cfg.frame_height, cfg.frame_width
    cs = CSS[fmt % 4]
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        assert a.stat("hbd_from_state") == 0
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=11, kind="smooth")):
            got = blank(fmt, 4 * h, 4 * w)
            a.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(fmt, got, cs))
            frame = b.process_image(f)
            assert same(got, expect(fmt, cs, frame, None)), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


def test_i410_output_of_a_plain_model_carries_the_frame():
    """A plain model's I410 planes, decoded on the CPU to D, against the runtime's state (P = p_from_state) and the twin's
    8-bit frame u8.  Nothing is resampled in 4:4:4, so every statement is per pixel and channel:

    (a) where P = 257 u8 in all three channels -- state and frame hold the same value -- D = u8 exactly: the chain is
        decode10(encode10(257 u8)), which returns every 8-bit colour (tests/test_yuv_sampled_cpu.py);
    (b) everywhere |D - P / 257| <= 0.95.  The 10-bit rounding of Y, U and V is at most half a code each; through the
        decode's real coefficients (limited range, the larger ones: 255 / 876 = 0.291 for Y, 2 (1 - K_b) 255 / 896 =
        0.528 for U into B in BT.709) that is at most 0.146 + 0.264 = 0.41 of an 8-bit step, the coefficients' rounding
        to 2^-16 and 2^-32 adds less than 0.02, and the decode rounds to nearest: 0.5.  Sum below 0.95;
    (c) D - u8 is 0 or 1.  The frame is floor(255 t) of the tail's output t and the state holds t rounded to f16, which
        puts P / 257 - u8 in [-0.035, 1.035] (derived in tests/test_gpu_yuv10.py, test_10_bit_luma_lies_around_4_times_
        the_8_bit_luma); with (b), D - u8 lies in [-0.985, 1.985].  So the decode never falls below the frame, and is
        one above where the state's fraction rounds up -- the frame truncates, the decode rounds: equality with the
        frame is NOT claimed there."""
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    for cs in (Y.CS_BT709_LIMITED, Y.CS_BT601_FULL):
        with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
            for f in M.synthetic_frames(3, h, w, seed=14, kind="smooth"):
                got = blank(I410, 4 * h, 4 * w)
                a.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(I410, got, cs))
                u8 = b.process_image(f)[..., :3].astype(np.int64)
                assert all(int(p.max()) <= 1023 for p in got)
                p = T.p_from_state(state_of(a, h, w))
                d = S.decode_planes(I410, cs, got)[..., :3].astype(np.int64)
                agree = (p == 257 * u8).all(axis=-1)
                err = np.abs(257 * d - p).max() / 257.0
                diff = d - u8
                print("I410:", cs, "pixels with P = 257 u8:", int(agree.sum()), "max |D - P / 257|:", err,
                      "D - u8 in", int(diff.min()), int(diff.max()))
                assert np.array_equal(d[agree], u8[agree])
                assert err <= 0.95
                assert diff.min() >= 0 and diff.max() <= 1


# ---- 5. pairs and places ------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Spec:
    fin: int
    cin: int
    lin: str
    layin: str
    fout: int
    cout: int
    lout: str
    layout: str


OLD = (NV12, I420, P010, I010)
LAYS = ("plain", "padded", "bottom-up")


def places():
    """Four frames per new format f: f as a host and as a device input, as a host and as a device output; over the four
    its planes are dense, padded and bottom-up; its partners are BGRX, an old format (on either side) and a new one."""
    specs = []
    for i, f in enumerate(NEW):
        lay = [LAYS[(i + j) % 3] for j in range(5)]
        cs = [(i + j) % 4 for j in range(5)]
        specs += [Spec(f, cs[0], "host", lay[0], OLD[(i + 1) % 4] if i % 2 else BGRX, cs[1], "device" if i % 4 < 2 else "host", lay[1]),
                  Spec(f, cs[1], "device", lay[1], NEW[(i + 2) % 7], cs[2], "device", lay[2]),
                  Spec(OLD[i % 4], cs[2], "device" if i % 2 else "host", lay[3], f, cs[3], "host", lay[2]),
                  Spec(BGRX, 0, "device", lay[4], f, cs[0], "device", lay[3])]
    return specs


PLACES = places()


def test_every_new_format_on_each_side_in_host_and_device_memory():
    for f in NEW:                                               # what the table must hold, per format
        name = NAMES[f]
        mine = [(s.lin, s.layin, s.fout) for s in PLACES if s.fin == f] + [(s.lout, s.layout, s.fin) for s in PLACES if s.fout == f]
        assert {s.lin for s in PLACES if s.fin == f} == {"host", "device"}, name      # each side in both kinds of memory
        assert {s.lout for s in PLACES if s.fout == f} == {"host", "device"}, name
        assert {lay for _, lay, _ in mine} == set(LAYS), name                          # dense, padded, bottom-up
        assert BGRX in {other for _, _, other in mine}, name                           # paired with BGRX,
        assert {other for _, _, other in mine} & set(OLD), name                        # with an old format
        assert {other for _, _, other in mine} & set(NEW), name                        # and with a new one
    # (and over the table an old format stands on either side of a new one)
    assert {s.fout for s in PLACES if s.fin in NEW} & set(OLD) and {s.fin for s in PLACES if s.fout in NEW} & set(OLD)
    torch, _ = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(len(PLACES), h, w, seed=4, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        for t, (f, s) in enumerate(zip(frames, PLACES)):
            held = source(f, s.fin, s.cin)
            sin = Side(s.fin, s.cin, s.lin, s.layin, held, w, h)
            sout = Side(s.fout, s.cout, s.lout, s.layout, blank(s.fout, 4 * h, 4 * w), 4 * w, 4 * h)
            torch.cuda.synchronize()
            if s.lin == "device" and s.lout == "device" and t % 2:
                a.enqueue_frame(sin.frame, sout.frame)
                a.synchronize()
            else:
                a.process_frame(sin.frame, sout.frame)
            frame = b.process_image(decoded(s.fin, s.cin, held))
            sout.check(expect(s.fout, s.cout, frame, state_of(b, h, w) if s.fout in S.DEEP else None))
            sin.check(held)                                     # (inputs and their guards untouched)
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


# ---- 6. look-ahead passes -----------------------------------------------------------------------------------------------
def twin_bytes(blob, dtype, frames, specs):
    """What ju_process_frame, called frame by frame on plain host frames, writes; + the state and the history."""
    cfg, _ = M.deserialize(blob)
    h, w = cfg.frame_height, cfg.frame_width
    want = []
    with R.Runtime(blob, 0, dtype) as rt:
        for f, s in zip(frames, specs):
            pout = blank(s.fout, 4 * h, 4 * w)
            pin = source(f, s.fin, s.cin)                       # (kept alive: the frame holds raw pointers)
            rt.process_frame(R.host_frame(s.fin, pin, s.cin), R.host_frame(s.fout, pout, s.cout))
            want.append(pout)
        tensors = [rt.read_tensor(n).copy() for n in ("state", "flow_in")]
    return want, tensors


def make_sides(frames, specs, h, w):
    ins = [Side(s.fin, s.cin, s.lin, s.layin, source(f, s.fin, s.cin), w, h) for f, s in zip(frames, specs)]
    outs = [Side(s.fout, s.cout, s.lout, s.layout, blank(s.fout, 4 * h, 4 * w), 4 * w, 4 * h) for s in specs]
    torch_dev()[0].cuda.synchronize()
    return ins, outs


def run_calls(rt, ins, outs, want, lengths):
    t = 0
    for k in lengths:
        rt.process_frames([x.frame for x in ins[t:t + k]], [x.frame for x in outs[t:t + k]])
        for i in range(t, t + k):
            outs[i].check(want[i])
        t += k


PASS_SPECS = PLACES[:12]


def test_passes_mixing_new_and_old_formats_give_the_frame_by_frame_bytes():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    specs = PASS_SPECS
    frames = M.synthetic_frames(len(specs), h, w, seed=19, kind="smooth")
    want, tensors = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        run_calls(rt, ins, outs, want, (7, 5))
        assert tensors_equal(rt, tensors)
        assert rt.stat("lookahead_frames") == 12 and rt.stat("lookahead_yuv_frames") == 12
        assert rt.stat("fallbacks") == 0
        hosts = sum(1 for s in specs if "host" in (s.lin, s.lout))
        assert rt.stat("lookahead_host_frames") == hosts
        for i in ins:                                           # (inputs and their guards untouched)
            i.check([p._rows(p.host) for p in i.planes])
        # the same buffers again: captured at the second use, replayed at the third, same bytes
        for _ in range(2):
            rt.reset()
            run_calls(rt, ins, outs, want, (7, 5))
        assert tensors_equal(rt, tensors) and rt.stat("graph_replays") >= 2


def test_a_pass_that_is_run_again_gives_the_same_planes():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    specs = [Spec(YUY2, 2, "host", "bottom-up", I410, 2, "host", "padded") for _ in range(3)] + \
            [Spec(I444, 1, "device", "padded", P210, 3, "device", "plain") for _ in range(3)] + \
            [Spec(I210, 0, "device", "plain", UYVY, 1, "host", "plain") for _ in range(2)]
    frames = M.synthetic_frames(len(specs), h, w, seed=7, kind="smooth")
    want, tensors = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        assert lib.ju_debug_set(b"pass_rerun", 1) == 0
        try:
            run_calls(rt, ins, outs, want, (5, 3))
        finally:
            lib.ju_debug_set(b"pass_rerun", 0)
        assert rt.stat("lookahead_frames") == 0 and rt.stat("lookahead_yuv_frames") == 0 and rt.stat("fallbacks") == 0
        assert tensors_equal(rt, tensors)


def test_a_packed_plane_over_an_earlier_input_plane_starts_a_new_pass():
    """Frame 1's output plane (YUY2: one plane of 2 bytes per pixel) lies over frame 0's input plane: frame 0 runs on its
    own and frames 1-3 as a pass, with the bytes of the frame-by-frame calls on the same buffers."""
    torch, dev = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    frames = M.synthetic_frames(4, h, w, seed=61, kind="smooth")
    src = [source(f, YUY2, cs) for f in frames]

    def run(call):
        arena = torch.zeros(2 * 16 * h * w, dtype=torch.uint8, device=dev)
        arena[: 2 * h * w] = torch.from_numpy(src[0][0].reshape(-1).copy()).to(dev)
        d_in = [torch.from_numpy(s[0].copy()).to(dev) for s in src]
        d_out = [torch.zeros((4 * h, 8 * w), dtype=torch.uint8, device=dev) for _ in frames]
        ins = [R.device_frame(YUY2, w, h, [arena], colorspace=cs)] + \
              [R.device_frame(YUY2, w, h, [d_in[t]], colorspace=cs) for t in (1, 2, 3)]
        outs = [R.device_frame(YUY2, 4 * w, 4 * h, [d_out[0]], colorspace=cs),
                R.device_frame(YUY2, 4 * w, 4 * h, [arena], colorspace=cs)] + \
               [R.device_frame(YUY2, 4 * w, 4 * h, [d_out[t]], colorspace=cs) for t in (2, 3)]
        torch.cuda.synchronize()
        with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
            call(rt, ins, outs)
            stats = (rt.stat("lookahead_frames"), rt.stat("lookahead_yuv_frames"))
            state = rt.read_tensor("state").copy()
        return [arena.cpu().numpy()] + [p.cpu().numpy() for p in d_out], state, stats

    def one_by_one(rt, ins, outs):
        for a, b in zip(ins, outs):
            rt.process_frame(a, b)

    want, want_state, _ = run(one_by_one)
    got, state, stats = run(lambda rt, ins, outs: rt.process_frames(ins, outs))
    assert same(got, want) and np.array_equal(state, want_state)
    assert stats == (3, 3)


# ---- 7. the source stage ------------------------------------------------------------------------------------------------
SRC_H, SRC_W = 60, 96


@pytest.mark.parametrize("fmt", [YUY2, I444], ids=name_of)
def test_a_scaled_source_is_decoded_at_source_size_then_scaled(fmt):
    torch, dev = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    clip = M.synthetic_frames(3, SRC_H, SRC_W, seed=5, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(SRC_W, SRC_H)
        for location in ("host", "device"):
            for t, f in enumerate(clip):
                planes = source(f, fmt, cs)
                want = b.process_image(SRC.scale(decoded(fmt, cs, planes), h, w))
                got = np.zeros((4 * h, 4 * w, 4), np.uint8)
                if location == "host":
                    f_in = R.host_frame(fmt, planes, cs)
                else:
                    held = [torch.from_numpy(p.copy()).to(dev) for p in planes]
                    torch.cuda.synchronize()
                    f_in = R.device_frame(fmt, SRC_W, SRC_H, held, colorspace=cs)
                a.process_frame(f_in, R.host_frame(R.FMT_BGRX, [got]))
                assert np.array_equal(got, want), (location, t)
                assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))
        assert a.stat("source_stage_frames") == 6


def test_a_masked_p210_output_comes_from_the_blended_8_bit_frame():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    rng = np.random.default_rng(2)
    mask = rng.integers(0, 256, (37, 50, 4), dtype=np.uint8)
    kind = rng.integers(0, 3, (37, 50))
    mask[kind == 0, :3] = 255
    mask[kind == 1, :3] = 0
    clip = M.synthetic_frames(2, SRC_H, SRC_W, seed=9, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(SRC_W, SRC_H)
        a.set_source_mask(mask)
        assert a.stat("hbd_from_state") == 1
        for t, f in enumerate(clip):
            planes = source(f, UYVY, cs)
            src = decoded(UYVY, cs, planes)
            plain = b.process_image(SRC.scale(src, h, w))
            want = SRC.blend(plain, src, mask)
            assert (want != plain).any()
            got = blank(P210, 4 * h, 4 * w)
            a.process_frame(R.host_frame(UYVY, planes, cs), R.host_frame(P210, got, cs))
            assert same(got, expect(P210, cs, want, None)), t
        assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))
        # without the mask the P210 output comes from the f16 state again
        a.set_source_mask(None)
        planes = source(clip[0], UYVY, cs)
        b.process_image(SRC.scale(decoded(UYVY, cs, planes), h, w))
        got = blank(P210, 4 * h, 4 * w)
        a.process_frame(R.host_frame(UYVY, planes, cs), R.host_frame(P210, got, cs))
        assert same(got, expect(P210, cs, None, state_of(b, h, w)))


# ---- 8. odd geometry through a model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,fin,fout", [((15, 23), I444, I410), ((15, 23), I410, I444), ((15, 24), YUY2, P210),
                                           ((15, 24), P210, YUY2)],
                         ids=["15x23-i444-i410", "15x23-i410-i444", "15x24-yuy2-p210", "15x24-p210-yuy2"])
def test_odd_geometry_through_a_model(size, fin, fout):
    torch, dev = torch_dev()
    h, w = size
    cfg = small_config(frame_height=h, frame_width=w)
    blob = blob_of(cfg)
    cs = Y.CS_BT601_LIMITED
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=6, kind="smooth")):
            held = source(f, fin, cs)
            loc = "host" if t % 2 == 0 else "device"
            sin = Side(fin, cs, loc, "padded", held, w, h)
            sout = Side(fout, cs, loc, "bottom-up", blank(fout, 4 * h, 4 * w), 4 * w, 4 * h)
            torch.cuda.synchronize()
            a.process_frame(sin.frame, sout.frame)
            frame = b.process_image(decoded(fin, cs, held))
            sout.check(expect(fout, cs, frame, state_of(b, h, w) if fout in S.DEEP else None))
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


# ---- 9. refusals --------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_runtime_unchanged():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    cs = Y.CS_BT709_LIMITED
    frames = M.synthetic_frames(4, h, w, seed=2, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        held_yuy2 = source(frames[0], YUY2, cs)
        held_p210 = source(frames[0], P210, cs)
        in_yuy2 = R.host_frame(YUY2, held_yuy2, cs)
        in_p210 = R.host_frame(P210, held_p210, cs)
        pout = blank(I410, 4 * h, 4 * w)
        good_out = R.host_frame(I410, pout, cs)
        pout422 = blank(I422, 4 * h, 4 * w)
        out_i422 = R.host_frame(I422, pout422, cs)

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
            "odd width for 4:2:2": (bad(in_yuy2, width=w - 1), good_out, "even width"),
            "odd output width for 4:2:2": (in_yuy2, bad(out_i422, width=4 * w - 1), "even width"),
            "odd address": (bad(in_p210, plane=(0, in_p210.planes[0] + 1)), good_out, "multiples of 2"),
            "odd stride": (bad(in_p210, stride=(1, 2 * w + 1)), good_out, "multiples of 2"),
            "odd output stride": (in_yuy2, bad(good_out, stride=(2, 8 * w + 1)), "multiples of 2"),
            "short packed stride": (bad(in_yuy2, stride=(0, 2 * w - 1)), good_out, "stride"),
            "a luma stride for a packed plane": (bad(in_yuy2, stride=(0, w)), good_out, "stride"),
            "short negative stride": (bad(in_yuy2, stride=(0, -(2 * w - 2))), good_out, "stride"),
            "short 4:4:4 chroma stride": (in_yuy2, bad(good_out, stride=(1, 4 * w)), "stride"),
            "NULL plane": (bad(in_p210, plane=(1, None)), good_out, "NULL"),
            "NULL packed plane": (bad(in_yuy2, plane=(0, None)), good_out, "NULL"),
            "NULL third plane": (in_yuy2, bad(good_out, plane=(2, None)), "NULL"),
            "graphics resource": (bad(in_yuy2, location=R.LOC_GRAPHICS_RESOURCE), good_out, "graphics"),
            "graphics resource output": (in_yuy2, bad(good_out, location=R.LOC_GRAPHICS_RESOURCE), "graphics"),
            "wrong size": (in_yuy2, bad(good_out, height=4 * h - 1), "exactly"),
        }
        for value in list(range(5, 16)) + [21, 22, 23, 26]:
            cases[f"unknown input format {value}"] = (bad(in_yuy2, format=value), good_out, "format")
            cases[f"unknown output format {value}"] = (in_yuy2, bad(good_out, format=value), "format")
        for name, (fi, fo, words) in cases.items():
            with pytest.raises(R.JoshUpscaleError) as e:
                a.process_frame(fi, fo)
            assert e.value.code == 1 and words in e.value.message, (name, e.value.message)
            assert "JU_" not in e.value.message
        # a bad frame in the middle of a ju_process_frames call is named by its index
        held_all = [source(f, YUY2, cs) for f in frames]        # (kept alive: the frames hold raw pointers)
        ins = [R.host_frame(YUY2, p, cs) for p in held_all]
        keep = [blank(I410, 4 * h, 4 * w) for _ in frames]
        outs = [R.host_frame(I410, p, cs) for p in keep]
        with pytest.raises(R.JoshUpscaleError) as e:
            a.process_frames([ins[0], ins[1], bad(ins[2], width=w + 1), ins[3]], outs)
        assert e.value.code == 1 and "frame 2" in e.value.message
        assert all((p == 0).all() for planes in keep for p in planes) and all((p == 0).all() for p in pout + pout422)
        # nothing ran: the stream goes on as its twin's.  Planes beyond a format's count are not read: the packed frame
        # carries junk in planes[1] and strides[2]
        for f in frames:
            held = source(f, UYVY, cs)
            got = blank(I410, 4 * h, 4 * w)
            a.process_frame(bad(R.host_frame(UYVY, held, cs), plane=(1, 12345), stride=(2, 7)), R.host_frame(I410, got, cs))
            frame = b.process_image(decoded(UYVY, cs, held))
            assert same(got, expect(I410, cs, frame, state_of(b, h, w)))
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))
        del held_yuy2, held_p210, held_all
