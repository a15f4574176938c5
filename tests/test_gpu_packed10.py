"""Packed 10-bit frame formats on the GPU (V210, Y210, Y410, X2RGB10, X2BGR10; csrc/colour_kernels.hip): the conversion
kernels alone against the numpy definition (tests/packed10_reference.py), bit for bit, at the widths where a partial group,
a thread boundary or a clamped neighbour can go wrong; the items kernel; inputs against a twin fed the decoded frame;
outputs against the definition applied to the runtime's own f16 state; look-ahead passes against a twin driven frame by
frame; the source and the output stage; the refused calls."""

import ctypes as C

import numpy as np
import pytest

import output_reference as O
import packed10_reference as P
import source_reference as SRC
import test_gpu_rgb as RG
import yuv10_reference as T
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_rgb import Side, Spec
from test_gpu_yuv import CSS, DevPlane, torch_dev
from test_gpu_yuv10 import LAYOUTS as LAYOUTS10
from test_gpu_yuv10 import as_bytes, blob_of, random_state, state_of, tensors_equal

pytestmark = pytest.mark.gpu

BGRX, I420, NV12, P010 = 0, 1, 2, 3
YUY2, P210, I410, RGB24, RGBP16 = 16, 19, 25, 33, 38
NEW = P.NEW_FORMATS
V210, Y210, Y410, X2RGB10, X2BGR10 = NEW
CS = R.CS_BT709_LIMITED
name_of = lambda f: P.FORMAT_NAMES.get(f) or RG.name_of(f)  # noqa: E731


def blank(fmt, h, w):
    return P.blank_planes(fmt, h, w) if fmt in NEW else RG.blank(fmt, h, w)


def decoded(fmt, cs, planes, w):
    """The BGRX frame the network consumes for the caller's planes."""
    return P.decode_planes(fmt, cs, planes, width=w) if fmt in NEW else RG.decoded(fmt, cs, planes)


def expect(fmt, cs, frame, state):
    """What a runtime writes for an output of the format: a deep format with a state given from the state, else from
    the 8-bit frame."""
    return P.encode_planes(fmt, cs, frame=frame, state=state) if fmt in NEW else RG.expect(fmt, cs, frame, state)


def source(frame, fmt, cs):
    """The planes of one input frame of a BGRX clip in the given format."""
    return P.encode_planes(fmt, cs, frame=frame) if fmt in NEW else RG.source(frame, fmt, cs)


def host(fmt, planes, w, cs=CS):
    return R.host_frame(fmt, planes, cs, width=w if fmt == V210 else None)


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(as_bytes(g), as_bytes(e)) for g, e in zip(got, want))


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------
# V210: 2 one pixel pair of one group; 4, 8, 46, 50 a partial last group (W mod 6 = 4 and 2); 6, 48 whole groups; 8 / 46 /
# 50 / 100 an odd count of groups (a thread's second group missing); 30, 100, 1920 several threads a row: the chroma
# neighbour across the thread boundary.  Y210 / Y410 / X2*: the 16-pixel strips -- 1, 2 and 17 (a strip of one pixel), 33,
# 100 (a partial last strip), 1920.
SIZES = {422: [(1, 2), (2, 4), (3, 6), (3, 8), (5, 46), (2, 48), (3, 50), (23, 30), (18, 100), (4, 1920)],
         444: [(1, 1), (2, 2), (3, 33), (23, 17), (18, 100), (4, 1920)]}
KINDS = ("random", "zero", "full", "extreme", "junk")
# planes of 32-bit words: word-aligned offsets only (the interface refuses others); Y210: 16-bit words, LAYOUTS10 as it is
LAYOUTS32 = {"dense": dict(pad=0, offset=0, flip=False), "padded": dict(pad=32, offset=0, flip=False),
             "bottom-up": dict(pad=16, offset=0, flip=True), "offset-4": dict(pad=12, offset=4, flip=False),
             "offset-8-bottom-up": dict(pad=4, offset=8, flip=True)}


def layouts(fmt):
    return LAYOUTS10 if fmt == Y210 else LAYOUTS32


KERNEL_CASES = [(f, lay) for f in NEW for lay in sorted(layouts(f))]


def run_debug(op, fmt, cs, w, h, image_ptr, image_stride, planes):
    lib = R.load_library(True)
    ptrs = (C.c_void_p * 3)(*([p.ptr for p in planes] + [None] * (3 - len(planes))))
    strides = (C.c_ssize_t * 3)(*([p.stride for p in planes] + [0] * (3 - len(planes))))
    rc = lib.ju_debug_packed10(op, fmt, cs, w, h, image_ptr, image_stride, ptrs, strides)
    assert rc == 0, lib.ju_last_error()


def content(kind, fmt, h, w, rng):
    """Three sample arrays of a frame of the format: (y, u, v) or (b, g, r)."""
    shapes = P.sample_shapes(fmt, h, w)
    if kind in ("random", "junk"):
        return [rng.integers(0, 1024, s, dtype=np.uint16) for s in shapes]
    if kind == "zero":
        return [np.zeros(s, np.uint16) for s in shapes]
    if kind == "full":
        return [np.full(s, 1023, np.uint16) for s in shapes]
    cb = (np.indices(shapes[1]).sum(0) % 2 * 1023).astype(np.uint16)   # extreme chroma in a checkerboard of samples
    return [rng.integers(0, 1024, shapes[0], dtype=np.uint16), cb, (1023 - cb).astype(np.uint16)]


def check_encode(op, fmt, cs, w, h, lay, image_ptr, image_stride, want):
    dst = [DevPlane(np.full_like(as_bytes(p), 0x77), **lay) for p in want]
    run_debug(op, fmt, cs, w, h, image_ptr, image_stride, dst)
    for p, e in zip(dst, want):
        p.check(as_bytes(e))                                    # (and the bytes between the row and the stride: guards)


@pytest.mark.parametrize("fmt,layout", KERNEL_CASES, ids=[f"{name_of(f)}-{lay}" for f, lay in KERNEL_CASES])
def test_kernels_equal_the_numpy_definition(fmt, layout):
    torch, dev = torch_dev()
    rng = np.random.default_rng(70 + fmt)
    lay = layouts(fmt)[layout]
    img_lay = dict(pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
    for n, (h, w) in enumerate(SIZES[P.SAMPLING.get(fmt, 444)]):
        # every colour space on random content, the other contents in one colour space each (all four over the sizes)
        cases = [("random", cs) for cs in CSS] + [(kind, CSS[(n + i) % 4]) for i, kind in enumerate(KINDS[1:])]
        for kind, cs in cases:
            samples = content(kind, fmt, h, w, rng)
            held = P.to_words(fmt, *samples)
            assert as_bytes(held[0]).shape[1] == P.row_bytes(fmt, w)
            if kind == "junk":
                held = P.junk(fmt, held, w, rng)
            # op 0: the plane -> BGRX
            src = [DevPlane(as_bytes(p), **lay) for p in held]
            out = DevPlane(np.full((h, w, 4), 0x77, np.uint8), **img_lay)
            run_debug(0, fmt, cs, w, h, out.ptr, out.stride, src)
            out.check(P.decode_planes(fmt, cs, P.to_words(fmt, *samples), width=w))
            for p, d in zip(src, held):
                p.check(as_bytes(d))                            # (inputs untouched)
            if kind == "junk":
                continue
            # op 1: a u8 frame (X random: ignored) -> the plane
            bgrx = rng.integers(0, 256, (h, w, 4), dtype=np.uint8) if kind == "random" else \
                P.decode_planes(fmt, cs, held, width=w)
            inb = DevPlane(bgrx, **img_lay)
            check_encode(1, fmt, cs, w, h, lay, inb.ptr, inb.stride, P.encode_planes(fmt, cs, frame=bgrx))
            inb.check(bgrx)
            # op 2: an f16 tensor -> the plane
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
            check_encode(2, fmt, cs, w, h, lay, d_state.data_ptr(), 0, P.encode_planes(fmt, cs, state=state))
            assert np.array_equal(d_state.cpu().numpy().view(np.uint16), state.view(np.uint16))
            # op 3: a u16 frame (the fourth lane random: unused) -> the plane
            if kind == "random":
                frame16 = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
            elif kind == "zero":
                frame16 = np.zeros((h, w, 4), np.uint16)
            elif kind == "full":
                frame16 = np.full((h, w, 4), 65535, np.uint16)
            else:
                frame16 = bgrx.astype(np.uint16) * 257
            d_frame = torch.from_numpy(frame16.view(np.int16)).to(dev)
            assert d_frame.data_ptr() % 8 == 0
            check_encode(3, fmt, cs, w, h, lay, d_frame.data_ptr(), 0, P.encode_planes(fmt, cs, frame16=frame16))
            assert np.array_equal(d_frame.cpu().numpy().view(np.uint16), frame16)


# ---- 2. the items kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [(V210, NV12, Y210, P210, Y410, I410, X2RGB10, X2BGR10),
                                 (I410, X2BGR10, V210, V210, NV12, Y410, P210, Y210)], ids=["a", "b"])
def test_items_kernel_decodes_new_and_old_formats_in_one_launch(mix):
    lib = R.load_library(True)
    rng = np.random.default_rng(41)
    for (h, w) in [(46, 30), (18, 100), (2, 8)]:
        fmts, css, outs, srcs, want, held_all = [], [], [], [], [], []
        for i, fmt in enumerate(mix):
            cs = i % 4
            if fmt in NEW:
                names = sorted(layouts(fmt))
                lay = layouts(fmt)[names[i % len(names)]]
                held = P.junk(fmt, P.to_words(fmt, *content("random", fmt, h, w, rng)), w, rng)
            else:
                names = sorted(LAYOUTS10)
                lay = LAYOUTS10[names[i % len(names)]]
                held = RG.source(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), fmt, cs)
            fmts.append(fmt)
            css.append(cs)
            held_all.append(held)
            want.append(decoded(fmt, cs, held, w))
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
            for p, d in zip(srcs[i], held_all[i]):
                p.check(as_bytes(d))


# ---- 3. through a small model -------------------------------------------------------------------------------------------
DTYPES = [pytest.param(R.DTYPE_F16, id="fp16"), pytest.param(R.DTYPE_BF16, id="bf16")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", NEW, ids=name_of)
def test_input_equals_process_of_the_decoded_frame(fmt, dtype):
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    rng = np.random.default_rng(3)
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=3, kind="smooth")):
            held = source(f, fmt, t % 4)
            if t % 2:
                held = P.junk(fmt, held, w, rng)                # (junk where the format ignores it)
            frame = decoded(fmt, t % 4, source(f, fmt, t % 4), w)
            got = np.zeros((4 * h, 4 * w, 4), np.uint8)
            a.process_frame(host(fmt, held, w, t % 4), R.host_frame(R.FMT_BGRX, [got]))
            want = b.process_image(frame)
            assert np.array_equal(got, want), t
            for name in ("state", "flow_in"):
                assert np.array_equal(a.read_tensor(name), b.read_tensor(name)), (t, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", NEW, ids=name_of)
def test_output_is_encoded_from_the_state(fmt, dtype):
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        assert a.stat("hbd_from_state") == 1
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=8, kind="smooth")):
            got = blank(fmt, 4 * h, 4 * w)
            a.process_frame(R.host_frame(R.FMT_BGRX, [f]), host(fmt, got, 4 * w, t % 4))
            frame = b.process_image(f)
            assert same(got, expect(fmt, t % 4, frame, state_of(a, h, w))), t
            assert not same(got, expect(fmt, t % 4, frame, None)), t   # (and that is not what the 8-bit frame would give)
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


@pytest.mark.parametrize("variant", ["brightness", "output-flow"])
@pytest.mark.parametrize("fmt", NEW, ids=name_of)
def test_models_whose_state_is_not_the_frame_encode_from_the_8_bit_frame(fmt, variant):
    if variant == "brightness":
        cfg = small_config(normalize_brightness=True)
        blob = blob_of(cfg)
    else:
        cfg = small_config()
        blob = M.serialize(*M.output_flow(cfg, M.make_seeded_weights(cfg)))
    h, w = cfg.frame_height, cfg.frame_width
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        assert a.stat("hbd_from_state") == 0
        for t, f in enumerate(M.synthetic_frames(2, h, w, seed=11, kind="smooth")):
            got = blank(fmt, 4 * h, 4 * w)
            a.process_frame(R.host_frame(R.FMT_BGRX, [f]), host(fmt, got, 4 * w))
            frame = b.process_image(f)
            assert same(got, expect(fmt, CS, frame, None)), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


def test_process_yuv_and_process_rgb_allocate_the_new_formats():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    f = M.synthetic_frames(1, h, w, seed=5, kind="smooth")[0]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        held = source(f, V210, CS)
        frame = b.process_image(decoded(V210, CS, held, w))
        state = state_of(b, h, w)
        (got,) = a.process_yuv(held[0], fmt=R.FMT_V210, width=w, out_format=R.FMT_Y410)
        assert got.dtype == np.uint32 and got.shape == (4 * h, 4 * w) and same([got], expect(Y410, CS, frame, state))
        a.reset()
        (got,) = a.process_yuv(held[0], fmt=R.FMT_V210, width=w)
        assert got.shape == (4 * h, R.v210_row_words(4 * w)) and same([got], expect(V210, CS, frame, state))
        a.reset()
        b.reset()
        held = source(f, X2BGR10, CS)
        frame = b.process_image(decoded(X2BGR10, CS, held, w))
        got = a.process_rgb(held[0], R.FMT_X2BGR10, out_format=R.FMT_X2RGB10)
        assert got.dtype == np.uint32 and same([got], expect(X2RGB10, CS, frame, state_of(b, h, w)))


# ---- 4. every format on each side, in host and device memory ----------------------------------------------------------------
LAYS = ("plain", "padded", "bottom-up")
OTHERS = (BGRX, NV12, I410, P010, YUY2, RGBP16)


def places():
    """Per new format f four frames: f as a host input, a device input, a host output and a device output, beside an old
    format or another new one on the other side, in changing layouts."""
    specs = []
    for i, f in enumerate(NEW):
        specs.append(Spec(f, "host", LAYS[i % 3], NEW[(i + 1) % 5], "device", LAYS[(i + 1) % 3], i % 4, (i + 1) % 4))
        specs.append(Spec(f, "device", LAYS[(i + 1) % 3], OTHERS[i % 6], "host", LAYS[(i + 2) % 3], (i + 2) % 4, i % 4))
        specs.append(Spec(OTHERS[(i + 3) % 6], "device", LAYS[(i + 2) % 3], f, "host", LAYS[i % 3], (i + 3) % 4, (i + 2) % 4))
        specs.append(Spec(NEW[(i + 2) % 5], "host", LAYS[i % 3], f, "device", LAYS[(i + 2) % 3], i % 4, (i + 3) % 4))
    return specs


PLACES = places()


def twin_bytes(blob, dtype, frames, specs):
    """What ju_process_frame, called frame by frame on plain host frames, writes; + the state and the history."""
    cfg, _ = M.deserialize(blob)
    h, w = cfg.frame_height, cfg.frame_width
    want = []
    with R.Runtime(blob, 0, dtype) as rt:
        for f, s in zip(frames, specs):
            pout = blank(s.fout, 4 * h, 4 * w)
            pin = source(f, s.fin, s.cin)                       # (kept alive: the frame holds raw pointers)
            rt.process_frame(host(s.fin, pin, w, s.cin), host(s.fout, pout, 4 * w, s.cout))
            want.append(pout)
        tensors = [rt.read_tensor(n).copy() for n in ("state", "flow_in")]
    return want, tensors


def make_sides(frames, specs, h, w):
    ins = [Side(s.fin, s.cin, s.lin, s.layin, source(f, s.fin, s.cin), w, h) for f, s in zip(frames, specs)]
    outs = [Side(s.fout, s.cout, s.lout, s.layout, blank(s.fout, 4 * h, 4 * w), 4 * w, 4 * h) for s in specs]
    torch_dev()[0].cuda.synchronize()
    return ins, outs


def test_every_new_format_on_each_side_in_host_and_device_memory():
    for f in NEW:
        assert {s.lin for s in PLACES if s.fin == f} == {"host", "device"}, name_of(f)
        assert {s.lout for s in PLACES if s.fout == f} == {"host", "device"}, name_of(f)
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(len(PLACES), h, w, seed=13, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        ins, outs = make_sides(frames, PLACES, h, w)
        for t, (f, s) in enumerate(zip(frames, PLACES)):
            a.process_frame(ins[t].frame, outs[t].frame)
            frame = b.process_image(decoded(s.fin, s.cin, source(f, s.fin, s.cin), w))
            outs[t].check(expect(s.fout, s.cout, frame, state_of(b, h, w)))
            ins[t].check([p._rows(p.host) for p in ins[t].planes])
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


# ---- 5. look-ahead passes -----------------------------------------------------------------------------------------------
def run_calls(rt, ins, outs, want, lengths):
    t = 0
    for k in lengths:
        rt.process_frames([x.frame for x in ins[t:t + k]], [x.frame for x in outs[t:t + k]])
        for i in range(t, t + k):
            outs[i].check(want[i])
        t += k


def test_passes_mixing_new_and_old_formats_give_the_frame_by_frame_bytes():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    specs = PLACES
    frames = M.synthetic_frames(len(specs), h, w, seed=19, kind="smooth")
    want, tensors = twin_bytes(blob, R.DTYPE_BF16, frames, specs)
    ins, outs = make_sides(frames, specs, h, w)
    with R.Runtime(blob, 0, R.DTYPE_BF16) as rt:
        run_calls(rt, ins, outs, want, (8, 7, 5))
        assert tensors_equal(rt, tensors)
        assert rt.stat("lookahead_frames") == 20 and rt.stat("lookahead_yuv_frames") == 20
        assert rt.stat("fallbacks") == 0
        hosts = sum(1 for s in specs if "host" in (s.lin, s.lout))
        assert rt.stat("lookahead_host_frames") == hosts
        for i in ins:                                           # (inputs and their guards untouched)
            i.check([p._rows(p.host) for p in i.planes])
        # the same buffers again: captured at the second use, replayed at the third, same bytes
        for _ in range(2):
            rt.reset()
            run_calls(rt, ins, outs, want, (8, 7, 5))
        assert tensors_equal(rt, tensors) and rt.stat("graph_replays") >= 2


def test_a_pass_that_is_run_again_gives_the_same_planes():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    specs = [Spec(V210, "host", "bottom-up", Y410, "host", "padded") for _ in range(3)] + \
            [Spec(X2RGB10, "device", "padded", V210, "device", "plain") for _ in range(3)] + \
            [Spec(I410, "device", "plain", Y210, "host", "plain"), Spec(Y210, "host", "plain", X2BGR10, "device", "bottom-up")]
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


# ---- 6. the source and the output stage ---------------------------------------------------------------------------------
SRC_H, SRC_W = 60, 94                                           # (V210: 15 whole groups and one of four pixels)


def test_a_scaled_v210_source_is_decoded_at_source_size_then_scaled():
    torch, dev = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    clip = M.synthetic_frames(2, SRC_H, SRC_W, seed=5, kind="smooth")
    rng = np.random.default_rng(4)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(SRC_W, SRC_H)
        for location in ("host", "device"):
            for t, f in enumerate(clip):
                planes = P.junk(V210, source(f, V210, CS), SRC_W, rng)
                want = b.process_image(SRC.scale(decoded(V210, CS, planes, SRC_W), h, w))
                got = np.zeros((4 * h, 4 * w, 4), np.uint8)
                if location == "host":
                    f_in = host(V210, planes, SRC_W)
                else:
                    held = [torch.from_numpy(p.view(np.int32).copy()).to(dev) for p in planes]
                    torch.cuda.synchronize()
                    f_in = R.device_frame(V210, SRC_W, SRC_H, held)
                a.process_frame(f_in, R.host_frame(R.FMT_BGRX, [got]))
                assert np.array_equal(got, want), (location, t)
                assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))
        assert a.stat("source_stage_frames") == 4


@pytest.mark.parametrize("fmt", [Y410, X2RGB10, V210], ids=name_of)
def test_an_output_at_an_output_size_is_encoded_from_the_scaled_16_bit_samples(fmt):
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    oh, ow = 90, 146                                            # (V210: 24 whole groups and one of two pixels)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_output_size(ow, oh)
        for t, f in enumerate(M.synthetic_frames(2, h, w, seed=6, kind="smooth")):
            got = blank(fmt, oh, ow)
            a.process_frame(R.host_frame(R.FMT_BGRX, [f]), host(fmt, got, ow))
            frame = b.process_image(f)
            scaled = O.scale16(T.p_from_state(state_of(b, h, w)), oh, ow)
            assert same(got, P.encode_planes(fmt, CS, frame16=scaled)), t
            assert not same(got, P.encode_planes(fmt, CS, frame=O.scale8(frame, oh, ow))), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


def test_a_masked_v210_output_comes_from_the_blended_8_bit_frame():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
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
            planes = source(f, Y210, CS)
            src = decoded(Y210, CS, planes, SRC_W)
            plain = b.process_image(SRC.scale(src, h, w))
            want = SRC.blend(plain, src, mask)
            assert (want != plain).any()
            got = blank(V210, 4 * h, 4 * w)
            a.process_frame(host(Y210, planes, SRC_W), host(V210, got, 4 * w))
            assert same(got, expect(V210, CS, want, None)), t
        assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))
        # without the mask the output comes from the f16 state again
        a.set_source_mask(None)
        planes = source(clip[0], Y210, CS)
        b.process_image(SRC.scale(decoded(Y210, CS, planes, SRC_W), h, w))
        got = blank(V210, 4 * h, 4 * w)
        a.process_frame(host(Y210, planes, SRC_W), host(V210, got, 4 * w))
        assert same(got, expect(V210, CS, None, state_of(b, h, w)))


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_runtime_unchanged():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(4, h, w, seed=2, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        held = {f: source(frames[0], f, CS) for f in NEW}
        fin = {f: host(f, p, w) for f, p in held.items()}
        pouts = {f: blank(f, 4 * h, 4 * w) for f in NEW}
        fout = {f: host(f, p, 4 * w) for f, p in pouts.items()}
        good_in, good_out = fin[V210], fout[Y410]
        row = {f: P.row_bytes(f, w) for f in NEW}
        orow = {f: P.row_bytes(f, 4 * w) for f in NEW}
        # a V210 row of 50 pixels holds as many bytes as one of 54 (nine groups): only the width tells
        assert P.row_bytes(V210, 50) == P.row_bytes(V210, 54) == 144

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
            "odd V210 width": (bad(fin[V210], width=w - 1), good_out, "even width"),
            "odd Y210 width": (bad(fin[Y210], width=w - 1), good_out, "even width"),
            "odd V210 output width": (good_in, bad(fout[V210], width=4 * w - 1), "even width"),
            "odd Y210 output width": (good_in, bad(fout[Y210], width=4 * w + 1), "even width"),
            "wrong size": (good_in, bad(good_out, height=4 * h - 1), "exactly"),
            "wrong V210 width": (bad(good_in, width=w - 2), good_out, "exactly"),
            "graphics resource": (bad(good_in, location=R.LOC_GRAPHICS_RESOURCE), good_out, "graphics"),
            "graphics resource output": (good_in, bad(fout[X2RGB10], location=R.LOC_GRAPHICS_RESOURCE), "graphics"),
        }
        for f in NEW:
            n = name_of(f)
            align = 2 if f == Y210 else 4
            cases[f"{n}: short stride"] = (bad(fin[f], stride=(0, row[f] - align)), good_out, "stride")
            cases[f"{n}: short negative stride"] = (bad(fin[f], stride=(0, -(row[f] - align))), good_out, "stride")
            cases[f"{n}: short output stride"] = (good_in, bad(fout[f], stride=(0, orow[f] - align)), "stride")
            cases[f"{n}: plane off alignment"] = (bad(fin[f], plane=(0, fin[f].planes[0] + align // 2)), good_out,
                                                  f"multiples of {align}")
            cases[f"{n}: stride off alignment"] = (bad(fin[f], stride=(0, row[f] + align // 2)), good_out, f"multiples of {align}")
            cases[f"{n}: output plane off alignment"] = (good_in, bad(fout[f], plane=(0, fout[f].planes[0] + align // 2)),
                                                         f"multiples of {align}")
            cases[f"{n}: NULL plane"] = (bad(fin[f], plane=(0, None)), good_out, "NULL")
            cases[f"{n}: NULL output plane"] = (good_in, bad(fout[f], plane=(0, None)), "NULL")
        # (Y210's rows are 4 W bytes: a P210 luma stride of 2 W is short; a 4 W stride is short of nothing for V210's 8 W / 3)
        cases["a 16-bit luma stride for a Y210 row"] = (bad(fin[Y210], stride=(0, 2 * w)), good_out, "stride")
        for value in (5, 7, 21, 42, 22, 23, 26, 27, 43, 46, 47, 51):
            cases[f"unknown input format {value}"] = (bad(good_in, format=value), good_out, "unknown format")
            cases[f"unknown output format {value}"] = (good_in, bad(good_out, format=value), "unknown format")
        before = {k: a.stat(k) for k in ("lookahead_frames", "source_stage_frames", "graph_replays")}
        for name, (fi, fo, words) in cases.items():
            with pytest.raises(R.JoshUpscaleError) as e:
                a.process_frame(fi, fo)
            assert e.value.code == 1 and words in e.value.message, (name, e.value.message)
            assert "JU_" not in e.value.message
        # a bad frame in the middle of a ju_process_frames call is named by its index
        held_all = [source(f, V210, CS) for f in frames]        # (kept alive: the frames hold raw pointers)
        ins = [host(V210, p, w) for p in held_all]
        keep = [blank(Y410, 4 * h, 4 * w) for _ in frames]
        outs = [host(Y410, p, 4 * w) for p in keep]
        with pytest.raises(R.JoshUpscaleError) as e:
            a.process_frames([ins[0], ins[1], bad(ins[2], stride=(0, row[V210] - 4)), ins[3]], outs)
        assert e.value.code == 1 and "frame 2" in e.value.message
        assert all((as_bytes(p) == 0).all() for planes in keep for p in planes)
        assert all((as_bytes(p) == 0).all() for planes in pouts.values() for p in planes)
        assert before == {k: a.stat(k) for k in before}
        # ju_process_group takes BGRX images only: a V210 buffer described as an image is refused as before
        out = np.zeros((4 * h, 4 * w, 4), np.uint8)
        img = R.JuImage(held[V210][0].ctypes.data, R.LOC_CPU, row[V210], w, h)
        with pytest.raises(R.JoshUpscaleError) as e:
            R.process_group([a], [img], [R.host_image(out)])
        assert e.value.code == 1 and "stride" in e.value.message and (out == 0).all()
        # nothing ran: the stream goes on as its twin's.  Planes beyond the one are not read; nor an RGB frame's colour space
        for t, f in enumerate(frames):
            fi, fo = NEW[t % 5], NEW[(t + 2) % 5]
            pin = source(f, fi, CS)
            got = blank(fo, 4 * h, 4 * w)
            a.process_frame(bad(host(fi, pin, w), plane=(1, 12345), stride=(2, 7), colorspace=-7 if fi in P.RGB else CS),
                            bad(host(fo, got, 4 * w), plane=(2, 99), colorspace=1000 if fo in P.RGB else CS))
            frame = b.process_image(decoded(fi, CS, pin, w))
            assert same(got, expect(fo, CS, frame, state_of(b, h, w))), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))
        del held, held_all
