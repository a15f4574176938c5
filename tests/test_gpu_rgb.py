"""RGB frame formats on the GPU (BGR24, RGB24, RGBX, BGRX64, RGBP8 / 10 / 16 / H / S, BGR96F; csrc/colour_kernels.hip,
engine_frames.cpp): the conversion kernels alone against the numpy definition (tests/rgb_reference.py), bit for bit; inputs
against a twin fed the decoded frame; outputs against the definition applied to the twin's frame or to the runtime's own
f16 state; look-ahead passes against a twin driven frame by frame; the source stage; the refused calls."""

import ctypes as C
import dataclasses

import numpy as np
import pytest

import rgb_reference as G
import source_reference as SRC
import test_gpu_yuv_sampled as YS
import yuv10_reference as T
import yuv_reference as Y
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_yuv import DevPlane, torch_dev
from test_gpu_yuv10 import HOST_LAYOUTS, as_bytes, blob_of, random_state, state_of, tensors_equal
from test_gpu_yuv_lookahead import HostPlane

pytestmark = pytest.mark.gpu

BGRX, I420, NV12, P010, I010 = 0, 1, 2, 3, 4
YUY2, P210, I444, I410 = 16, 19, 24, 25
NEW = G.NEW_FORMATS
(BGR24, RGB24, RGBX, BGRX64, RGBP8, RGBP10, RGBP16, RGBPH, RGBPS, BGR96F) = NEW
name_of = lambda f: G.FORMAT_NAMES.get(f) or YS.NAMES[f]  # noqa: E731
CS = Y.CS_BT709_LIMITED


def sample_bytes(fmt):
    return np.dtype(G.DTYPE[fmt]).itemsize


def blank(fmt, h, w):
    return G.blank_planes(fmt, h, w) if fmt in NEW else YS.blank(fmt, h, w)


def decoded(fmt, cs, planes):
    """The BGRX frame the network consumes for the caller's planes."""
    return G.decode_planes(fmt, planes) if fmt in NEW else YS.decoded(fmt, cs, planes)


def expect(fmt, cs, frame, state):
    """What a runtime writes for an output of the format: from its 8-bit frame, or -- a deep format with a state given --
    from the state."""
    if fmt in NEW:
        return G.encode_planes(fmt, frame=frame, state=state if fmt in G.DEEP else None)
    return YS.expect(fmt, cs, frame, state)


def source(frame, fmt, cs):
    """The planes of one input frame of a BGRX clip in the given format."""
    return G.encode_planes(fmt, frame=frame) if fmt in NEW else YS.source(frame, fmt, cs)


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(as_bytes(g), as_bytes(e)) for g, e in zip(got, want))


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------
SIZES = [(h, w) for w in (1, 3, 15, 16, 17, 23, 33, 100) for h in (1, 2, 3)] + [(2, 1920)]
LAYOUT_NAMES = ("dense", "padded", "bottom-up", "offset", "offset-bottom-up")


def layout(name, b):
    """Plane layouts for samples of b bytes: dense rows (rows of the 3-byte formats then start at every alignment),
    padded, bottom-up, and offset by one sample -- 1, 2 or 4 bytes -- with a pitch that keeps moving the alignment."""
    return {"dense": dict(pad=0, offset=0, flip=False), "padded": dict(pad=32, offset=0, flip=False),
            "bottom-up": dict(pad=16, offset=0, flip=True), "offset": dict(pad=3 * b, offset=b, flip=False),
            "offset-bottom-up": dict(pad=b, offset=b, flip=True)}[name]


KERNEL_CASES = [(f, lay) for f in NEW for lay in LAYOUT_NAMES]


def run_debug(op, fmt, w, h, image_ptr, image_stride, planes):
    lib = R.load_library(True)
    ptrs = (C.c_void_p * 3)(*([p.ptr for p in planes] + [None] * (3 - len(planes))))
    strides = (C.c_ssize_t * 3)(*([p.stride for p in planes] + [0] * (3 - len(planes))))
    rc = lib.ju_debug_rgb(op, fmt, w, h, image_ptr, image_stride, ptrs, strides)
    assert rc == 0, lib.ju_last_error()


def special_floats(top):
    """Float inputs a decode has to get exactly right: k / 255 x top, its two f32 neighbours, values outside the range,
    NaN, +-inf, zeros of both signs, the half-way points."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255) * np.float32(top)).astype(np.float32)
    mid = ((np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255) * np.float32(top)).astype(np.float32)
    t = np.float32(top)
    odd = np.array([-1.0, -0.0, 0.0, t, t * 1.5, 1e30, -1e30, np.inf, -np.inf, np.nan, -np.nan, 1e-40, -1e-40, 65504.0,
                    t * 0.5], np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(1e9)), np.nextafter(k, np.float32(-1e9)), mid,
                           np.nextafter(mid, np.float32(1e9)), np.nextafter(mid, np.float32(-1e9)), odd])


def input_planes(kind, fmt, h, w, rng):
    """Planes of the format with content of the kind: random (junk in the bits and lanes the format ignores), zero, full,
    or -- the float formats -- special."""
    dt = G.DTYPE[fmt]
    shapes = [p.shape for p in G.blank_planes(fmt, h, w)]
    if fmt in G.FLOAT:
        top = 255.0 if fmt == BGR96F else 1.0
        if kind == "zero":
            return [np.zeros(s, dt) for s in shapes]
        if kind == "full":
            return [np.full(s, top, dt) for s in shapes]
        if kind == "special":
            pool = special_floats(top)
            with np.errstate(over="ignore"):
                return [pool[(rng.integers(0, pool.size) + np.arange(int(np.prod(s)))) % pool.size].reshape(s).astype(dt)
                        for s in shapes]
        return [rng.uniform(-0.1 * top, 1.1 * top, s).astype(dt) for s in shapes]
    top = 1 << (8 * np.dtype(dt).itemsize)
    if kind == "zero":
        return [np.zeros(s, dt) for s in shapes]
    if kind == "full":
        return [np.full(s, 1023 if fmt == RGBP10 else top - 1, dt) for s in shapes]
    return [rng.integers(0, top, s, dtype=dt) for s in shapes]  # (RGBP10: junk in the upper 6 bits; X lanes: junk)


def check_decode(fmt, lay, h, w, held):
    src = [DevPlane(as_bytes(p), **lay) for p in held]
    out = DevPlane(np.full((h, w, 4), 0x77, np.uint8), pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
    run_debug(0, fmt, w, h, out.ptr, out.stride, src)
    out.check(G.decode_planes(fmt, held))
    for p, d in zip(src, held):
        p.check(as_bytes(d))                                    # (inputs and their guards untouched)


def check_encode(fmt, lay, h, w, bgrx):
    inb = DevPlane(bgrx, pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
    want = G.encode_planes(fmt, frame=bgrx)
    dst = [DevPlane(np.full_like(as_bytes(p), 0x77), **lay) for p in want]
    run_debug(1, fmt, w, h, inb.ptr, inb.stride, dst)
    for p, e in zip(dst, want):
        p.check(as_bytes(e))
    inb.check(bgrx)


def check_state_encode(fmt, lay, h, w, state):
    torch, dev = torch_dev()
    d_state = torch.from_numpy(state).to(dev)
    assert d_state.data_ptr() % 16 == 0
    want = G.encode_planes(fmt, state=state)
    dst = [DevPlane(np.full_like(as_bytes(p), 0x77), **lay) for p in want]
    run_debug(2, fmt, w, h, d_state.data_ptr(), 0, dst)
    for p, e in zip(dst, want):
        p.check(as_bytes(e))
    assert np.array_equal(d_state.cpu().numpy().view(np.uint16), state.view(np.uint16))


@pytest.mark.parametrize("fmt,lay_name", KERNEL_CASES, ids=[f"{G.FORMAT_NAMES[f]}-{lay}" for f, lay in KERNEL_CASES])
def test_kernels_equal_the_numpy_definition(fmt, lay_name):
    rng = np.random.default_rng(100 + fmt)
    lay = layout(lay_name, sample_bytes(fmt))
    for n, (h, w) in enumerate(SIZES):
        kinds = ["random", ("zero", "full")[n % 2]] + (["special"] if fmt in G.FLOAT else [])
        for kind in kinds:
            check_decode(fmt, lay, h, w, input_planes(kind, fmt, h, w, rng))
        bgrx = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)  # (X random: ignored)
        if n % 8 == 1:
            bgrx[..., :3] = 0
        if n % 8 == 5:
            bgrx[..., :3] = 255
        check_encode(fmt, lay, h, w, bgrx)
        if fmt in G.DEEP:
            check_state_encode(fmt, lay, h, w, random_state(h, w, rng))


@pytest.mark.parametrize("fmt", [BGRX64, RGBP16, RGBP10], ids=name_of)
def test_every_16_bit_word_decodes_as_defined(fmt):
    """A 256 x 256 frame holding every word once in each channel (three different orders); RGBP10: every 10-bit value with
    every setting of the six ignored bits."""
    words = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    b, g, r = words, words[::-1, ::-1].copy(), words.T.copy()
    held = G.assemble(fmt, b, g, r)
    if fmt == BGRX64:
        held[0][..., 3] = words[::-1]                           # (X: ignored)
    check_decode(fmt, layout("dense", 2), 256, 256, held)


@pytest.mark.parametrize("fmt", G.DEEP, ids=name_of)
def test_every_in_range_state_value_encodes_as_defined(fmt):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    s = bits.view(np.float16)
    with np.errstate(invalid="ignore"):
        s = s[np.isfinite(s) & (np.abs(s.astype(np.float32)) <= 0.5)]
    h, w = 60, 481                                              # (28 860 pixels for 28 674 values; the rest repeats)
    idx = np.arange(h * w) % s.size
    state = np.zeros((h, w, 4), np.float16)
    state[..., 0] = s[idx].reshape(h, w)
    state[..., 1] = s[idx[::-1]].reshape(h, w)
    state[..., 2] = s[(idx * 7) % s.size].reshape(h, w)
    state[..., 3] = np.float16(0.123)                           # (the unused lane: not read into the output)
    check_state_encode(fmt, layout("dense", sample_bytes(fmt)), h, w, state)


# ---- 2. the items kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [(BGR24, I420, RGBPS, I444, BGRX64, P010, RGBP10, BGR96F),
                                 (RGB24, RGBX, NV12, RGBP8, I410, RGBP16, RGBPH, YUY2)], ids=["a", "b"])
def test_items_kernel_decodes_new_and_old_formats_in_one_launch(mix):
    lib = R.load_library(True)
    rng = np.random.default_rng(31)
    for (h, w) in [(46, 30), (18, 100)]:
        fmts, css, outs, srcs, want, held_all = [], [], [], [], [], []
        for i, fmt in enumerate(mix):
            if fmt in NEW:
                b = sample_bytes(fmt)
                lay = layout(LAYOUT_NAMES[i % len(LAYOUT_NAMES)], b)
                held = input_planes("special" if fmt in G.FLOAT and i % 2 else "random", fmt, h, w, rng)
                cs = 7 + i                                      # (ignored for an RGB item)
            else:
                b = 2 if fmt in YS.S.DEEP or fmt in (P010, I010) else 1
                lay = layout(LAYOUT_NAMES[i % len(LAYOUT_NAMES)], b)
                held = YS.source(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), fmt, i % 4)
                cs = i % 4
            fmts.append(fmt)
            css.append(cs)
            held_all.append(held)
            want.append(decoded(fmt, cs, held))
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
def input_clip_planes(frame, fmt, t, rng):
    """The planes of an input frame; on odd frames with junk where the format ignores it, and -- the float formats -- moved
    to a neighbouring float that decodes alike."""
    held = G.encode_planes(fmt, frame=frame)
    if t % 2 == 0:
        return held
    if fmt == RGBP10:
        held = [p | (rng.integers(0, 64, p.shape, dtype=np.uint16) << 10).astype(np.uint16) for p in held]
    elif fmt in (RGBX, BGRX64):
        held[0][..., 3] = rng.integers(0, 256, held[0].shape[:2])
    elif fmt in (RGBPS, BGR96F):
        held = [np.nextafter(p, np.float32(-1)) for p in held]
    return held


@pytest.mark.parametrize("dtype", [pytest.param(R.DTYPE_F16, id="fp16"), pytest.param(R.DTYPE_BF16, id="bf16")])
@pytest.mark.parametrize("fmt", NEW, ids=name_of)
def test_input_equals_process_of_the_decoded_frame(fmt, dtype):
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    rng = np.random.default_rng(3)
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=3, kind="smooth")):
            held = input_clip_planes(f, fmt, t, rng)
            frame = G.decode_planes(fmt, held)
            assert np.array_equal(frame[..., :3], f[..., :3])
            got = np.zeros((4 * h, 4 * w, 4), np.uint8)
            a.process_frame(R.host_frame(fmt, held, colorspace=99), R.host_frame(R.FMT_BGRX, [got]))   # (colorspace: ignored)
            want = b.process_image(frame)
            assert np.array_equal(got, want), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


DTYPES = [pytest.param(R.DTYPE_F16, id="fp16"), pytest.param(R.DTYPE_BF16, id="bf16")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", NEW, ids=name_of)
def test_output_equals_the_definition(fmt, dtype):
    """8-bit formats: the twin's BGRX output, permuted; deep formats: the definition applied to the runtime's own f16 state."""
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        assert a.stat("hbd_from_state") == 1
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=8, kind="smooth")):
            got = blank(fmt, 4 * h, 4 * w)
            a.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(fmt, got))
            frame = b.process_image(f)
            want = expect(fmt, CS, frame, state_of(a, h, w))
            assert same(got, want), t
            if fmt in G.DEEP:                                   # (and that is not what the 8-bit frame would give)
                assert not same(got, expect(fmt, CS, frame, None)), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["brightness", "output-flow"])
@pytest.mark.parametrize("fmt", G.DEEP, ids=name_of)
def test_models_whose_state_is_not_the_frame_encode_from_the_8_bit_frame(fmt, variant, dtype):
    if variant == "brightness":
        cfg = small_config(normalize_brightness=True)
        blob = blob_of(cfg)
    else:
        cfg = small_config()
        blob = M.serialize(*M.output_flow(cfg, M.make_seeded_weights(cfg)))
    h, w = cfg.frame_height, cfg.frame_width
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        assert a.stat("hbd_from_state") == 0
        for t, f in enumerate(M.synthetic_frames(3, h, w, seed=11, kind="smooth")):
            got = blank(fmt, 4 * h, 4 * w)
            a.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(fmt, got))
            frame = b.process_image(f)
            assert same(got, expect(fmt, CS, frame, None)), t
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state")), t


def test_process_rgb():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    f = M.synthetic_frames(1, h, w, seed=5, kind="smooth")[0]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        frame = b.process_image(f)
        got = a.process_rgb(np.ascontiguousarray(f[..., :3]), R.FMT_BGR24)
        assert got.shape == (4 * h, 4 * w, 3) and np.array_equal(got, frame[..., :3])
        a.reset()
        r, g, bl = a.process_rgb(G.encode_planes(RGBPS, frame=f), R.FMT_RGBPS, out_format=R.FMT_RGBP8)
        assert np.array_equal(np.stack([bl, g, r], -1), frame[..., :3])
        a.reset()
        assert np.array_equal(a.process_rgb(G.encode_planes(RGBP16, frame=f), R.FMT_RGBP16, out_format=R.FMT_BGRX), frame)


# ---- 4. a relation that a wrong source cannot meet ---------------------------------------------------------------------
def test_deep_outputs_of_a_plain_model_carry_the_frame():
    """A plain f16 model's RGBP16 / RGBPS / BGR96F planes, decoded on the CPU to D, against the twin's 8-bit frame u8:
    D - u8 is 0 or 1 everywhere.

    With t = r + 0.5 of the tail's f32 output r, the frame is u8 = floor(255 t) and the state holds r rounded to f16;
    t' = s + 0.5 and P = floor(65536 t').  tests/test_gpu_yuv10.py (test_10_bit_luma_lies_around_4_times_the_8_bit_luma)
    derives P / 257 - u8 in [-0.035, 1.035].  RGBP16 decodes to (P + 128) // 257 = round(P / 257): 0 or 1 above u8.
    255 t' lies in [255 P / 65536, 255 (P + 1) / 65536), within 255 / 65536 + P / (257 x 65536) < 0.008 of P / 257, so
    255 t' - u8 is in [-0.043, 1.043]; RGBPS holds t' exactly and its decode floor(t' x 255 + 0.5) carries two f32
    roundings of at most 255 x 2^-24 + 2^-17 < 3e-5 together, BGR96F holds the same product: round(255 t') is u8 or
    u8 + 1 with a margin of 0.45.  The frame truncates, the decodes round: equality with the frame is NOT claimed, nor
    that trunc(BGR96F) is the frame."""
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    for fmt in (RGBP16, RGBPS, BGR96F):
        with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
            seen = set()
            for f in M.synthetic_frames(3, h, w, seed=14, kind="smooth"):
                got = blank(fmt, 4 * h, 4 * w)
                a.process_frame(R.host_frame(R.FMT_BGRX, [f]), R.host_frame(fmt, got))
                u8 = b.process_image(f)[..., :3].astype(np.int64)
                diff = G.decode_planes(fmt, got)[..., :3].astype(np.int64) - u8
                print(G.FORMAT_NAMES[fmt], "D - u8 in", int(diff.min()), int(diff.max()), "pixels above:", int((diff == 1).sum()))
                assert diff.min() >= 0 and diff.max() <= 1
                seen |= set(np.unique(diff).tolist())
            assert seen == {0, 1}                               # (an encode from the 8-bit frame would give 0 alone)


# ---- 5. look-ahead passes -----------------------------------------------------------------------------------------------
class Side:
    """One side of a frame call: its planes in host or device memory with guard bytes around them."""

    def __init__(self, fmt, cs, loc, layout_name, planes, w, h):
        lay = dict(HOST_LAYOUTS[layout_name], offset=0)
        if fmt == BGRX:
            lay["pad"] *= 4
        cls = HostPlane if loc == "host" else DevPlane
        self.fmt = fmt
        self.planes = [cls(p if fmt == BGRX else as_bytes(p), **lay) for p in planes]
        self.frame = R._frame(fmt, cs, R.LOC_CPU if loc == "host" else R.LOC_DEVICE, w, h,
                              [p.ptr for p in self.planes], [p.stride for p in self.planes])

    def check(self, want):
        for p, e in zip(self.planes, want):
            p.check(e if self.fmt == BGRX else as_bytes(e))


@dataclasses.dataclass
class Spec:
    fin: int
    lin: str
    layin: str
    fout: int
    lout: str
    layout: str
    cin: int = CS
    cout: int = CS


LAYS = ("plain", "padded", "bottom-up")
OTHERS = (BGRX, NV12, I410, P010, YUY2, I420)


def pass_specs():
    """Two frames per new format f: f as an input (host, then device for the next format, ...) beside an old or another
    new format, and f as an output."""
    specs = []
    for i, f in enumerate(NEW):
        loc = ("host", "device")
        specs.append(Spec(f, loc[i % 2], LAYS[i % 3], OTHERS[i % 6] if i % 3 else NEW[(i + 3) % 10], loc[(i // 2) % 2], LAYS[(i + 1) % 3]))
        specs.append(Spec(OTHERS[(i + 2) % 6] if i % 2 else NEW[(i + 5) % 10], loc[(i + 1) % 2], LAYS[(i + 2) % 3], f, loc[(i + i // 2) % 2], LAYS[i % 3]))
    return specs


PASS_SPECS = pass_specs()


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


def test_the_pass_table_holds_every_new_format_on_each_side_in_both_memories():
    for f in NEW:
        assert {s.lin for s in PASS_SPECS if s.fin == f}, name_of(f)
        assert {s.lout for s in PASS_SPECS if s.fout == f}, name_of(f)
    assert {s.lin for s in PASS_SPECS if s.fin in NEW} == {"host", "device"}
    assert {s.lout for s in PASS_SPECS if s.fout in NEW} == {"host", "device"}
    assert {s.fout for s in PASS_SPECS if s.fin in NEW} & set(OTHERS) and {s.fin for s in PASS_SPECS if s.fout in NEW} & set(OTHERS)


def test_passes_mixing_new_and_old_formats_give_the_frame_by_frame_bytes():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    specs = PASS_SPECS
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
    specs = [Spec(BGR24, "host", "bottom-up", RGBPS, "host", "padded") for _ in range(3)] + \
            [Spec(RGBPH, "device", "padded", BGRX64, "device", "plain") for _ in range(3)] + \
            [Spec(I410, "device", "plain", BGR96F, "host", "plain") for _ in range(2)]
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


# ---- 6. the source stage ------------------------------------------------------------------------------------------------
SRC_H, SRC_W = 60, 95


@pytest.mark.parametrize("fmt", [BGR24, RGBPS], ids=name_of)
def test_a_scaled_source_is_decoded_at_source_size_then_scaled(fmt):
    torch, dev = torch_dev()
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    clip = M.synthetic_frames(3, SRC_H, SRC_W, seed=5, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(SRC_W, SRC_H)
        for location in ("host", "device"):
            for t, f in enumerate(clip):
                planes = source(f, fmt, CS)
                want = b.process_image(SRC.scale(decoded(fmt, CS, planes), h, w))
                got = np.zeros((4 * h, 4 * w, 4), np.uint8)
                if location == "host":
                    f_in = R.host_frame(fmt, planes)
                else:
                    held = [torch.from_numpy(p.copy()).to(dev) for p in planes]
                    torch.cuda.synchronize()
                    f_in = R.device_frame(fmt, SRC_W, SRC_H, held)
                a.process_frame(f_in, R.host_frame(R.FMT_BGRX, [got]))
                assert np.array_equal(got, want), (location, t)
                assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))
        assert a.stat("source_stage_frames") == 6


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", [RGBPS, BGRX64], ids=name_of)
def test_a_masked_deep_output_comes_from_the_blended_8_bit_frame(fmt, dtype):
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    rng = np.random.default_rng(2)
    mask = rng.integers(0, 256, (37, 50, 4), dtype=np.uint8)
    kind = rng.integers(0, 3, (37, 50))
    mask[kind == 0, :3] = 255
    mask[kind == 1, :3] = 0
    clip = M.synthetic_frames(2, SRC_H, SRC_W, seed=9, kind="smooth")
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        a.set_source_size(SRC_W, SRC_H)
        a.set_source_mask(mask)
        assert a.stat("hbd_from_state") == 1
        for t, f in enumerate(clip):
            planes = source(f, RGB24, CS)
            src = decoded(RGB24, CS, planes)
            plain = b.process_image(SRC.scale(src, h, w))
            want = SRC.blend(plain, src, mask)
            assert (want != plain).any()
            got = blank(fmt, 4 * h, 4 * w)
            a.process_frame(R.host_frame(RGB24, planes), R.host_frame(fmt, got))
            assert same(got, expect(fmt, CS, want, None)), t
        assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))
        # without the mask the deep output comes from the f16 state again
        a.set_source_mask(None)
        planes = source(clip[0], RGB24, CS)
        b.process_image(SRC.scale(decoded(RGB24, CS, planes), h, w))
        got = blank(fmt, 4 * h, 4 * w)
        a.process_frame(R.host_frame(RGB24, planes), R.host_frame(fmt, got))
        assert same(got, expect(fmt, CS, None, state_of(b, h, w)))


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_runtime_unchanged():
    cfg = small_config()
    blob = blob_of(cfg)
    h, w = cfg.frame_height, cfg.frame_width
    frames = M.synthetic_frames(4, h, w, seed=2, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_BF16) as a, R.Runtime(blob, 0, R.DTYPE_BF16) as b:
        held = {f: source(frames[0], f, CS) for f in (BGR24, BGRX64, RGBP16, RGBPH, RGBPS, BGR96F)}
        fin = {f: R.host_frame(f, p) for f, p in held.items()}
        pouts = {f: blank(f, 4 * h, 4 * w) for f in (RGBPS, BGR96F, RGBP10, RGB24, BGRX64)}
        fout = {f: R.host_frame(f, p) for f, p in pouts.items()}
        good_in, good_out = fin[BGR24], fout[RGBPS]

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
            "odd address, 16-bit words": (bad(fin[BGRX64], plane=(0, fin[BGRX64].planes[0] + 1)), good_out, "multiples of 2"),
            "odd address, planar words": (bad(fin[RGBP16], plane=(1, fin[RGBP16].planes[1] + 1)), good_out, "multiples of 2"),
            "odd address, f16": (bad(fin[RGBPH], plane=(2, fin[RGBPH].planes[2] + 1)), good_out, "multiples of 2"),
            "odd stride, f16": (bad(fin[RGBPH], stride=(0, 2 * w + 1)), good_out, "multiples of 2"),
            "odd output stride, 10-bit": (good_in, bad(fout[RGBP10], stride=(1, 8 * w + 1)), "multiples of 2"),
            "address at 2, f32": (bad(fin[RGBPS], plane=(0, fin[RGBPS].planes[0] + 2)), good_out, "multiples of 4"),
            "stride at 2, f32": (bad(fin[BGR96F], stride=(0, 12 * w + 2)), good_out, "multiples of 4"),
            "output address at 2, f32": (good_in, bad(good_out, plane=(2, good_out.planes[2] + 2)), "multiples of 4"),
            "output stride at 2, packed f32": (good_in, bad(fout[BGR96F], stride=(0, 48 * w + 2)), "multiples of 4"),
            "short 24-bit stride": (bad(good_in, stride=(0, 3 * w - 1)), good_out, "stride"),
            "a BGRX stride for a BGRX64 row": (bad(fin[BGRX64], stride=(0, 4 * w)), good_out, "stride"),
            "short negative stride": (bad(good_in, stride=(0, -(3 * w - 3))), good_out, "stride"),
            "short f32 plane stride": (good_in, bad(good_out, stride=(1, 8 * w)), "stride"),
            "short packed f32 stride": (good_in, bad(fout[BGR96F], stride=(0, 16 * w)), "stride"),
            "NULL packed plane": (bad(good_in, plane=(0, None)), good_out, "NULL"),
            "NULL second plane": (bad(fin[RGBP16], plane=(1, None)), good_out, "NULL"),
            "NULL third output plane": (good_in, bad(good_out, plane=(2, None)), "NULL"),
            "graphics resource": (bad(good_in, location=R.LOC_GRAPHICS_RESOURCE), good_out, "graphics"),
            "graphics resource output": (good_in, bad(fout[RGB24], location=R.LOC_GRAPHICS_RESOURCE), "graphics"),
            "wrong size": (good_in, bad(good_out, height=4 * h - 1), "exactly"),
            "wrong input width": (bad(good_in, width=w - 1), good_out, "exactly"),
        }
        for value in list(range(5, 16)) + [21, 22, 23, 26, 27, 31, 42, 43]:
            cases[f"unknown input format {value}"] = (bad(good_in, format=value), good_out, "format")
            cases[f"unknown output format {value}"] = (good_in, bad(good_out, format=value), "format")
        for name, (fi, fo, words) in cases.items():
            with pytest.raises(R.JoshUpscaleError) as e:
                a.process_frame(fi, fo)
            assert e.value.code == 1 and words in e.value.message, (name, e.value.message)
            assert "JU_" not in e.value.message
        # a bad frame in the middle of a ju_process_frames call is named by its index
        held_all = [source(f, BGR96F, CS) for f in frames]      # (kept alive: the frames hold raw pointers)
        ins = [R.host_frame(BGR96F, p) for p in held_all]
        keep = [blank(RGBPH, 4 * h, 4 * w) for _ in frames]
        outs = [R.host_frame(RGBPH, p) for p in keep]
        with pytest.raises(R.JoshUpscaleError) as e:
            a.process_frames([ins[0], ins[1], bad(ins[2], stride=(0, 12 * w - 4)), ins[3]], outs)
        assert e.value.code == 1 and "frame 2" in e.value.message
        assert all((as_bytes(p) == 0).all() for planes in keep for p in planes)
        assert all((as_bytes(p) == 0).all() for planes in pouts.values() for p in planes)
        # ju_process_group takes BGRX images only: a 24-bit buffer described as an image is refused as before
        out = np.zeros((4 * h, 4 * w, 4), np.uint8)
        img = R.JuImage(held[BGR24][0].ctypes.data, R.LOC_CPU, 3 * w, w, h)
        with pytest.raises(R.JoshUpscaleError) as e:
            R.process_group([a], [img], [R.host_image(out)])
        assert e.value.code == 1 and "stride" in e.value.message and (out == 0).all()
        # nothing ran: the stream goes on as its twin's.  Planes beyond a format's count are not read, nor is the colour space
        for t, f in enumerate(frames):
            pin = source(f, RGB24, CS)
            got = blank(RGBPS, 4 * h, 4 * w)
            a.process_frame(bad(R.host_frame(RGB24, pin), plane=(1, 12345), stride=(2, 7), colorspace=-5 - t),
                            bad(R.host_frame(RGBPS, got), colorspace=1000))
            frame = b.process_image(decoded(RGB24, CS, pin))
            assert same(got, expect(RGBPS, CS, frame, state_of(b, h, w)))
            assert np.array_equal(a.read_tensor("state"), b.read_tensor("state"))
        del held, held_all
