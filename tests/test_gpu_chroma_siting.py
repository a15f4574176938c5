"""Chroma siting (left, centre, top-left) and BT.2020 on the GPU (csrc/colour_kernels.hip), byte for byte against the
definition (tests/chroma_siting_reference.py): every 4:2:0 and 4:2:2 kernel alone at the sizes where each index rule can
go wrong; the two items kernels; single frames, a look-ahead pass, a group pass and a tiled frame against twins fed the
definition's decode and encoded by the definition; the refused values."""

import ctypes as C
import itertools

import numpy as np
import pytest

import chroma_siting_reference as CS
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_packed10 import LAYOUTS32
from test_gpu_yuv import LAYOUTS as LAYOUTS8
from test_gpu_yuv import DevPlane, torch_dev
from test_gpu_yuv10 import LAYOUTS as LAYOUTS16
from test_gpu_yuv10 import as_bytes, blob_of, random_state, state_of

pytestmark = pytest.mark.gpu

I420, NV12, P010, I010 = 1, 2, 3, 4
YUY2, UYVY, I422, P210, I210, I444, I410 = 16, 17, 18, 19, 20, 24, 25
V210, Y210, Y410 = 48, 49, 50
KERNEL_FORMATS = (I420, NV12, P010, I010, YUY2, UYVY, I422, P210, I210, Y210, V210)
LEFT, CENTER, TOPLEFT = R.CHROMA_LEFT, R.CHROMA_CENTER, R.CHROMA_TOPLEFT
# centre and top-left with the first and the last matrix; the default siting with the two new matrices
COMBOS = (CENTER | 0, CENTER | 5, TOPLEFT | 0, TOPLEFT | 5, LEFT | 4, LEFT | 5)
# (h, w).  4:2:0: 2x2 every clamp at once; 18 wide = one full strip and a two-column strip -- at column 16 centre reads the
# neighbouring strip's chroma -- and 4 rows = two chroma rows, where top-left's encode reads row 2j - 1 across threads;
# 34x6 three strips and rows; 30x46 odd chroma counts, one partial strip.  4:2:2: one row per thread.  V210: 12-pixel
# strips of two groups -- a lone pair, one group, a partial second group, five strips with a partial last group.
SIZES = {420: [(2, 2), (4, 18), (6, 34), (46, 30)], 422: [(1, 2), (3, 18), (47, 30)], "v210": [(1, 2), (2, 6), (3, 8), (3, 50)]}
name_of = CS.FORMAT_NAMES.get


def layouts_of(fmt):
    lays = LAYOUTS32 if fmt in (V210, Y410) else (LAYOUTS16 if fmt in CS.DEEP else LAYOUTS8)
    return [lays[k] for k in sorted(lays)]


def hook_of(fmt):
    lib = R.load_library(True)
    if fmt in (V210, Y210, Y410):
        return lib.ju_debug_packed10
    if CS.SAMPLING[fmt] != 420:
        return lib.ju_debug_yuv_sampled
    return lib.ju_debug_yuv10 if fmt in CS.DEEP else lib.ju_debug_yuv


def plane_args(planes):
    return ((C.c_void_p * 3)(*([p.ptr for p in planes] + [None] * (3 - len(planes)))),
            (C.c_ssize_t * 3)(*([p.stride for p in planes] + [0] * (3 - len(planes)))))


def run_hook(op, fmt, cs, w, h, image_ptr, image_stride, planes):
    """op 0: planes -> BGRX; 1: BGRX u8 -> planes; 2: the f16 state -> planes; 3: a u16 frame -> planes."""
    lib = R.load_library(True)
    ptrs, strides = plane_args(planes)
    if op == 3:
        rc = lib.ju_debug_output(1, None, w, h, image_ptr, 0, 0, fmt, cs, ptrs, strides)
    else:
        rc = hook_of(fmt)(op, fmt, cs, w, h, image_ptr, image_stride, ptrs, strides)
    assert rc == 0, lib.ju_last_error()


def content(kind, fmt, h, w, rng):
    """(y, u, v) sample arrays of a frame of the format."""
    top, dt = (1023, np.uint16) if fmt in CS.DEEP else (255, np.uint8)
    c = CS.YS.chroma_shape(CS.SAMPLING[fmt], h, w)
    if kind == "random":
        return [rng.integers(0, top + 1, s).astype(dt) for s in ((h, w), c, c)]
    if kind == "zero":
        return [np.zeros(s, dt) for s in ((h, w), c, c)]
    if kind == "full":
        return [np.full(s, top, dt) for s in ((h, w), c, c)]
    cb = (np.indices(c).sum(0) % 2 * top).astype(dt)            # extreme chroma in a checkerboard of samples
    return [rng.integers(0, top + 1, (h, w)).astype(dt), cb, (top - cb).astype(dt)]


def check_encode(op, fmt, cs, w, h, lay, image_ptr, image_stride, want):
    dst = [DevPlane(np.full_like(as_bytes(p), 0x77), **lay) for p in want]
    run_hook(op, fmt, cs, w, h, image_ptr, image_stride, dst)
    for p, e in zip(dst, want):
        p.check(as_bytes(e))                                    # (and the guard bytes around the rows)


# ---- 1. the kernels alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", KERNEL_FORMATS, ids=name_of)
def test_kernels_equal_the_definition(fmt):
    torch, dev = torch_dev()
    rng = np.random.default_rng(500 + fmt)
    lays = layouts_of(fmt)
    deep = fmt in CS.DEEP
    for (h, w) in SIZES["v210" if fmt == V210 else CS.SAMPLING[fmt]]:
        # every siting | matrix x every layout x every content: the sizes are tiny
        for cs, lay, kind in itertools.product(COMBOS, lays, ("random", "zero", "full", "extreme")):
            img_lay = dict(pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"])
            held = CS.to_words(fmt, *content(kind, fmt, h, w, rng))
            # the decode
            src = [DevPlane(as_bytes(p), **lay) for p in held]
            out = DevPlane(np.full((h, w, 4), 0x77, np.uint8), **img_lay)
            run_hook(0, fmt, cs, w, h, out.ptr, out.stride, src)
            out.check(CS.decode_planes(fmt, cs, held, width=w))
            for p, d in zip(src, held):
                p.check(as_bytes(d))                        # (inputs untouched)
            # the encode from a u8 frame (X random: ignored)
            bgrx = rng.integers(0, 256, (h, w, 4), dtype=np.uint8) if kind == "random" else \
                CS.decode_planes(fmt, cs, held, width=w)
            inb = DevPlane(bgrx, **img_lay)
            check_encode(1, fmt, cs, w, h, lay, inb.ptr, inb.stride, CS.encode_planes(fmt, cs, frame=bgrx))
            if not deep:
                continue
            # ... from the f16 state
            if kind == "random":
                state = random_state(h, w, rng)
            elif kind in ("zero", "full"):
                state = np.full((h, w, 4), -0.5 if kind == "zero" else 0.5, np.float16)
            else:
                state = (bgrx.astype(np.float32) / 255.0 - 0.5).astype(np.float16)
            d_state = torch.from_numpy(state).to(dev)
            check_encode(2, fmt, cs, w, h, lay, d_state.data_ptr(), 0, CS.encode_planes(fmt, cs, state=state))
            # ... from a u16 frame (the fourth lane random: unused)
            if kind == "random":
                frame16 = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
            elif kind in ("zero", "full"):
                frame16 = np.full((h, w, 4), 0 if kind == "zero" else 65535, np.uint16)
            else:
                frame16 = bgrx.astype(np.uint16) * 257
            d_frame = torch.from_numpy(frame16.view(np.int16)).to(dev)
            check_encode(3, fmt, cs, w, h, lay, d_frame.data_ptr(), 0, CS.encode_planes(fmt, cs, frame16=frame16))


def test_a_4_4_4_format_takes_a_siting_and_ignores_it():
    rng = np.random.default_rng(12)
    h, w = 3, 18
    for fmt in (I444, I410, Y410):
        lay = layouts_of(fmt)[0]
        held = CS.to_words(fmt, *content("random", fmt, h, w, rng))
        bgrx = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        for siting in (CENTER, TOPLEFT):
            src = [DevPlane(as_bytes(p), **lay) for p in held]
            out = DevPlane(np.full((h, w, 4), 0x77, np.uint8))
            run_hook(0, fmt, 4 | siting, w, h, out.ptr, out.stride, src)
            out.check(CS.decode_planes(fmt, 4, held))
            inb = DevPlane(bgrx)
            check_encode(1, fmt, 5 | siting, w, h, lay, inb.ptr, inb.stride, CS.encode_planes(fmt, 5, frame=bgrx))


# ---- 2. the items kernels -----------------------------------------------------------------------------------------------
ITEMS = [(NV12, CENTER | 1), (P010, TOPLEFT | 4), (I420, TOPLEFT | 3), (YUY2, CENTER | 5), (V210, CENTER | 2),
         (I010, CENTER | 0), (P210, LEFT | 5), (Y410, TOPLEFT | 4)]


@pytest.mark.parametrize("sized", [False, True], ids=["plain", "sized"])
def test_items_kernels_take_a_siting_and_a_matrix_per_item(sized):
    lib = R.load_library(True)
    rng = np.random.default_rng(77)
    for (h, w) in [(4, 18), (46, 30)]:
        sizes = [((h, w) if not sized or i % 2 == 0 else (h + 2, w + 6)) for i in range(8)]
        outs, srcs, want, single = [], [], [], []
        for i, (fmt, cs) in enumerate(ITEMS):
            ih, iw = sizes[i]
            lays = layouts_of(fmt)
            lay = lays[i % len(lays)]
            held = CS.to_words(fmt, *content("random", fmt, ih, iw, rng))
            want.append(CS.decode_planes(fmt, cs, held, width=iw))
            srcs.append([DevPlane(as_bytes(p), **lay) for p in held])
            outs.append(DevPlane(np.zeros((ih, iw, 4), np.uint8), pad=lay["pad"] * 4, offset=lay["offset"], flip=lay["flip"]))
            alone = DevPlane(np.zeros((ih, iw, 4), np.uint8))
            run_hook(0, fmt, cs, iw, ih, alone.ptr, alone.stride, srcs[-1])
            single.append(alone)
        ptrs, strides = [], []
        for planes in srcs:
            ptrs += [p.ptr for p in planes] + [None] * (3 - len(planes))
            strides += [p.stride for p in planes] + [0] * (3 - len(planes))
        common = ((C.c_void_p * 8)(*[o.ptr for o in outs]), (C.c_ssize_t * 8)(*[o.stride for o in outs]),
                  (C.c_void_p * 24)(*ptrs), (C.c_ssize_t * 24)(*strides))
        fmts, css = (C.c_int * 8)(*[f for f, _ in ITEMS]), (C.c_int * 8)(*[c for _, c in ITEMS])
        if sized:
            rc = lib.ju_debug_yuv_items_sized(8, fmts, css, (C.c_size_t * 8)(*[s[1] for s in sizes]),
                                              (C.c_size_t * 8)(*[s[0] for s in sizes]), *common)
        else:
            rc = lib.ju_debug_yuv_items(8, fmts, css, w, h, *common)
        assert rc == 0, lib.ju_last_error()
        for o, e, alone in zip(outs, want, single):
            o.check(e)
            alone.check(e)                                      # (the single kernel's bytes)


# ---- 3. end to end on the suite's smallest model ------------------------------------------------------------------------
N = 8
IN_CS = [CENTER | 1, TOPLEFT | 4, LEFT | 5, CENTER | 3, TOPLEFT | 0, CENTER | 5, LEFT | 2, TOPLEFT | 1]
OUT_CS = [TOPLEFT | 4, CENTER | 5, TOPLEFT | 2, LEFT | 4, CENTER | 0, TOPLEFT | 5, CENTER | 4, LEFT | 5]
_TWIN = {}


def twin():
    """NV12 frames, their colour spaces, and what the definition gives for them: definition-decode, a twin runtime's
    ju_process, definition-encode to P010 from that twin's state.  Computed once and left unchanged."""
    if not _TWIN:
        cfg = small_config()
        blob = blob_of(cfg)
        h, w = cfg.frame_height, cfg.frame_width
        clip = M.synthetic_frames(N, h, w, seed=31, kind="smooth")
        held = [CS.encode_planes(NV12, IN_CS[t], frame=clip[t]) for t in range(N)]
        want = []
        with R.Runtime(blob, 0, R.DTYPE_F16) as b:
            assert b.stat("hbd_from_state") == 1
            for t in range(N):
                b.process_image(CS.decode_planes(NV12, IN_CS[t], held[t]))
                want.append(CS.encode_planes(P010, OUT_CS[t], state=state_of(b, h, w)))
            tensors = [b.read_tensor(n).copy() for n in ("state", "flow_in")]
        for planes in held + want:
            for p in planes:
                p.setflags(write=False)
        _TWIN.update(blob=blob, h=h, w=w, held=held, want=want, tensors=tensors)
    return _TWIN


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, e) for g, e in zip(got, want))


def blank_p010(h, w):
    return [np.zeros((h, w), np.uint16), np.zeros((h // 2, w), np.uint16)]


def test_single_frames_nv12_centre_in_p010_top_left_bt2020_out():
    t = twin()
    h, w = t["h"], t["w"]
    assert (IN_CS[0], OUT_CS[0]) == (R.CHROMA_CENTER | R.CS_BT601_FULL, R.CHROMA_TOPLEFT | R.CS_BT2020_LIMITED)
    with R.Runtime(t["blob"], 0, R.DTYPE_F16) as a:
        for k in range(N):
            got = blank_p010(4 * h, 4 * w)
            a.process_frame(R.host_frame(NV12, t["held"][k], IN_CS[k]), R.host_frame(P010, got, OUT_CS[k]))
            assert same(got, t["want"][k]), k
        assert all(np.array_equal(a.read_tensor(n), e) for n, e in zip(("state", "flow_in"), t["tensors"]))


def test_one_look_ahead_pass_of_8_with_the_siting_changing_per_frame():
    t = twin()
    h, w = t["h"], t["w"]
    with R.Runtime(t["blob"], 0, R.DTYPE_F16) as a:
        got = [blank_p010(4 * h, 4 * w) for _ in range(N)]
        a.process_frames([R.host_frame(NV12, t["held"][k], IN_CS[k]) for k in range(N)],
                         [R.host_frame(P010, got[k], OUT_CS[k]) for k in range(N)])
        assert a.stat("lookahead_yuv_frames") == N and a.stat("lookahead_frames") == N and a.stat("fallbacks") == 0
        for k in range(N):
            assert same(got[k], t["want"][k]), k
        assert all(np.array_equal(a.read_tensor(n), e) for n, e in zip(("state", "flow_in"), t["tensors"]))


def test_two_members_of_a_group_pass_with_different_sitings():
    t = twin()
    h, w = t["h"], t["w"]
    # member 0 follows the twin's stream; member 1 takes frame 0 under OTHER sitings, against a twin of its own
    cin, cout = TOPLEFT | 5, CENTER | 4
    held1 = CS.encode_planes(I420, cin, frame=M.synthetic_frames(1, h, w, seed=31, kind="smooth")[0])
    with R.Runtime(t["blob"], 0, R.DTYPE_F16) as b:
        b.process_image(CS.decode_planes(I420, cin, held1))
        want1 = CS.encode_planes(I010, cout, state=state_of(b, h, w))
    with R.Runtime(t["blob"], 0, R.DTYPE_F16) as m0, R.Runtime(t["blob"], 0, R.DTYPE_F16) as m1:
        got0 = blank_p010(4 * h, 4 * w)
        got1 = [np.zeros((4 * h, 4 * w), np.uint16), np.zeros((2 * h, 2 * w), np.uint16), np.zeros((2 * h, 2 * w), np.uint16)]
        R.process_group_frames([m0, m1], [R.host_frame(NV12, t["held"][0], IN_CS[0]), R.host_frame(I420, held1, cin)],
                               [R.host_frame(P010, got0, OUT_CS[0]), R.host_frame(I010, got1, cout)])
        assert m0.stat("group_frames") == 1 and m1.stat("group_frames") == 1
        assert same(got0, t["want"][0])
        assert same(got1, want1)


def test_one_tiled_frame():
    """80 x 30, two tiles: NV12 centre-sited in, NV12 top-left BT.2020 out, against the tiled route on the decoded frame."""
    cfg = small_config()
    blob = blob_of(cfg)
    cin, cout = CENTER | 1, TOPLEFT | 4
    frame = M.synthetic_frames(1, 30, 80, seed=9, kind="smooth")[0]
    held = CS.encode_planes(NV12, cin, frame=frame)
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 80, 30, 4) as b:
        assert b.stat("tiles") == 2
        want = CS.encode_planes(NV12, cout, frame=b.run(CS.decode_planes(NV12, cin, held)))
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 80, 30, 4) as tr:
        got = [np.zeros((120, 320), np.uint8), np.zeros((60, 320), np.uint8)]
        tr.process_frame(R.host_frame(NV12, held, cin), R.host_frame(NV12, got, cout))
        assert same(got, want)


# ---- 4. the refused values ----------------------------------------------------------------------------------------------
def test_refused_values_leave_the_runtime_as_it_was():
    t = twin()
    h, w = t["h"], t["w"]
    bad = {"siting 3": (3 << 8 | 2, "chroma siting 3"), "bit 10": (1 << 10 | 2, "bits above bit 9"), "low byte 6": (6, "colour space 6")}
    with R.Runtime(t["blob"], 0, R.DTYPE_F16) as a:
        got = blank_p010(4 * h, 4 * w)
        for name, (value, words) in bad.items():
            for side in ("input", "output"):
                fin = R.host_frame(NV12, t["held"][0], value if side == "input" else IN_CS[0])
                fout = R.host_frame(P010, got, value if side == "output" else OUT_CS[0])
                for call in (lambda: a.process_frame(fin, fout), lambda: a.process_frames([fin], [fout])):
                    with pytest.raises(R.JoshUpscaleError) as e:
                        call()
                    assert e.value.code == 1 and words in e.value.message and side in e.value.message, (name, side, e.value.message)
                    if name == "low byte 6":
                        assert "colour space" in e.value.message
        assert not any(p.any() for p in got)
        # nothing ran: the stream goes on as the twin's that never saw a bad call
        for k in range(3):
            a.process_frame(R.host_frame(NV12, t["held"][k], IN_CS[k]), R.host_frame(P010, got, OUT_CS[k]))
            assert same(got, t["want"][k]), k
    # an RGB frame keeps ignoring the whole field
    with R.Runtime(t["blob"], 0, R.DTYPE_F16) as a, R.Runtime(t["blob"], 0, R.DTYPE_F16) as b:
        frame = M.synthetic_frames(1, h, w, seed=31, kind="smooth")[0]
        rgb = np.ascontiguousarray(frame[..., 2::-1])
        out = np.zeros((4 * h, 4 * w, 4), np.uint8)
        a.process_frame(R.host_frame(R.FMT_RGB24, [rgb], 0x7fff), R.host_frame(R.FMT_BGRX, [out]))
        assert np.array_equal(out, b.process_image(frame))
