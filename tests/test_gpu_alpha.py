"""The alpha channel on the GPU (csrc/alpha_kernels.hip, engine_frames.cpp "Alpha"; docs/alpha.md): the two kernels alone
against the numpy definition (tests/alpha_reference.py), code for code, with every other bit of the destination held; a
runtime under ju_set_alpha against a twin in mode 0 fed the same frames -- colour and state the twin's, alpha the
definition's -- on every entry point; the routing; turning it off; the refused calls."""

import functools

import numpy as np
import pytest

import alpha_reference as A
import scale_filter_reference as F
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_source import make_mask, same_state
from test_gpu_yuv import DevPlane, torch_dev

pytestmark = pytest.mark.gpu

BGRX, NV12, RGBX, BGRX64, X2RGB10 = R.FMT_BGRX, R.FMT_NV12, R.FMT_RGBX, R.FMT_BGRX64, R.FMT_X2RGB10
KIND_INDEX = {k: i for i, k in enumerate(A.KINDS)}

# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------
# (source, destination) as (H, W): the model's ratio; the identity; an odd source (rows off 16-byte alignment); down and up
# at once; 16 : 1 (33 taps, two tiles across: the triangle only); 8 : 1 (the cubic limit); 1 : 16; the checkerboard's 1 : 4
SHAPES = [((30, 48), (120, 192)), ((16, 24), (16, 24)), ((17, 23), (16, 24)), ((16, 24), (7, 50)), ((64, 1024), (4, 64)),
          ((64, 512), (8, 64)), ((4, 6), (64, 96)), ((16, 24), (64, 96))]
CONTENTS = ("random", "zero", "top", "checkerboard")
# layouts of a side, as DevPlane takes them; the offsets are the address phases the kind allows
SRC_LAYOUTS = {"byte": [dict(), dict(offset=1, pad=12), dict(pad=16, flip=True), dict(offset=1, pad=3, flip=True)],
               "word": [dict(), dict(offset=2, pad=6), dict(pad=16, flip=True)],
               "bits": [dict(), dict(offset=4, pad=12), dict(pad=16, flip=True)]}
SINK_LAYOUTS = {"byte": [dict(), dict(offset=1, pad=5), dict(offset=4), dict(offset=8, pad=8), dict(offset=12), dict(pad=3, flip=True)],
                "word": [dict(), dict(offset=2, pad=6), dict(pad=16, flip=True)],
                "bits": [dict(), dict(offset=4, pad=12), dict(pad=16, flip=True)]}


def filters_of(src, dst):
    return [f for f in F.FILTERS if src[0] <= F.down_max(f) * dst[0] and src[1] <= F.down_max(f) * dst[1]]


@functools.lru_cache(maxsize=None)
def source_codes(kind, content, hw):
    """The alpha codes of a source of `kind`; the checkerboard and "top" are the plane's two ends in every width."""
    top = A.TOP[kind]
    if content == "random":
        codes = np.random.default_rng(hw[0] * 131 + hw[1]).integers(0, top + 1, hw, dtype=np.int64)
    elif content == "zero":
        codes = np.zeros(hw, np.int64)
    elif content == "top":
        codes = np.full(hw, top, np.int64)
    else:
        codes = A.checkerboard(*hw) // 65535 * top
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def scaled_plane(kind, content, src, dst, filt):
    """A' of the definition: computed once, shared by the three sinks."""
    codes = None if kind == "none" else source_codes(kind, content, src)
    out = A.scale(A.plane(kind, codes, *src), *dst, filt)
    out.setflags(write=False)
    return out


def pixels(kind, hw, codes, seed):
    """Rows of pixels [H, W * pixel bytes] uint8 with random colour samples and `codes` in the alpha slot."""
    h, w = hw
    rng = np.random.default_rng(seed)
    if kind == "byte":
        px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        px[..., 3] = codes
    elif kind == "word":
        px = rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
        px[..., 3] = codes
    else:
        px = rng.integers(0, 1 << 30, (h, w), dtype=np.uint32) | (np.asarray(codes).astype(np.uint32) << 30)
    return np.ascontiguousarray(px).view(np.uint8).reshape(h, -1)


def alpha_scale(src_kind, sink_kind, filt, dst, dst_hw, src, src_hw):
    lib = R.load_library(True)
    return lib.ju_debug_alpha_scale(KIND_INDEX[src_kind], KIND_INDEX[sink_kind], filt, dst.ptr, dst.stride, dst_hw[1], dst_hw[0],
                                    src.ptr if src else None, src.stride if src else 0, src_hw[1], src_hw[0])


def alpha_fill(sink_kind, dst, dst_hw):
    return R.load_library(True).ju_debug_alpha_fill(KIND_INDEX[sink_kind], dst.ptr, dst.stride, dst_hw[1], dst_hw[0])


def last_error():
    return R.load_library(True).ju_last_error().decode()


@pytest.mark.parametrize("sink_kind", ["byte", "word", "bits"])
@pytest.mark.parametrize("src_kind", A.KINDS)
def test_alpha_scale_kernel_equals_the_definition_code_for_code(src_kind, sink_kind):
    case = 0
    clamped = False
    for src_hw, dst_hw in SHAPES:
        for filt in filters_of(src_hw, dst_hw):
            for content in (CONTENTS if src_kind != "none" else ("top",)):
                # every layout at the model's ratio with random alpha; else the layouts in turn
                every = (src_hw, content) == ((30, 48), "random")
                src_lays = SRC_LAYOUTS.get(src_kind, [None])
                sink_lays = SINK_LAYOUTS[sink_kind]
                pairs = [(s, d) for s in src_lays for d in sink_lays] if every else \
                    [(src_lays[case % len(src_lays)], sink_lays[case % len(sink_lays)])]
                want_plane = scaled_plane(src_kind, content, src_hw, dst_hw, filt)
                want_codes = A.code(sink_kind, want_plane)
                if content == "top":
                    assert (want_codes == A.TOP[sink_kind]).all()
                if content == "zero":
                    assert (want_codes == 0).all()
                if content == "checkerboard" and filt == F.CATMULL_ROM and dst_hw[0] > src_hw[0]:
                    acc = A.sums(A.plane(src_kind, source_codes(src_kind, content, src_hw)), *dst_hw, filt)[1] >> 24
                    clamped |= bool(acc.min() < 0 and acc.max() > 65535)
                if src_hw == dst_hw and filt != F.MITCHELL and src_kind == sink_kind:
                    assert (want_codes == source_codes(src_kind, content, src_hw)).all()
                for src_lay, sink_lay in pairs:
                    case += 1
                    src_rows = d_src = None
                    if src_kind != "none":
                        src_rows = pixels(src_kind, src_hw, source_codes(src_kind, content, src_hw), case)
                        d_src = DevPlane(src_rows, **src_lay)
                    before = pixels(sink_kind, dst_hw, np.random.default_rng(case).integers(0, A.TOP[sink_kind] + 1, dst_hw), case + 1)
                    d_dst = DevPlane(before, **sink_lay)
                    rc = alpha_scale(src_kind, sink_kind, filt, d_dst, dst_hw, d_src, src_hw)
                    assert rc == 0, (last_error(), src_hw, dst_hw, filt, content, src_lay, sink_lay)
                    # every bit outside the slots survives (the same random colour, the wanted codes), and the guards
                    d_dst.check(pixels(sink_kind, dst_hw, want_codes, case + 1))
                    if d_src is not None:
                        d_src.check(src_rows)
    assert clamped or src_kind == "none"                                  # (the clamp was exercised: test_alpha_cpu.py)


@pytest.mark.parametrize("sink_kind", ["byte", "word", "bits"])
def test_alpha_fill_kernel_writes_the_top_code_and_nothing_else(sink_kind):
    case = 0
    for _, dst_hw in SHAPES + [((0, 0), (5, 130))]:
        for lay in SINK_LAYOUTS[sink_kind]:
            case += 1
            d_dst = DevPlane(pixels(sink_kind, dst_hw, np.zeros(dst_hw, np.int64), case), **lay)
            assert alpha_fill(sink_kind, d_dst, dst_hw) == 0, last_error()
            d_dst.check(pixels(sink_kind, dst_hw, np.full(dst_hw, A.TOP[sink_kind]), case))


def test_the_hooks_refuse_bad_arguments_before_any_launch():
    hw = (16, 24)
    rows = pixels("word", hw, np.zeros(hw, np.int64), 1)
    src, dst = DevPlane(rows), DevPlane(rows.copy())

    class At:                                                             # a side at another address or stride
        def __init__(self, ptr, stride):
            self.ptr, self.stride = ptr, stride
    for args, text in [(("byte", "byte", 1, dst, hw, src, hw), "unknown filter 1"),
                       (("byte", "byte", 0, At(None, 96), hw, src, hw), "NULL destination"),
                       (("byte", "byte", 0, dst, hw, At(None, 96), hw), "NULL source"),
                       (("byte", "byte", 0, At(dst.ptr, 95), hw, src, hw), "|stride| smaller than a row"),
                       (("byte", "byte", 0, dst, hw, At(src.ptr, -95), hw), "|stride| smaller than a row"),
                       (("word", "byte", 0, dst, hw, At(src.ptr + 1, 192), hw), "multiples of 2"),
                       (("byte", "word", 0, At(dst.ptr, 193), hw, src, hw), "multiples of 2"),
                       (("byte", "bits", 0, At(dst.ptr + 2, 96), hw, src, hw), "multiples of 4"),
                       (("bits", "byte", 0, dst, hw, At(src.ptr, 98), hw), "multiples of 4"),
                       (("byte", "byte", 0, dst, (1, 24), src, (17, 24)), "beyond a factor"),
                       (("byte", "byte", 0, dst, hw, src, (0, 24)), "1 .. 32768")]:
        assert alpha_scale(*args) == 1 and text in last_error(), (args[:3], last_error())
    lib = R.load_library(True)
    assert lib.ju_debug_alpha_scale(4, 0, 0, dst.ptr, 96, 24, 16, src.ptr, 96, 24, 16) == 1 and "source kind 4" in last_error()
    assert lib.ju_debug_alpha_scale(0, 3, 0, dst.ptr, 96, 24, 16, src.ptr, 96, 24, 16) == 1 and "sink kind 3" in last_error()
    assert lib.ju_debug_alpha_fill(3, dst.ptr, 96, 24, 16) == 1 and "sink kind 3" in last_error()
    assert lib.ju_debug_alpha_fill(0, None, 96, 24, 16) == 1 and "NULL destination" in last_error()
    assert lib.ju_debug_alpha_fill(1, dst.ptr, 190, 24, 16) == 1 and "smaller than a row" in last_error()
    src.check(rows)
    dst.check(rows)


# ---- 2. end to end -------------------------------------------------------------------------------------------------------
def blob_and_clip(n, seed=5):
    cfg = small_config()
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    return cfg, blob, M.synthetic_frames(n, cfg.frame_height, cfg.frame_width, seed=seed, kind="smooth")


def with_alpha(fmt, bgrx, seed):
    """(the frame's one array in `fmt` with random alpha in its slot, the codes) of a [H, W, 4] uint8 BGRX frame."""
    kind = A.kind_of(fmt)
    h, w = bgrx.shape[:2]
    codes = np.random.default_rng(seed).integers(0, A.TOP[kind] + 1, (h, w), dtype=np.int64)
    b, g, r = (bgrx[..., c].astype(np.uint32) for c in range(3))
    if fmt == BGRX:
        out = bgrx.copy()
        out[..., 3] = codes
    elif fmt == RGBX:
        out = np.stack([bgrx[..., 2], bgrx[..., 1], bgrx[..., 0], codes.astype(np.uint8)], axis=2)
    elif fmt == BGRX64:
        out = np.stack([b * 257, g * 257, r * 257, codes.astype(np.uint32)], axis=2).astype(np.uint16)
    else:
        ten = [(c << 2) | (c >> 6) for c in (b, g, r)]
        out = (ten[0] | (ten[1] << 10) | (ten[2] << 20) | (codes.astype(np.uint32) << 30)).astype(np.uint32)
    return np.ascontiguousarray(out), codes


def blank(fmt, h, w):
    if fmt == BGRX64:
        return np.full((h, w, 4), 0x5A5A, np.uint16)
    if fmt == X2RGB10:
        return np.full((h, w), 0x5A5A5A5A, np.uint32)
    return np.full((h, w, 4), 0x5A, np.uint8)


def split(fmt, arr):
    """(the array with its alpha slot cleared, the slot's codes)."""
    if fmt == X2RGB10:
        return arr & np.uint32(0x3fffffff), (arr >> 30).astype(np.int64)
    colour = arr.copy()
    colour[..., 3] = 0
    return colour, arr[..., 3].astype(np.int64)


def frame_of(fmt, arr, location, keep):
    """A ju_frame over `arr`: the host array, or a dense device copy kept in `keep`."""
    h, w = arr.shape[:2]
    if location == "host":
        keep.append(arr)
        return R.host_frame(fmt, [arr])
    torch, dev = torch_dev()
    rows = np.ascontiguousarray(arr).view(np.uint8).reshape(h, -1)
    t = torch.from_numpy(rows.copy()).to(dev)
    torch.cuda.synchronize()
    keep.append(t)
    return R.device_frame(fmt, w, h, [t], [rows.shape[1]])


def fetch(arr, location, keep):
    if location == "host":
        return arr
    return keep[-1].cpu().numpy().view(arr.dtype).reshape(arr.shape)


def run_frame(rt, in_fmt, in_arr, out_fmt, out_hw, location):
    """One ju_process_frame: the output array."""
    keep = []
    out = blank(out_fmt, *out_hw)
    fin = frame_of(in_fmt, in_arr, location, keep)
    fout = frame_of(out_fmt, out, location, keep)
    rt.process_frame(fin, fout)
    return fetch(out, location, keep)


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_ju_process_carries_the_alpha_and_leaves_colour_and_state_to_the_twin(dtype):
    cfg, blob, clip = blob_and_clip(8)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    filt = F.CATMULL_ROM if dtype == R.DTYPE_F16 else F.MITCHELL
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        assert a.get_alpha() == (0, 0) and a.stat("alpha_mode") == 0 and a.stat("alpha_frames") == 0
        a.set_alpha(R.ALPHA_SOURCE, filt)
        assert a.get_alpha() == (R.ALPHA_SOURCE, filt) and a.stat("alpha_mode") == 2 and a.stat("alpha_filter") == filt
        written = 0
        for t, f in enumerate(clip):
            frame, codes = with_alpha(BGRX, f, 100 + t)
            how = ("host", "bottom-up", "device", "enqueue")[t % 4]
            if t == 4:                                                    # OPAQUE from here; a reset keeps the setting
                a.set_alpha(R.ALPHA_OPAQUE, filt)
                a.reset()
                b.reset()
                assert a.get_alpha() == (R.ALPHA_OPAQUE, filt)
            outs = []
            for rt in (a, b):
                if how == "host":
                    out = rt.process_image(frame)
                elif how == "bottom-up":
                    store = np.empty((4 * h, 4 * w, 4), np.uint8)
                    out = rt.process_image(frame[::-1].copy()[::-1], store[::-1])
                else:
                    d_in = torch.from_numpy(frame).to(dev)
                    d_out = torch.full((4 * h, 4 * w, 4), 0x5A, dtype=torch.uint8, device=dev)
                    torch.cuda.synchronize()
                    pair = (rt.device_image(d_in.data_ptr(), w, h), rt.device_image(d_out.data_ptr(), 4 * w, 4 * h))
                    if how == "device":
                        rt.process(*pair)
                    else:
                        rt.enqueue(*pair)
                        rt.synchronize()
                    out = d_out.cpu().numpy()
                    assert np.array_equal(d_in.cpu().numpy(), frame)      # (the input untouched)
                outs.append(out)
            written += 1
            mode = R.ALPHA_SOURCE if t < 4 else R.ALPHA_OPAQUE
            want = A.alpha(mode, "byte", codes, (h, w), "byte", (4 * h, 4 * w), filt)
            assert np.array_equal(outs[0][..., :3], outs[1][..., :3]) and (outs[1][..., 3] == 0).all(), (t, how)
            assert np.array_equal(outs[0][..., 3], want), (t, how)
            assert same_state(a, b), (t, how)
            assert a.stat("alpha_frames") == written and b.stat("alpha_frames") == 0
        assert a.stat("lookahead_frames") == 0 and a.stat("source_stage_frames") == b.stat("source_stage_frames") == 0


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_ju_process_frame_carries_the_alpha_between_the_formats(dtype):
    cfg, blob, clip = blob_and_clip(6, seed=7)
    h, w = cfg.frame_height, cfg.frame_width
    fmts = (RGBX, BGRX64, X2RGB10)
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        a.set_alpha(R.ALPHA_SOURCE, F.TRIANGLE)
        for t, f in enumerate(clip):
            in_fmt, out_fmt = fmts[t % 3], fmts[(t + 1 + t // 3) % 3]     # (every format on either side, in and out differing and equal)
            location = ("host", "device")[t % 2]
            frame, codes = with_alpha(in_fmt, f, 200 + t)
            got = run_frame(a, in_fmt, frame, out_fmt, (4 * h, 4 * w), location)
            twin = run_frame(b, in_fmt, frame, out_fmt, (4 * h, 4 * w), location)
            colour, slot = split(out_fmt, got)
            twin_colour, twin_slot = split(out_fmt, twin)
            want = A.alpha(A.SOURCE, A.kind_of(in_fmt), codes, (h, w), A.kind_of(out_fmt), (4 * h, 4 * w))
            assert np.array_equal(colour, twin_colour) and (twin_slot == 0).all(), (t, in_fmt, out_fmt)
            assert np.array_equal(slot, want), (t, in_fmt, out_fmt)
            assert same_state(a, b)
        assert a.stat("alpha_frames") == len(clip)
        # an input without a slot: opaque
        keep = []
        yuv = [np.full((h, w), 90, np.uint8), np.full((h // 2, w), 128, np.uint8)]
        for rt, store in ((a, keep), (b, keep)):
            out = np.full((4 * h, 4 * w, 4), 0x5A, np.uint8)
            rt.process_frame(R.host_frame(NV12, yuv), R.host_frame(BGRX, [out]))
            store.append(out)
        assert np.array_equal(keep[0][..., :3], keep[1][..., :3]) and (keep[0][..., 3] == 255).all() and (keep[1][..., 3] == 0).all()
        assert a.stat("alpha_frames") == len(clip) + 1
        # an output without a slot: the twin's planes, and nothing launched
        frame, _ = with_alpha(BGRX, clip[0], 1)
        planes = []
        for rt in (a, b):
            out = [np.full((4 * h, 4 * w), 0x5A, np.uint8), np.full((2 * h, 4 * w), 0x5A, np.uint8)]
            rt.process_frame(R.host_frame(BGRX, [frame]), R.host_frame(NV12, out))
            planes.append(out)
        assert all(np.array_equal(x, y) for x, y in zip(*planes)) and same_state(a, b)
        assert a.stat("alpha_frames") == len(clip) + 1


def test_batches_and_groups_take_the_single_frame_route():
    cfg, blob, clip = blob_and_clip(8, seed=3)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    frames, codes = zip(*[with_alpha(BGRX, f, 300 + t) for t, f in enumerate(clip)])
    want = [A.alpha(A.SOURCE, "byte", c, (h, w), "byte", (4 * h, 4 * w)) for c in codes]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_alpha(R.ALPHA_SOURCE)
        for rt in (a, b):
            rt.set_stage_lookahead(1)                                     # (whatever the stage settings say)
            rt.set_stage_group(1)
        d_in = torch.from_numpy(np.stack(frames)).to(dev)
        outs = {}
        for rt in (a, b):
            d_out = torch.zeros((8, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ins = [rt.device_image(d_in[k].data_ptr(), w, h) for k in range(8)]
            dsts = [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(8)]
            if rt is a:
                assert rt.prepare_batch(ins[:4], dsts[:4]) == 0 and rt.prepare_frames(ins[0], dsts[0]) == 0
            rt.process_batch(ins[:4], dsts[:4])
            rt.process_frames([R.device_frame(BGRX, w, h, [d_in[k]]) for k in range(4, 8)],
                              [R.device_frame(BGRX, 4 * w, 4 * h, [d_out[k]]) for k in range(4, 8)])
            outs[rt] = d_out.cpu().numpy()
        assert a.stat("lookahead_frames") == 0 and b.stat("lookahead_frames") == 8 and a.stat("alpha_frames") == 8
        for k in range(8):
            assert np.array_equal(outs[a][k][..., :3], outs[b][k][..., :3]) and (outs[b][k][..., 3] == 0).all(), k
            assert np.array_equal(outs[a][k][..., 3], want[k]), k
        assert same_state(a, b)
    # a group: one alpha member beside two plain ones, which still ride
    with R.Runtime(blob, 0, R.DTYPE_F16) as p, R.Runtime(blob, 0, R.DTYPE_F16) as q, R.Runtime(blob, 0, R.DTYPE_F16) as a, \
            R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_alpha(R.ALPHA_SOURCE)
        members = [p, a, q]
        for t in range(2):
            d_in = torch.from_numpy(np.stack([frames[t], frames[t + 2], frames[t + 4]])).to(dev)
            d_out = torch.zeros((3, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            R.process_group(members, [m.device_image(d_in[i].data_ptr(), w, h) for i, m in enumerate(members)],
                            [m.device_image(d_out[i].data_ptr(), 4 * w, 4 * h) for i, m in enumerate(members)])
            got = d_out.cpu().numpy()
            twin = b.process_image(frames[t + 2])
            assert np.array_equal(got[1][..., :3], twin[..., :3]) and np.array_equal(got[1][..., 3], want[t + 2])
            assert (got[0][..., 3] == 0).all() and (got[2][..., 3] == 0).all() and same_state(a, b)
        assert p.stat("group_frames") == 2 and q.stat("group_frames") == 2 and a.stat("group_frames") == 0
        assert a.stat("alpha_frames") == 2


def test_sizes_and_a_mask_alpha_goes_straight_from_source_to_output():
    cfg, blob, clip = blob_and_clip(3, seed=11)
    sh, sw, oh, ow = 60, 96, 90, 144
    big = M.synthetic_frames(3, sh, sw, seed=12, kind="smooth")
    mask = make_mask((37, 50), 2)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        for rt in (a, b):
            rt.set_source_size(sw, sh, F.MITCHELL)
            rt.set_output_size(ow, oh, F.CATMULL_ROM)
            rt.set_source_mask(mask)
        a.set_alpha(R.ALPHA_SOURCE, F.CATMULL_ROM)
        for t, f in enumerate(big):
            frame, codes = with_alpha(BGRX, f, 400 + t)
            location = ("host", "device", "host")[t]
            got = run_frame(a, BGRX, frame, BGRX, (oh, ow), location)
            twin = run_frame(b, BGRX, frame, BGRX, (oh, ow), location)
            want = A.alpha(A.SOURCE, "byte", codes, (sh, sw), "byte", (oh, ow), F.CATMULL_ROM)
            assert np.array_equal(got[..., :3], twin[..., :3]) and (twin[..., 3] == 0).all()
            assert np.array_equal(got[..., 3], want) and same_state(a, b)
        # a deep output from the scaled state, and its word 3
        frame, codes = with_alpha(BGRX64, big[0], 9)
        a.set_source_mask(None)
        b.set_source_mask(None)
        got = run_frame(a, BGRX64, frame, BGRX64, (oh, ow), "device")
        twin = run_frame(b, BGRX64, frame, BGRX64, (oh, ow), "device")
        want = A.alpha(A.SOURCE, "word", codes, (sh, sw), "word", (oh, ow), F.CATMULL_ROM)
        assert np.array_equal(got[..., :3], twin[..., :3]) and (twin[..., 3] == 0).all() and np.array_equal(got[..., 3], want)
        assert a.stat("source_stage_frames") == b.stat("source_stage_frames")
        # source and output both 60 x 96: the alpha comes back byte for byte
        for rt in (a, b):
            rt.set_output_size(sw, sh, F.TRIANGLE)
        a.set_alpha(R.ALPHA_SOURCE, F.TRIANGLE)
        frame, codes = with_alpha(BGRX, big[1], 10)
        got = run_frame(a, BGRX, frame, BGRX, (sh, sw), "host")
        twin = run_frame(b, BGRX, frame, BGRX, (sh, sw), "host")
        assert np.array_equal(got[..., 3], frame[..., 3]) and np.array_equal(got[..., :3], twin[..., :3]) and same_state(a, b)


def test_mode_zero_again_is_a_runtime_that_never_had_the_setting():
    cfg, blob, clip = blob_and_clip(6, seed=13)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    frames = [with_alpha(BGRX, f, 500 + t)[0] for t, f in enumerate(clip)]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_alpha(R.ALPHA_SOURCE, F.MITCHELL)
        first = a.process_image(frames[0])
        assert np.array_equal(first[..., :3], b.process_image(frames[0])[..., :3]) and first[..., 3].any()
        a.set_alpha(R.ALPHA_ZERO, F.MITCHELL)
        assert a.get_alpha() == (0, F.MITCHELL) and a.stat("alpha_mode") == 0 and a.stat("alpha_frames") == 1
        keys = ("lookahead_frames", "graph_replays", "eager_runs", "source_stage_frames", "alpha_frames", "direct_graphs")
        base = {rt: {k: rt.stat(k) for k in keys} for rt in (a, b)}
        d_in = torch.from_numpy(np.stack(frames)).to(dev)
        outs = {}
        for rt in (a, b):
            d_out = torch.full((6, 4 * h, 4 * w, 4), 0x5A, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ins = [rt.device_image(d_in[k].data_ptr(), w, h) for k in range(6)]
            dsts = [rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h) for k in range(6)]
            rt.process(ins[0], dsts[0])
            rt.process(ins[1], dsts[1])
            rt.process_batch(ins[2:], dsts[2:])
            outs[rt] = d_out.cpu().numpy()
        assert np.array_equal(outs[a], outs[b]) and (outs[a][..., 3] == 0).all() and same_state(a, b)
        for key in keys:                                                  # (stat for stat, since the mode went back)
            assert a.stat(key) - base[a][key] == b.stat(key) - base[b][key], key
        assert a.stat("lookahead_frames") == 4 and a.stat("alpha_frames") == 1


def test_the_refused_calls_change_nothing():
    cfg, blob, clip = blob_and_clip(1)
    h, w = cfg.frame_height, cfg.frame_width
    torch, dev = torch_dev()
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        a.set_alpha(R.ALPHA_OPAQUE, F.CATMULL_ROM)
        for mode, filt in [(3, 0), (-1, 0), (R.ALPHA_SOURCE, 1), (R.ALPHA_ZERO, 4)]:
            with pytest.raises(ValueError, match="ju_set_alpha"):
                a.set_alpha(mode, filt)
            assert lib.ju_set_alpha(a._h, mode, filt) == 1                # (the C layer itself)
            assert lib.ju_last_error().decode() == "std::invalid_argument: ju_set_alpha: " + \
                R.alpha_problem(mode, filt, w, h, 4 * w, 4 * h)
            assert a.get_alpha() == (R.ALPHA_OPAQUE, F.CATMULL_ROM)
    # the ratio limits through each of the three setters: 16 : 1 in and 1 : 16 out are 64 : 1
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        def settings():
            return a.get_alpha(), a.get_source_size(), a.get_output_size()
        # ju_set_alpha: the sizes are there first
        a.set_source_size(16 * w, 16 * h)
        a.set_output_size(4 * w // 16, 4 * h // 16 + 1)
        keep = settings()
        text = R.alpha_problem(R.ALPHA_SOURCE, 0, 16 * w, 16 * h, 4 * w // 16, 4 * h // 16 + 1)
        assert text and "alpha" in text
        with pytest.raises(ValueError, match="ju_set_alpha"):
            a.set_alpha(R.ALPHA_SOURCE)
        assert lib.ju_set_alpha(a._h, R.ALPHA_SOURCE, 0) == 1
        assert lib.ju_last_error().decode() == "std::invalid_argument: ju_set_alpha: " + text and settings() == keep
        # ju_set_output_size: alpha and the source size are there first
        a.set_output_size(0, 0)
        a.set_alpha(R.ALPHA_SOURCE)                                       # (768 x 480 -> 192 x 120)
        keep = settings()
        with pytest.raises(ValueError, match="ju_set_output_size: alpha from the source"):
            a.set_output_size(4 * w // 16, 4 * h // 16 + 1)
        assert lib.ju_set_output_size(a._h, 4 * w // 16, 4 * h // 16 + 1, 0) == 1
        assert lib.ju_last_error().decode() == "std::invalid_argument: ju_set_output_size: " + text and settings() == keep
        # ju_set_source_size: alpha and the output size are there first
        a.set_source_size(0, 0)
        a.set_output_size(4 * w // 16, 4 * h // 16 + 1)                   # (48 x 30 -> 12 x 8)
        keep = settings()
        with pytest.raises(ValueError, match="ju_set_source_size: alpha from the source"):
            a.set_source_size(16 * w, 16 * h)
        assert lib.ju_set_source_size(a._h, 16 * w, 16 * h, 0) == 1
        assert lib.ju_last_error().decode() == "std::invalid_argument: ju_set_source_size: " + text and settings() == keep
        # ... and turning a size OFF can leave the limits as well: 3 x 2 -> 48 x 30 is fine, 3 x 2 -> the model's 192 x 120 is not
        a.set_alpha(R.ALPHA_ZERO)
        a.set_output_size(w, h)
        a.set_source_size(3, 2)
        a.set_alpha(R.ALPHA_SOURCE)
        keep = settings()
        with pytest.raises(ValueError, match="ju_set_output_size: alpha from the source"):
            a.set_output_size(0, 0)
        assert lib.ju_set_output_size(a._h, 0, 0, 0) == 1 and "3x2" in lib.ju_last_error().decode() and settings() == keep
        a.set_alpha(R.ALPHA_OPAQUE)
        a.set_output_size(0, 0)
        a.set_source_size(0, 0)
        # a frame still runs after all of this, opaque
        out = a.process_image(clip[0])
        assert (out[..., 3] == 255).all()
        # an overlapping device pair under ALPHA_SOURCE: refused before anything is launched
        a.set_alpha(R.ALPHA_SOURCE)
        buf = torch.zeros(4 * h * 4 * w * 4, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        before = a.stat("graph_replays") + a.stat("eager_runs")
        with pytest.raises(R.JoshUpscaleError, match="must not overlap"):
            a.process(a.device_image(buf.data_ptr(), w, h), a.device_image(buf.data_ptr(), 4 * w, 4 * h))
        with pytest.raises(R.JoshUpscaleError, match="must not overlap"):
            a.process_batch([a.device_image(buf.data_ptr(), w, h)], [a.device_image(buf.data_ptr(), 4 * w, 4 * h)])
        assert a.stat("graph_replays") + a.stat("eager_runs") == before and a.stat("alpha_frames") == 1
        a.set_alpha(R.ALPHA_OPAQUE)                                       # (nothing of the input is read behind the output)
        a.process(a.device_image(buf.data_ptr(), w, h), a.device_image(buf.data_ptr(), 4 * w, 4 * h))
