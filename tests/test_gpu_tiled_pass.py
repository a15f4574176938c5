"""Look-ahead passes of a tiled object on the GPU (csrc/tile_kernels.hip tile_split_frames_kernel, tiled.cpp; docs/tiled.md
"Look-ahead passes") -- needs an MI355X.

The kernel alone through its hook against the numpy definition applied frame by frame (tests/tiled_reference.py split),
byte for byte, the frames of ONE launch differing in alignment, padding and row order; then ju_tiled_process_frames /
ju_tiled_process_batch against a TWIN tiled object driven frame by frame through ju_tiled_process_frame -- which the
existing tests hold to the numpy definition -- byte for byte in every plane and every byte around it, with one more frame
through ju_tiled_process_frame on both afterwards, so that the states are equal too."""

import ctypes as C

import numpy as np
import pytest

import tiled_pass_reference as P
import tiled_reference as T
import tiled_scene_reference as TS
import yuv_reference as Y
from helpers import M
from joshupscale_amd import runtime as R
from test_gpu_tiled import LAYOUTS, small_blob
from test_gpu_yuv import DevPlane, torch_dev

pytestmark = pytest.mark.gpu

JU_ERR_INVALID_ARGUMENT = 1
W, H = 48, 30                                    # helpers.small_config()
GUARD = 0xEE
CS = R.CS_BT709_LIMITED
ORDER = ["dense", "off-16", "padded", "bottom-up", "off-16-bottom-up"]      # LAYOUTS, rotating across the frames of a launch


# ---- 1. tile_split_frames_kernel alone ---------------------------------------------------------------------------------------
def slots(frames, tiles, tile_bytes=W * H * 4):
    """K x T tile slots in one device buffer filled with 0xA5, each with 256 guard bytes or more behind its tile:
    (tensor [K, T, per], pointers of frame 0, the slot stride)."""
    torch, dev = torch_dev()
    per = -(-(tile_bytes + 256) // 256) * 256
    buf = torch.full((frames, tiles, per), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    ptrs = (C.c_void_p * tiles)(*[buf.data_ptr() + k * per for k in range(tiles)])
    return buf, ptrs, tiles * per


def split_frames(planes, sw, sh, ov, ptrs, slot, n, w=W, h=H):
    lib = R.load_library(True)
    k = len(planes)
    rc = lib.ju_debug_tile_split_frames((C.c_void_p * k)(*[p.ptr for p in planes]), (C.c_ssize_t * k)(*[p.stride for p in planes]),
                                        k, sw, sh, w, h, ov, ptrs, slot, n)
    assert rc == 0, lib.ju_last_error()


@pytest.mark.parametrize("frames", [1, 2, 3, 8])
def test_split_frames_kernel_equals_the_definition_frame_by_frame(frames):
    torch, dev = torch_dev()
    case = 0
    for sw, sh in [(49, 31), (80, 30), (100, 70)]:
        rng = np.random.default_rng(sw * 100 + sh + frames)
        srcs = rng.integers(0, 256, (frames, sh, sw, 4), dtype=np.uint8)      # (X random: written as 0)
        for ov in (0, 4, 7):
            # one launch holds a 16-byte-aligned frame, one at 4 mod 16, a padded one and bottom-up ones
            layouts = [ORDER[(case + f) % len(ORDER)] for f in range(frames)]
            case += 1
            planes = [DevPlane(srcs[f], **LAYOUTS[layouts[f]]) for f in range(frames)]
            want = [T.split(srcs[f], W, H, ov) for f in range(frames)]
            n = len(want[0])
            buf, ptrs, slot = slots(frames, n)
            torch.cuda.synchronize()
            split_frames(planes, sw, sh, ov, ptrs, slot, n)
            got = buf.cpu().numpy()
            for f in range(frames):
                for k, tile in enumerate(want[f]):
                    assert np.array_equal(got[f, k, :tile.size].reshape(tile.shape), tile), (sw, sh, ov, layouts, f, k)
                    assert (got[f, k, tile.size:] == 0xA5).all(), (sw, sh, ov, f, k)      # (nothing behind a tile's slot)
                planes[f].check(srcs[f])                           # (the source and the bytes around it untouched)


def test_split_frames_kernel_at_the_grids_limit():
    """384 x 240 at overlap 0: 8 x 8 = 64 tiles, x 8 frames = 512 slices of the grid."""
    torch, dev = torch_dev()
    sw, sh, frames = 384, 240, 8
    assert T.problem(sw, sh, W, H, 0) == ""
    rng = np.random.default_rng(3)
    srcs = rng.integers(0, 256, (frames, sh, sw, 4), dtype=np.uint8)
    planes = [DevPlane(srcs[f], **LAYOUTS[ORDER[f % len(ORDER)]]) for f in range(frames)]
    buf, ptrs, slot = slots(frames, 64)
    torch.cuda.synchronize()
    split_frames(planes, sw, sh, 0, ptrs, slot, 64)
    got = buf.cpu().numpy()
    for f in range(frames):
        want = T.split(srcs[f], W, H, 0)
        assert len(want) == 64
        for k, tile in enumerate(want):
            assert np.array_equal(got[f, k, :tile.size].reshape(tile.shape), tile), (f, k)
        assert (got[f, :, W * H * 4:] == 0xA5).all(), f


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_one_frame_is_the_single_frame_kernel(layout):
    torch, dev = torch_dev()
    lib = R.load_library(True)
    rng = np.random.default_rng(41)
    for sw, sh, ov in [(49, 31, 0), (100, 70, 4), (100, 70, 7)]:
        src = rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8)
        plane = DevPlane(src, **LAYOUTS[layout])
        n = len(T.split(src, W, H, ov))
        a, pa, slot = slots(1, n)
        b, pb, _ = slots(1, n)
        torch.cuda.synchronize()
        split_frames([plane], sw, sh, ov, pa, slot, n)
        assert lib.ju_debug_tile_split(plane.ptr, plane.stride, sw, sh, W, H, ov, pb, n) == 0, lib.ju_last_error()
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), (sw, sh, ov)


def test_the_hook_refuses_before_a_launch():
    lib = R.load_library(True)
    buf, ptrs, slot = slots(3, 9)
    src = np.zeros((70, 100, 4), np.uint8)
    planes = [DevPlane(src) for _ in range(3)]

    def call(ps=None, strides=None, frames=3, sw=100, ov=4, t=ptrs, s=slot, n=9):
        ps = [p.ptr for p in planes] if ps is None else ps
        strides = [p.stride for p in planes] if strides is None else strides
        return lib.ju_debug_tile_split_frames((C.c_void_p * len(ps))(*ps), (C.c_ssize_t * len(strides))(*strides), frames, sw, 70, W, H,
                                              ov, t, s, n)
    base = [p.ptr for p in planes]
    odd = (C.c_void_p * 9)(*[ptrs[k] + (8 if k == 5 else 0) for k in range(9)])
    for kw, word in [(dict(frames=0), "1 .. 8 frames"), (dict(frames=9), "1 .. 8 frames"), (dict(ov=8), "overlap"),
                     (dict(n=4), "9 tiles"), (dict(sw=47), "source size"), (dict(t=odd), "tile 5"),
                     (dict(ps=[base[0], None, base[2]]), "null buffer (frame 1)"),
                     (dict(ps=[base[0], base[1], base[2] + 2]), "multiples of 4 (frame 2)"),
                     (dict(strides=[400, 402, 400]), "multiples of 4 (frame 1)"),
                     (dict(strides=[400, 400, 396]), "smaller than a row (frame 2)"),
                     (dict(s=slot + 8), "multiple of 16"), (dict(s=W * H * 4 - 16), "hold a tile")]:
        assert call(**kw) == JU_ERR_INVALID_ARGUMENT, kw
        assert word in lib.ju_last_error().decode(), (word, lib.ju_last_error())
    assert (buf.cpu().numpy() == 0xA5).all()
    for p in planes:
        p.check(src)


# ---- 2. end to end against a twin driven frame by frame --------------------------------------------------------------------
class Plane:
    """[rows][row bytes] inside a buffer of GUARD bytes, in host or device memory: rows `pad` bytes apart beyond their own,
    the first `offset` bytes behind a 64-byte guard, bottom-up when `flip`."""

    def __init__(self, data, device, pad=0, offset=0, flip=False):
        rows = np.ascontiguousarray(data).reshape(data.shape[0], -1).view(np.uint8)
        self.rows, self.row_bytes = rows.shape
        self.pitch, self.lead, self.flip, self.device = self.row_bytes + pad, 64 + offset, flip, device
        host = np.full(self.lead + self.rows * self.pitch + 64, GUARD, np.uint8)
        self.body(host)[...] = rows
        self.initial = host.copy()
        if device:
            torch, dev = torch_dev()
            self.buf = torch.from_numpy(host).to(dev)
            self.base = self.buf.data_ptr()
        else:
            self.buf = host
            self.base = host.ctypes.data

    def body(self, whole):
        b = whole[self.lead:self.lead + self.rows * self.pitch].reshape(self.rows, self.pitch)[:, :self.row_bytes]
        return b[::-1] if self.flip else b

    @property
    def ptr(self):
        return self.base + self.lead + ((self.rows - 1) * self.pitch if self.flip else 0)

    @property
    def stride(self):
        return -self.pitch if self.flip else self.pitch

    def whole(self):
        return self.buf.cpu().numpy() if self.device else self.buf.copy()

    def around_untouched(self):
        got, want = self.whole(), self.initial.copy()
        self.body(want)[...] = self.body(got)
        return np.array_equal(got, want)


def frame_of(fmt, planes, w, h, device):
    f = R.device_frame(fmt, w, h, [p.ptr for p in planes], [p.stride for p in planes], colorspace=CS)
    f.location = R.LOC_DEVICE if device else R.LOC_CPU
    return f


# kind: (input format, on the device, layout), (output format, on the device, layout)
DENSE, PADDED, UP, OFF = dict(), dict(pad=48), dict(pad=16, flip=True), dict(pad=4, offset=4)
KINDS = {
    "dev": ((R.FMT_BGRX, True, DENSE), (R.FMT_BGRX, True, DENSE)),
    "dev-off16": ((R.FMT_BGRX, True, OFF), (R.FMT_BGRX, True, UP)),
    "host": ((R.FMT_BGRX, False, DENSE), (R.FMT_BGRX, False, DENSE)),
    "host-up": ((R.FMT_BGRX, False, UP), (R.FMT_BGRX, False, UP)),
    "nv12-host": ((R.FMT_NV12, False, PADDED), (R.FMT_NV12, False, DENSE)),
    "nv12-dev": ((R.FMT_NV12, True, DENSE), (R.FMT_NV12, True, PADDED)),
    "p010-host": ((R.FMT_BGRX, False, DENSE), (R.FMT_P010, False, PADDED)),
    "p010-dev": ((R.FMT_BGRX, True, DENSE), (R.FMT_P010, True, DENSE)),
    "nv12-host-to-dev": ((R.FMT_NV12, False, DENSE), (R.FMT_BGRX, True, PADDED)),
    "dev-to-nv12-host": ((R.FMT_BGRX, True, UP), (R.FMT_NV12, False, UP)),
}


class IO:
    """The input and the output of one frame of one kind, for ONE object (its twin gets buffers of its own)."""

    def __init__(self, kind, frame, ow, oh):
        (ifmt, idev, ilay), (ofmt, odev, olay) = KINDS[kind]
        sh, sw = frame.shape[:2]
        if ifmt == R.FMT_BGRX:
            data = [frame]
        else:
            y, u, v = Y.encode(frame, CS)
            data = [y, Y.to_nv12(u, v)]
        self.ins = [Plane(d, idev, **ilay) for d in data]
        sample = {R.FMT_BGRX: 4, R.FMT_NV12: 1, R.FMT_P010: 2}[ofmt]
        shapes = [(oh, ow * 4)] if ofmt == R.FMT_BGRX else [(oh, ow * sample), (oh // 2, ow * sample)]
        self.outs = [Plane(np.full(s, 0x5A, np.uint8), odev, **olay) for s in shapes]
        self.inp = frame_of(ifmt, self.ins, sw, sh, idev)
        self.out = frame_of(ofmt, self.outs, ow, oh, odev)


def equal_outputs(a, b, note):
    for k, (pa, pb) in enumerate(zip(a.outs, b.outs)):
        wa, wb = pa.whole(), pb.whole()
        assert np.array_equal(wa, wb), (note, k, int(np.count_nonzero(wa != wb)))
        assert pa.around_untouched(), (note, k)                   # nothing around the planes is written
        assert not (pa.body(wa) == 0x5A).all(), (note, k)         # (and the plane was)
    for p in a.ins:
        assert np.array_equal(p.whole(), p.initial), note         # the inputs are left alone


STATS = ["frames", "group_frames", "deep_state_frames", "output_scaled_frames", "source_mask_frames", "scene_frames", "scene_cuts"]


def drive(a, b, clip, kinds, calls=None, note="", stats=STATS):
    """`clip` through `a` in calls of `calls` frames (default: one call) and through `b` frame by frame, frame t of kind
    kinds[t % len(kinds)]; every output plane and every byte around it equal."""
    torch, dev = torch_dev()
    ow, oh = a.frame_output_size()
    assert (ow, oh) == b.frame_output_size()
    io_a = [IO(kinds[t % len(kinds)], f, ow, oh) for t, f in enumerate(clip)]
    io_b = [IO(kinds[t % len(kinds)], f, ow, oh) for t, f in enumerate(clip)]
    torch.cuda.synchronize()
    at = 0
    for n in calls or [len(clip)]:
        a.process_frames([io.inp for io in io_a[at:at + n]], [io.out for io in io_a[at:at + n]])
        at += n
    assert at == len(clip)
    for io in io_b:
        b.process_frame(io.inp, io.out)
    for t, (x, y) in enumerate(zip(io_a, io_b)):
        equal_outputs(x, y, (note, t, kinds[t % len(kinds)]))
    for key in stats:
        assert a.stat(key) == b.stat(key), (note, key, a.stat(key), b.stat(key))


def one_more(a, b, frame, note=""):
    """One more frame through ju_tiled_process_frame on both: the states a pass left are the twin's."""
    torch, dev = torch_dev()
    ow, oh = a.frame_output_size()
    x, y = IO("dev", frame, ow, oh), IO("dev", frame, ow, oh)
    torch.cuda.synchronize()
    a.process_frame(x.inp, x.out)
    b.process_frame(y.inp, y.out)
    equal_outputs(x, y, (note, "one more"))


_CLIPS = {}


def clip_of(sw, sh, n=12):
    if (sw, sh, n) not in _CLIPS:
        c = M.synthetic_frames(n, sh, sw, seed=5 + sw, kind="smooth")
        c.setflags(write=False)
        _CLIPS[(sw, sh, n)] = c
    return _CLIPS[(sw, sh, n)]


def pair(dtype=R.DTYPE_F16, sw=100, sh=70, ov=4):
    blob = small_blob()
    return R.TiledRuntime(blob, 0, dtype, sw, sh, ov), R.TiledRuntime(blob, 0, dtype, sw, sh, ov)


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("sw,sh,tiles", [(100, 70, 9), (80, 30, 2)])
def test_a_clip_in_one_call_equals_the_twin(sw, sh, tiles, dtype):
    """100 x 70 at overlap 4: 9 tiles, two group passes per frame; 80 x 30: 2 tiles, one."""
    clip = clip_of(sw, sh)
    a, b = pair(dtype, sw, sh)
    with a, b:
        assert a.stat("tiles") == tiles and a.stat("lookahead") == 8
        for kinds in (["dev"], ["host"], ["host-up"]):
            drive(a, b, clip[:4], kinds, note=kinds[0])
            one_more(a, b, clip[4], kinds[0])
            a.reset()                                             # a reset between calls
            b.reset()
        assert a.stat("pass_calls") == 3 and a.stat("pass_frames") == 12 and a.stat("pass_split_launches") == 3
        assert a.stat("pass_overlapped_copies") == 6 and b.stat("pass_frames") == 0 and b.stat("pass_overlapped_copies") == 0
        assert a.stat("group_frames") == tiles * 15 and a.stat("lookahead") == 8


@pytest.mark.parametrize("lookahead,passes", [(8, [8, 3]), (3, [3, 3, 3, 2])])
def test_eleven_frames_split_into_consecutive_passes(lookahead, passes):
    clip = clip_of(100, 70)
    assert [n for _, n in P.passes(11, lookahead)] == passes
    a, b = pair()
    with a, b:
        a.set_lookahead(lookahead)
        assert a.stat("lookahead") == lookahead
        drive(a, b, clip[:11], ["host", "dev"])
        one_more(a, b, clip[11])
        assert a.stat("pass_calls") == len(passes) and a.stat("pass_frames") == 11
        assert a.stat("pass_split_launches") == len(passes)
        # host outputs are the even frames: each but a pass's last is copied out under the next frame's group passes
        starts = P.plan(11, lookahead)
        last = {s + n - 1 for s, n in P.passes(11, lookahead)}
        assert a.stat("pass_overlapped_copies") == sum(1 for t in range(0, 11, 2) if t not in last)
        assert starts[0] == 0
        a.set_lookahead(99)
        assert a.stat("lookahead") == 8
        a.set_lookahead(-2)
        assert a.stat("lookahead") == 1
        a.reset()
        assert a.stat("lookahead") == 1                           # ju_tiled_reset keeps the cap


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_formats_and_places_rotate_within_one_call(dtype):
    clip = clip_of(100, 70)
    a, b = pair(dtype)
    with a, b:
        kinds = ["nv12-host", "dev", "host-up", "nv12-dev", "dev-off16", "p010-host", "nv12-host-to-dev", "dev-to-nv12-host"]
        drive(a, b, clip[:8], kinds)
        one_more(a, b, clip[8])
        assert a.stat("pass_calls") == 1 and a.stat("pass_frames") == 8 and a.stat("pass_split_launches") == 1


@pytest.mark.parametrize("kind", ["nv12-host", "nv12-dev"])
def test_nv12_in_and_out(kind):
    clip = clip_of(100, 70)
    a, b = pair()
    with a, b:
        drive(a, b, clip[:4], [kind])
        one_more(a, b, clip[4])
        assert a.stat("pass_frames") == 4 and a.stat("pass_overlapped_copies") == (3 if kind == "nv12-host" else 0)


@pytest.mark.parametrize("kind", ["p010-host", "p010-dev"])
def test_p010_from_the_states(kind):
    clip = clip_of(100, 70)
    a, b = pair()
    with a, b:
        for tr in (a, b):
            tr.set_deep_from_state(1)
            assert tr.stat("hbd_from_state") == 1
        drive(a, b, clip[:4], [kind])
        one_more(a, b, clip[4])
        assert a.stat("deep_state_frames") == 4 and a.stat("pass_frames") == 4


def rectangle_mask(sw, sh):
    """A HUD-like black rectangle across the first seam of both axes, edges off multiples of 4, on white."""
    m = np.full((4 * sh, 4 * sw, 4), 255, np.uint8)
    _, first_x, _ = T.layout(sw, W, 4)
    _, first_y, _ = T.layout(sh, H, 4)
    cx, cy = int(np.flatnonzero(np.diff(first_x))[0]), int(np.flatnonzero(np.diff(first_y))[0])
    m[cy - 21:cy + 18, cx - 35:cx + 30, :3] = 0
    return m


@pytest.mark.parametrize("setting", ["output-size", "black-mask", "rectangle-mask", "mask-and-output-size"])
def test_settings_are_not_told_about_passes(setting):
    clip = clip_of(100, 70)
    a, b = pair()
    with a, b:
        for tr in (a, b):
            if "output-size" in setting:
                tr.set_output_size(300, 210, R.SCALE_MITCHELL if setting == "output-size" else R.SCALE_TRIANGLE)
            if setting == "black-mask":
                tr.set_source_mask(np.zeros((3, 2, 4), np.uint8))
            if setting in ("rectangle-mask", "mask-and-output-size"):
                tr.set_source_mask(rectangle_mask(100, 70))
        if "mask" in setting:
            assert a.stat("source_mask") == 1 and a.stat("mask_box_x1") > a.stat("mask_box_x0")
        drive(a, b, clip[:5], ["host", "dev", "nv12-host", "host-up", "dev-off16"])
        one_more(a, b, clip[5])
        assert a.stat("pass_frames") == 5 and a.stat("pass_split_launches") == 1
        assert a.stat("output_scaled_frames") == (6 if "output-size" in setting else 0)
        assert a.stat("source_mask_frames") == (6 if "mask" in setting else 0)


# ---- 3. the scene detector ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [R.SCENE_REPORT, R.SCENE_RESET], ids=["report", "reset"])
def test_the_scene_detector_inside_passes(mode):
    """The known clip at 100 x 70 (cuts at 4, 7, 10, 12) in passes of four: a cut on a pass's first frame (4, 12), in the
    middle of one (10) and on its last (7)."""
    thr = 18500
    clip = TS.known_clip(M.synthetic_frames, 70, 100)
    recs = TS.run(clip, thr)
    assert TS.cuts(recs) == [4, 7, 10, 12] and P.plan(13, 4) == [0, 4, 8, 12]
    a, b = pair()
    with a, b:
        for tr in (a, b):
            tr.set_scene_detect(mode, thr)
        a.set_lookahead(4)
        drive(a, b, clip, ["dev", "host", "host-up"])
        assert a.scene_info() == b.scene_info() == recs
        assert a.stat("scene_cuts") == 4 and a.stat("scene_frames") == 13
        assert a.stat("pass_calls") == 3 and a.stat("pass_frames") == 12
        assert a.stat("pass_split_launches") == 0                 # the fused per-frame split stays while the detector is on
        one_more(a, b, clip[3])
        assert a.scene_info(1) == b.scene_info(1)
        for tr in (a, b):                                         # the detector off again: the multi-frame split
            tr.set_scene_detect(R.SCENE_OFF, 0)
        drive(a, b, clip[:4], ["dev"])
        assert a.stat("pass_split_launches") == 1


# ---- 4. routes ----------------------------------------------------------------------------------------------------------------
def test_the_stats_of_an_all_host_call():
    clip = clip_of(100, 70)
    a, b = pair()
    with a, b:
        drive(a, b, clip[:4], ["host"])
        assert a.stat("pass_frames") == 4 and a.stat("pass_split_launches") == 1 and a.stat("pass_overlapped_copies") == 3
        assert a.stat("group_frames") == 36 and a.stat("pass_calls") == 1 and a.stat("frames") == 4


def test_an_output_over_a_later_input_starts_a_new_pass():
    """outputs[1] holds inputs[2] (device): frame 2 reads what frame 1 wrote, as frame by frame -- two passes."""
    torch, dev = torch_dev()
    clip = clip_of(100, 70)
    a, b = pair()
    with a, b:
        results = []
        for tr, batch in ((a, True), (b, False)):
            ins = [torch.from_numpy(np.array(f)).to(dev) for f in clip[:4]]
            outs = [torch.full((280, 400, 4), 0x5A, dtype=torch.uint8, device=dev) for _ in range(4)]
            torch.cuda.synchronize()
            fi = [R.JuImage(t.data_ptr(), R.LOC_DEVICE, 400, 100, 70) for t in ins]
            fo = [R.JuImage(t.data_ptr(), R.LOC_DEVICE, 1600, 400, 280) for t in outs]
            fi[2] = R.JuImage(outs[1].data_ptr() + 1600 * 100 + 400, R.LOC_DEVICE, 1600, 100, 70)   # a window of outputs[1]
            if batch:
                tr.process_batch(fi, fo)
            else:
                for i, o in zip(fi, fo):
                    tr.process(i, o)
            results.append([t.cpu().numpy() for t in outs])
        for t in range(4):
            assert np.array_equal(results[0][t], results[1][t]), t
        assert not np.array_equal(results[0][2], results[0][3])
        assert a.stat("pass_calls") == 2 and a.stat("pass_frames") == 4 and a.stat("frames") == 4
        one_more(a, b, clip[4])


def test_outputs_may_repeat():
    """outputs[0] is outputs[2] (host): the buffer ends up holding frame 2."""
    clip = clip_of(100, 70)
    a, b = pair()
    with a, b:
        outs = [np.full((280, 400, 4), 0x5A, np.uint8) for _ in range(3)]
        ins = [np.ascontiguousarray(f) for f in clip[:4]]
        a.process_batch([R.host_image(f) for f in ins], [R.host_image(outs[t]) for t in (0, 1, 0, 2)])
        want = [b.run(f) for f in ins]
        assert np.array_equal(outs[0], want[2]) and np.array_equal(outs[1], want[1]) and np.array_equal(outs[2], want[3])
        assert a.stat("pass_calls") == 1 and a.stat("pass_frames") == 4 and a.stat("pass_overlapped_copies") == 3
        one_more(a, b, clip[4])


def test_a_one_tile_object_equals_a_plain_runtime():
    blob = small_blob()
    clip = clip_of(W, H)
    with R.Runtime(blob, 0, R.DTYPE_F16) as rt, R.TiledRuntime(blob, 0, R.DTYPE_F16, W, H, 7) as tr:
        assert tr.stat("tiles") == 1
        x = [IO(k, f, 4 * W, 4 * H) for k, f in zip(["host", "dev", "nv12-host", "host-up", "dev"], clip[:5])]
        y = [IO(k, f, 4 * W, 4 * H) for k, f in zip(["host", "dev", "nv12-host", "host-up", "dev"], clip[:5])]
        tr.process_frames([io.inp for io in x], [io.out for io in x])
        rt.process_frames([io.inp for io in y], [io.out for io in y])
        for t, (p, q) in enumerate(zip(x, y)):
            equal_outputs(p, q, t)
        assert tr.stat("pass_frames") == 5 and tr.stat("group_frames") == 0 and tr.stat("frames") == 5
        assert tr.stat("pass_overlapped_copies") == 0             # one tile: no group pass to copy under


def test_an_object_created_under_ju_lookahead_1_runs_frame_by_frame(monkeypatch):
    clip = clip_of(100, 70)
    blob = small_blob()
    monkeypatch.setenv("JU_LOOKAHEAD", "1")
    a = R.TiledRuntime(blob, 0, R.DTYPE_F16, 100, 70, 4)
    monkeypatch.delenv("JU_LOOKAHEAD")
    b = R.TiledRuntime(blob, 0, R.DTYPE_F16, 100, 70, 4)
    with a, b:
        assert a.stat("lookahead") == 1 and b.stat("lookahead") == 8
        # (the members of `a` have a look-ahead of 1 too: its tiles run one by one, so "group_frames" is 0 for it alone)
        drive(a, b, clip[:4], ["host", "dev"], stats=[k for k in STATS if k != "group_frames"])
        assert a.stat("pass_frames") == 0 and a.stat("pass_calls") == 0 and a.stat("frames") == 4
        assert a.stat("group_frames") == 0 and b.stat("group_frames") == 36
        one_more(a, b, clip[4])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing():
    torch, dev = torch_dev()
    lib = R.load_library()
    clip = clip_of(100, 70)
    a, b = pair()
    with a, b:
        drive(a, b, clip[:2], ["dev"])
        ios = [IO("dev" if t % 2 else "host", f, 400, 280) for t, f in enumerate(clip[2:6])]
        torch.cuda.synchronize()
        ins, outs = (R.JuFrame * 4)(*[io.inp for io in ios]), (R.JuFrame * 4)(*[io.out for io in ios])
        before = {k: a.stat(k) for k in STATS + ["pass_calls", "pass_frames", "pass_split_launches", "pass_overlapped_copies"]}

        def refused(rc, word):
            message = lib.ju_last_error().decode()
            assert rc == JU_ERR_INVALID_ARGUMENT and word in message, (rc, word, message)

        ins[2].width = 99                                         # a wrong-size frame at index 2 of 4
        refused(lib.ju_tiled_process_frames(a._h, ins, outs, 4), "ju_tiled_process_frames: frame 2: input image must be exactly 100x70")
        ins[2].width = 100
        outs[3].strides[0] = 1596
        refused(lib.ju_tiled_process_frames(a._h, ins, outs, 4), "frame 3: |stride| smaller than a row")
        outs[3].strides[0] = 1600
        keep = ins[1].format
        ins[1].format = 99
        refused(lib.ju_tiled_process_frames(a._h, ins, outs, 4), "frame 1: frame has an unknown format 99")
        ins[1].format = keep
        images = (R.JuImage * 4)(*[R.JuImage(io.ins[0].ptr, R.LOC_DEVICE if io.ins[0].device else R.LOC_CPU, io.ins[0].stride, 100, 70)
                                   for io in ios])
        results = (R.JuImage * 4)(*[R.JuImage(io.outs[0].ptr, R.LOC_DEVICE if io.outs[0].device else R.LOC_CPU, io.outs[0].stride,
                                              400, 280) for io in ios])
        results[1].height = 279
        refused(lib.ju_tiled_process_batch(a._h, images, results, 4), "ju_tiled_process_batch: frame 1: output image must be exactly 400x280")
        results[1].height = 280
        refused(lib.ju_tiled_process_frames(a._h, ins, outs, -1), "NULL frames or a negative count")
        refused(lib.ju_tiled_process_frames(a._h, None, outs, 4), "NULL frames or a negative count")
        refused(lib.ju_tiled_process_frames(a._h, ins, None, 4), "NULL frames or a negative count")
        refused(lib.ju_tiled_process_batch(a._h, None, results, 4), "NULL images or a negative count")
        refused(lib.ju_tiled_process_batch(a._h, images, results, -3), "NULL images or a negative count")
        assert lib.ju_tiled_process_frames(a._h, None, None, 0) == 0     # count == 0 is a no-op
        assert lib.ju_tiled_process_batch(a._h, images, results, 0) == 0
        assert {k: a.stat(k) for k in before} == before
        for io in ios:                                            # nothing was uploaded, launched or written
            for p in io.outs + io.ins:
                assert np.array_equal(p.whole(), p.initial)
        # the same call, whole, through ju_tiled_process_batch; then the next frame equals the twin's: nothing had changed
        assert lib.ju_tiled_process_batch(a._h, images, results, 4) == 0, lib.ju_last_error()
        twin = [IO("dev" if t % 2 else "host", f, 400, 280) for t, f in enumerate(clip[2:6])]
        torch.cuda.synchronize()
        for io in twin:
            b.process_frame(io.inp, io.out)
        for t, (x, y) in enumerate(zip(ios, twin)):
            equal_outputs(x, y, t)
        one_more(a, b, clip[6])
