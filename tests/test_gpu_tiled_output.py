"""A tiled object's output size on the GPU (csrc/tile_kernels.hip tile_stitch_scale_kernel / tile_stitch_scale_state_kernel,
tiled.cpp stitchOut; docs/tiled.md "An output size") -- needs an MI355X.

Each fused kernel alone against the numpy definition (tests/tiled_output_reference.py), byte for byte, through its hook;
one tile against the existing scale kernels' hooks; the hooks' refusals; a ju_tiled with an output size against TWINS (one
plain runtime per tile, their outputs / 16-bit states blended, scaled and encoded in numpy), with no tolerance; a one-tile
object against a plain runtime under ju_set_output_size; turning the setting off and on; the refused calls; a scene cut."""

import ctypes as C

import numpy as np
import pytest

import output_reference as O
import scale_filter_reference as F
import tiled_deep_reference as D
import tiled_output_reference as TO
import tiled_reference as T
from helpers import M
from joshupscale_amd import runtime as R
from test_gpu_output import blank, byte_rows, same_planes
from test_gpu_tiled import tile_buffers, twins
from test_gpu_tiled_deep import clip_of, run, small_blob, states_of, twins16
from test_gpu_yuv import DevPlane, torch_dev
from test_tiled_output_cpu import GEOMETRIES, H, W, sizes, tiles_of

pytestmark = pytest.mark.gpu

JU_ERR_INVALID_ARGUMENT = 1
CS = R.CS_BT709_LIMITED
BGRX, NV12, P010, I410, BGRX64, RGBPH = R.FMT_BGRX, R.FMT_NV12, R.FMT_P010, R.FMT_I410, R.FMT_BGRX64, R.FMT_RGBPH
FORMATS = (BGRX, NV12, P010, I410, BGRX64, RGBPH)
NAMES = {BGRX: "bgrx", **O.NAMES}
# the 8-bit destination's rows: `offset` is the address phase mod 16 (DevPlane starts 64 bytes past a 256-byte boundary)
LAYOUTS = [dict(pad=0, offset=0, flip=False), dict(pad=8, offset=4, flip=False), dict(pad=16, offset=8, flip=False),
           dict(pad=4, offset=12, flip=False), dict(pad=3, offset=1, flip=False), dict(pad=16, offset=0, flip=True)]


class Sized:
    """A ju_tiled as test_gpu_tiled_deep.run sees it, with the frames' size in the place of the blended size."""

    def __init__(self, tr):
        self.tr = tr
        self.out_width, self.out_height = tr.frame_output_size()

    def process_frame(self, inp, out):
        self.tr.process_frame(inp, out)


def frame(tr, image, fmt, location, flip=False):
    return run(Sized(tr), image, fmt, location, flip)


# ---- 1. each fused kernel alone -------------------------------------------------------------------------------------------
_BLENDED = {}


def blended(sw, sh, ov):
    """(tiles, states, T.stitch of the tiles, D.stitch16 of the states' samples) of one geometry, computed once."""
    if (sw, sh, ov) not in _BLENDED:
        tiles, states = tiles_of(sw, sh, ov), states_of(sw, sh, ov)
        p = [D.p_from_state(s) for s in states]
        assert min(int(q.min()) for q in p) == 0 and max(int(q.max()) for q in p) == 65535           # both clamps of P
        b8, b16 = T.stitch(tiles, sw, sh, W, H, ov), D.stitch16(p, sw, sh, W, H, ov)
        b8.setflags(write=False)
        b16.setflags(write=False)
        _BLENDED[(sw, sh, ov)] = (tiles, states, b8, b16)
    return _BLENDED[(sw, sh, ov)]


@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_stitch_scale_kernel_equals_the_numpy_definition(sw, sh, ov):
    lib = R.load_library(True)
    tiles, _, b8, _ = blended(sw, sh, ov)
    buf, ptrs, _ = tile_buffers(tiles)
    before = buf.cpu().numpy()
    k = 0
    for filt in F.FILTERS:
        for name, (ow, oh) in sizes(sw, sh, filt).items():
            want = F.scale8(b8, oh, ow, filt)                         # (= TO.frame8(tiles, ...): the blend is shared)
            if name == "same" and filt != F.MITCHELL:
                assert np.array_equal(want, b8)
            lay = LAYOUTS[k % len(LAYOUTS)]
            k += 1
            d = DevPlane(np.full((oh, ow, 4), 0x5A, np.uint8), **lay)
            assert d.ptr % 16 == lay["offset"] or lay["flip"]
            rc = lib.ju_debug_tile_stitch_scale(d.ptr, d.stride, ow, oh, filt, sw, sh, W, H, ov, ptrs, len(tiles))
            assert rc == 0, lib.ju_last_error()
            d.check(want)                                             # (X = 0; the guard bytes around every row)
    assert k == 18 and np.array_equal(buf.cpu().numpy(), before)      # (every layout three times; the tiles untouched)


@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_stitch_scale_state_kernel_equals_the_numpy_definition(sw, sh, ov):
    lib = R.load_library(True)
    _, states, _, b16 = blended(sw, sh, ov)
    buf, ptrs, _ = tile_buffers([s.view(np.uint8) for s in states])
    before = buf.cpu().numpy()
    for filt in F.FILTERS:
        for name, (ow, oh) in sizes(sw, sh, filt).items():
            want = F.scale16(b16, oh, ow, filt)
            if name == "same" and filt != F.MITCHELL:
                assert np.array_equal(want, b16)
            d = DevPlane(np.full((oh, ow * 8), 0x5A, np.uint8))
            assert d.ptr % 8 == 0
            rc = lib.ju_debug_tile_stitch_scale_state(d.ptr, ow, oh, filt, sw, sh, W, H, ov, ptrs, len(states))
            assert rc == 0, lib.ju_last_error()
            assert (want[..., 3] == 0).all()
            d.check(byte_rows(want))                                  # (X words 0; the guard bytes around the frame)
    assert np.array_equal(buf.cpu().numpy(), before)                  # (the states untouched)


def test_the_definition_is_the_blend_then_the_scale():
    """What the two tests above compare with is TO.frame8 / TO.frame16 of the same tiles."""
    sw, sh, ov = 49, 31, 4
    tiles, states, b8, b16 = blended(sw, sh, ov)
    ow, oh = sizes(sw, sh, F.CATMULL_ROM)["odd"]
    assert np.array_equal(TO.frame8(tiles, sw, sh, W, H, ov, oh, ow, F.CATMULL_ROM), F.scale8(b8, oh, ow, F.CATMULL_ROM))
    p = [D.p_from_state(s) for s in states]
    assert np.array_equal(TO.frame16(p, sw, sh, W, H, ov, oh, ow, F.CATMULL_ROM), F.scale16(b16, oh, ow, F.CATMULL_ROM))


# ---- 2. one tile: the existing scale kernels' bytes -------------------------------------------------------------------------
@pytest.mark.parametrize("filt", F.FILTERS, ids=lambda f: F.NAMES[f])
def test_one_tile_equals_the_scale_kernels(filt):
    lib = R.load_library(True)
    sw, sh, ov = 48, 30, 7
    tiles, states, _, _ = blended(sw, sh, ov)
    buf8, ptrs8, _ = tile_buffers(tiles)
    buf16, ptrs16, _ = tile_buffers([s.view(np.uint8) for s in states])
    for name, (ow, oh) in sizes(sw, sh, filt).items():
        a, b = DevPlane(np.full((oh, ow, 4), 0x5A, np.uint8)), DevPlane(np.full((oh, ow, 4), 0x5A, np.uint8))
        assert lib.ju_debug_tile_stitch_scale(a.ptr, a.stride, ow, oh, filt, sw, sh, W, H, ov, ptrs8, 1) == 0, lib.ju_last_error()
        assert lib.ju_debug_scale(0, filt, b.ptr, b.stride, ow, oh, ptrs8[0], 4 * W * 4, 4 * W, 4 * H, None, None, None) == 0
        assert np.array_equal(a.buf.cpu().numpy(), b.buf.cpu().numpy()), name
        a, b = DevPlane(np.full((oh, ow * 8), 0x5A, np.uint8)), DevPlane(np.full((oh, ow * 8), 0x5A, np.uint8))
        assert lib.ju_debug_tile_stitch_scale_state(a.ptr, ow, oh, filt, sw, sh, W, H, ov, ptrs16, 1) == 0, lib.ju_last_error()
        assert lib.ju_debug_scale(1, filt, b.ptr, 0, ow, oh, ptrs16[0], 0, 4 * W, 4 * H, None, None, None) == 0
        assert np.array_equal(a.buf.cpu().numpy(), b.buf.cpu().numpy()), name


# ---- 3. the hooks' refusals ---------------------------------------------------------------------------------------------------
def test_the_hooks_refuse_before_a_launch():
    lib = R.load_library(True)
    buf, ptrs, slot = tile_buffers([np.zeros((4 * H, 4 * W, 8), np.uint8)] * 9)
    odd = (C.c_void_p * 9)(*[buf.data_ptr() + k * slot + (8 if k == 5 else 0) for k in range(9)])
    blank8, blank16 = np.full((210, 300, 4), 0x5A, np.uint8), np.full((210, 300 * 8), 0x5A, np.uint8)
    d8, d16 = DevPlane(blank8), DevPlane(blank16)

    def eight(dst=d8.ptr, stride=d8.stride, ow=300, oh=210, filt=0, sw=100, sh=70, ov=4, tiles=ptrs, n=9):
        return lib.ju_debug_tile_stitch_scale(dst, stride, ow, oh, filt, sw, sh, W, H, ov, tiles, n)

    def sixteen(dst=d16.ptr, ow=300, oh=210, filt=0, sw=100, sh=70, ov=4, tiles=ptrs, n=9):
        return lib.ju_debug_tile_stitch_scale_state(dst, ow, oh, filt, sw, sh, W, H, ov, tiles, n)

    for call in (eight, sixteen):
        for kw, word in [(dict(dst=None), "null"), (dict(tiles=None), "null"), (dict(tiles=odd), "tile 5"),
                         (dict(n=4), "9 tiles"), (dict(n=10), "9 tiles"), (dict(ov=8), "overlap"), (dict(ov=-1), "overlap"),
                         (dict(sw=47), "source size"), (dict(sh=241), "source size"),
                         (dict(ow=24), "output size 24x210"), (dict(oh=16 * 280 + 1), "output size 300x4481"),
                         (dict(ow=1), "output size 1x210"), (dict(filt=1), "unknown filter 1"), (dict(filt=4), "unknown filter 4"),
                         (dict(ow=49, filt=2), "at least an 8th")]:
            assert call(**kw) == JU_ERR_INVALID_ARGUMENT, (call.__name__, kw)
            assert word in lib.ju_last_error().decode(), (word, lib.ju_last_error())
        assert call(ow=24) == JU_ERR_INVALID_ARGUMENT and \
            "the blended frame 400x280, four times the tiled source size" in lib.ju_last_error().decode()
    assert eight(stride=1196) == JU_ERR_INVALID_ARGUMENT and "smaller than a row" in lib.ju_last_error().decode()
    assert sixteen(dst=d16.ptr + 4) == JU_ERR_INVALID_ARGUMENT and "8-byte aligned" in lib.ju_last_error().decode()
    d8.check(blank8)
    d16.check(blank16)


# ---- 4. end to end against twins --------------------------------------------------------------------------------------------
CASES = [(100, 70, 4, 9, 300, 210, F.TRIANGLE), (49, 31, 7, 4, 392, 248, F.CATMULL_ROM)]


def wanted(fmt, rec8, rec16, t, sw, sh, ov, oh, ow, filt, deep):
    b16 = D.stitch16(rec16[t], sw, sh, W, H, ov) if deep else None
    return TO.planes_of_blended(fmt, CS, rec8[t], b16, oh, ow, filt, deep)


@pytest.mark.parametrize("deep_from_state", [0, 1])
@pytest.mark.parametrize("sw,sh,ov,tiles,ow,oh,filt", CASES)
@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_frames_equal_the_twins_blended_scaled_and_encoded(dtype, sw, sh, ov, tiles, ow, oh, filt, deep_from_state):
    """Four frames, a reset, three more; the formats and the frame's place rotate.  rec8: the twins' outputs blended by
    T.stitch (test_gpu_tiled.twins); rec16: the 16-bit samples of every twin's state (test_gpu_tiled_deep.twins16)."""
    blob, clip = small_blob(), clip_of(sw, sh)
    rec8 = twins(blob, dtype, clip, W, H, ov, ("100x70" if (sw, sh, ov) == (100, 70, 4) else (sw, sh, ov), dtype))
    rec16 = twins16(blob, dtype, clip, ov, (sw, sh, ov, dtype))
    with R.TiledRuntime(blob, 0, dtype, sw, sh, ov) as tr:
        assert tr.get_output_size() == (0, 0) and tr.stat("output_scaled") == 0 and tr.stat("output_filter") == 0
        assert tr.frame_output_size() == (4 * sw, 4 * sh)
        tr.set_output_size(ow, oh, filt)
        tr.set_deep_from_state(deep_from_state)
        assert tr.get_output_size() == tr.frame_output_size() == (ow, oh)
        assert tr.stat("output_scaled") == 1 and tr.stat("output_filter") == filt and tr.stat("hbd_from_state") == 1
        assert (tr.out_width, tr.out_height) == (4 * sw, 4 * sh) == (tr.info()["out_width"], tr.info()["out_height"])
        frames = deep_frames = 0
        for order in ((0, 1, 2, 3), (0, 1, 2)):                       # (the second run: behind a reset)
            for t in order:
                fmt = FORMATS[(frames + frames // 6) % 6]
                location = ("host", "device")[(frames + frames // 4) % 2]
                deep = bool(deep_from_state) and fmt in O.DEEP
                got = frame(tr, clip[t], fmt, location, flip=location == "host" and frames == 2)
                want = wanted(fmt, rec8, rec16, t, sw, sh, ov, oh, ow, filt, deep)
                assert same_planes(got, want), (NAMES[fmt], t, location, deep)
                frames += 1
                deep_frames += deep
            tr.reset()
            assert tr.get_output_size() == (ow, oh) and tr.stat("output_filter") == filt      # (reset keeps the setting)
        assert frames == 7 and tr.stat("frames") == 7 and tr.stat("output_scaled_frames") == 7
        assert tr.stat("deep_state_frames") == deep_frames and (deep_frames > 0) == bool(deep_from_state)
        if tiles == 9:
            assert tr.stat("group_frames") == 9 * 7


# ---- 5. one tile against a plain runtime under ju_set_output_size -----------------------------------------------------------
@pytest.mark.parametrize("filt", F.FILTERS, ids=lambda f: F.NAMES[f])
def test_one_tile_is_a_plain_runtime_under_ju_set_output_size(filt):
    blob = small_blob()
    clip = M.synthetic_frames(6, H, W, seed=7, kind="smooth")
    ow, oh = 150, 94
    with R.Runtime(blob, 0, R.DTYPE_F16) as rt, R.TiledRuntime(blob, 0, R.DTYPE_F16, W, H, 7) as tr:
        rt.set_output_size(ow, oh, filt)
        tr.set_output_size(ow, oh, filt)
        tr.set_deep_from_state(1)
        assert tr.stat("tiles") == 1
        for t, image in enumerate(clip):
            fmt = FORMATS[t]
            want = blank(fmt, oh, ow)
            rt.process_frame(R.host_frame(BGRX, [image]), R.host_frame(fmt, want, CS))
            assert same_planes(frame(tr, image, fmt, ("device", "host")[t % 2]), want), (NAMES[fmt], t)
        assert tr.stat("output_scaled_frames") == 6 and tr.stat("deep_state_frames") == 4


# ---- 6. off and on again ------------------------------------------------------------------------------------------------------
def test_turning_it_off_restores_the_former_bytes_and_another_size_remakes_the_buffers():
    sw, sh, ov = 100, 70, 4
    blob, clip = small_blob(), clip_of(sw, sh)
    rec8 = twins(blob, R.DTYPE_F16, clip, W, H, ov, ("100x70", R.DTYPE_F16))
    rec16 = twins16(blob, R.DTYPE_F16, clip, ov, (sw, sh, ov, R.DTYPE_F16))
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as tr:
        tr.set_deep_from_state(1)
        t = 0
        for fmt, location in ((NV12, "host"), (P010, "host"), (BGRX, "host")):          # (all through the staging buffers)
            tr.set_output_size(300, 210, F.TRIANGLE)
            got = frame(tr, clip[t], fmt, location)
            assert same_planes(got, wanted(fmt, rec8, rec16, t, sw, sh, ov, 210, 300, F.TRIANGLE, fmt == P010)), (NAMES[fmt], "on")
            tr.set_output_size(0, 0)
            assert tr.get_output_size() == (0, 0) and tr.stat("output_scaled") == 0 and tr.stat("output_filter") == 0
            tr.reset()
            got = frame(tr, clip[t], fmt, location)                                      # (off: the bytes of before)
            if fmt == P010:
                assert same_planes(got, D.planes(fmt, CS, rec16[t], sw, sh, W, H, ov)), "off"
            else:
                assert same_planes(got, [rec8[t]] if fmt == BGRX else O.encode8(fmt, CS, rec8[t])), (NAMES[fmt], "off")
            tr.set_output_size(640, 440, F.MITCHELL)                                     # (larger than before: remade buffers)
            tr.reset()
            got = frame(tr, clip[t], fmt, location)
            assert same_planes(got, wanted(fmt, rec8, rec16, t, sw, sh, ov, 440, 640, F.MITCHELL, fmt == P010)), (NAMES[fmt], "again")
            tr.reset()
        assert tr.stat("frames") == 9 and tr.stat("output_scaled_frames") == 6 and tr.stat("deep_state_frames") == 3


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_setting_state_and_frame_count_alone():
    sw, sh, ov = 100, 70, 4
    blob, clip = small_blob(), clip_of(sw, sh)
    rec8 = twins(blob, R.DTYPE_F16, clip, W, H, ov, ("100x70", R.DTYPE_F16))
    lib = R.load_library()
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as tr:
        tr.set_output_size(300, 210, F.CATMULL_ROM)
        assert np.array_equal(frame(tr, clip[0], BGRX, "device")[0], F.scale8(rec8[0], 210, 300, F.CATMULL_ROM))
        # the setter: the Python twin refuses with the C layer's words; the C layer itself refuses the same
        for size, filt, word in [((49, 210), 2, "at least an 8th"), ((300, 16 * 280 + 1), 0, "within a factor of 16"),
                                 ((300, 210), 1, "unknown filter 1"), ((1, 1), 0, "2 .. 16384"), ((0, 0), 5, "unknown filter 5")]:
            with pytest.raises(ValueError) as err:
                tr.set_output_size(*size, filt)
            assert lib.ju_tiled_set_output_size(tr._h, size[0], size[1], filt) == JU_ERR_INVALID_ARGUMENT
            text = lib.ju_last_error().decode()
            assert word in text and text.endswith(str(err.value)), (text, str(err.value))
            if "filter" not in word:
                assert "the blended frame 400x280, four times the tiled source size" in text
            assert tr.get_output_size() == (300, 210) and tr.stat("output_filter") == 2
        assert lib.ju_tiled_set_output_size(None, 300, 210, 0) == JU_ERR_INVALID_ARGUMENT
        # a frame at the blended size, an odd output size with NV12, an unknown stat
        out = np.zeros((280, 400, 4), np.uint8)
        with pytest.raises(R.JoshUpscaleError, match="300x210 \\(the output size set\\)"):
            tr.run(clip[1], out)
        assert not out.any()
        tr.set_output_size(301, 211, F.CATMULL_ROM)                    # (an odd size: BGRX and 4:4:4 frames only)
        torch, dev = torch_dev()
        mem = torch.zeros((2 * 212 * 304,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(R.JoshUpscaleError, match="NV12 needs an even width and height"):
            tr.process_frame(R.host_frame(BGRX, [clip[1]]), R.device_frame(NV12, 301, 211, [mem, mem], [304, 304], CS))
        with pytest.raises(R.JoshUpscaleError, match="301x211 \\(the output size set\\)"):
            tr.process_frame(R.host_frame(BGRX, [clip[1]]), R.device_frame(NV12, 302, 212, [mem, mem], [304, 304], CS))
        assert not mem.cpu().numpy().any()
        with pytest.raises(R.JoshUpscaleError, match="unknown stat"):
            tr.stat("output_size")
        tr.set_output_size(300, 210, F.CATMULL_ROM)
        assert tr.stat("frames") == 1 and tr.stat("output_scaled_frames") == 1
        # every tile's state as it was: the second frame is the twins' second
        assert np.array_equal(tr.run(clip[1]), F.scale8(rec8[1], 210, 300, F.CATMULL_ROM))
        assert tr.run(clip[2]).shape == (210, 300, 4)                  # (run allocates at frame_output_size)


# ---- 8. a scene cut -----------------------------------------------------------------------------------------------------------
def test_scene_reset_across_a_cut_equals_an_object_reset_by_hand():
    from test_gpu_tiled_scene import OV, SH, SW, THR, known
    clip, recs = known()
    blob = small_blob()
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as a, R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as b:
        a.set_scene_detect(R.SCENE_RESET, THR)
        for tr in (a, b):
            tr.set_output_size(300, 210, F.MITCHELL)
            tr.set_deep_from_state(1)
        for t, image in enumerate(clip[:6]):                           # across the cut at frame 4
            if recs[t]["cut"]:
                b.reset()
            fmt = (BGRX, BGRX64)[t % 2]
            assert same_planes(frame(a, image, fmt, "device"), frame(b, image, fmt, "device")), t
        assert [r["cut"] for r in a.scene_info()] == [r["cut"] for r in recs[:6]] and a.stat("scene_cuts") == 1
        assert a.stat("output_scaled_frames") == 6 and a.stat("deep_state_frames") == 3
