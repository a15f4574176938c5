"""A tiled object's source mask on the GPU (csrc/tile_kernels.hip tile_stitch_mask_kernel / tile_stitch_mask_scale_kernel,
tiled.cpp stitchOut; docs/tiled.md "A mask") -- needs an MI355X.  Byte for byte throughout, no tolerance anywhere.

Each kernel alone against the numpy definition (tests/tiled_mask_reference.py) through its hook, over the geometries of
test_tiled_output_cpu and the masks of test_tiled_mask_cpu; a white mask and no mask against the unmasked hooks; the hooks'
refusals; a ju_tiled under a mask against TWINS (one plain runtime per tile, their outputs stitched, masked, scaled and
encoded in numpy); host, bottom-up and NV12 sources; a one-tile object against a plain runtime under ju_set_source_mask;
no feedback into the tiles; a scene cut; the refused calls; the box's stats."""

import ctypes as C

import numpy as np
import pytest

import output_reference as O
import scale_filter_reference as F
import source_reference as S
import tiled_mask_reference as TM
import yuv_reference as Y
from helpers import M
from joshupscale_amd import runtime as R
from test_gpu_output import blank, same_planes
from test_gpu_tiled import tile_buffers, twins
from test_gpu_tiled_deep import clip_of, small_blob
from test_gpu_tiled_output import CASES, LAYOUTS, blended, frame
from test_gpu_yuv import DevPlane, torch_dev
from test_tiled_mask_cpu import masks_of, source_of
from test_tiled_output_cpu import GEOMETRIES, H, W, sizes

pytestmark = pytest.mark.gpu

JU_ERR_INVALID_ARGUMENT = 1
CS = R.CS_BT709_LIMITED
BGRX, NV12, P010, BGRX64, RGBPH = R.FMT_BGRX, R.FMT_NV12, R.FMT_P010, R.FMT_BGRX64, R.FMT_RGBPH
FORMATS = (BGRX, NV12, P010, BGRX64, RGBPH)
NAMES = {BGRX: "bgrx", **O.NAMES}
# the unscaled destination: address phases 0, 4, 8 and 12 mod 16, and bottom-up (addresses and strides multiples of 4)
PLAIN_LAYOUTS = [lay for lay in LAYOUTS if lay["offset"] % 4 == 0 and lay["pad"] % 4 == 0]
# the source's and the mask's rows: top-down and bottom-up, dense and padded
ROWS = [dict(pad=0, offset=0, flip=False), dict(pad=12, offset=4, flip=True), dict(pad=32, offset=8, flip=False),
        dict(pad=0, offset=12, flip=True)]


def test_the_layouts_cover_the_phases():
    assert sorted(lay["offset"] for lay in PLAIN_LAYOUTS if not lay["flip"]) == [0, 4, 8, 12]
    assert any(lay["flip"] for lay in PLAIN_LAYOUTS) and any(lay["offset"] == 1 for lay in LAYOUTS)


def stitch_mask(lib, d, sw, sh, ov, ptrs, n, d_src, d_mask, mask):
    if mask is None:
        return lib.ju_debug_tile_stitch_mask(d.ptr, d.stride, sw, sh, W, H, ov, ptrs, n, None, 0, None, 0, 0, 0)
    return lib.ju_debug_tile_stitch_mask(d.ptr, d.stride, sw, sh, W, H, ov, ptrs, n, d_src.ptr, d_src.stride, d_mask.ptr,
                                         d_mask.stride, mask.shape[1], mask.shape[0])


def stitch_mask_scale(lib, d, ow, oh, filt, sw, sh, ov, ptrs, n, d_src, d_mask, mask):
    if mask is None:
        return lib.ju_debug_tile_stitch_mask_scale(d.ptr, d.stride, ow, oh, filt, sw, sh, W, H, ov, ptrs, n, None, 0, None, 0, 0, 0)
    return lib.ju_debug_tile_stitch_mask_scale(d.ptr, d.stride, ow, oh, filt, sw, sh, W, H, ov, ptrs, n, d_src.ptr, d_src.stride,
                                               d_mask.ptr, d_mask.stride, mask.shape[1], mask.shape[0])


_MASKED = {}


def masked_of(sw, sh, ov, name):
    """S.blend of the geometry's blended frame, its source and one of its masks: computed once, shared by both kernels' tests."""
    key = (sw, sh, ov, name)
    if key not in _MASKED:
        want = S.blend(blended(sw, sh, ov)[2], source_of(sw, sh), masks_of(sw, sh, ov)[name])
        want.setflags(write=False)
        _MASKED[key] = want
    return _MASKED[key]


# ---- 1. each kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_stitch_mask_kernel_equals_the_numpy_definition(sw, sh, ov):
    lib = R.load_library(True)
    tiles = blended(sw, sh, ov)[0]
    buf, ptrs, _ = tile_buffers(tiles)
    before = buf.cpu().numpy()
    src = source_of(sw, sh)
    for k, (name, mask) in enumerate(masks_of(sw, sh, ov).items()):
        want = masked_of(sw, sh, ov, name)
        if name == "rectangle":
            assert np.array_equal(want, TM.masked(tiles, src, mask, W, H, ov))                     # (the shared blend is the definition's)
        d_src, d_mask = DevPlane(src, **ROWS[k % 4]), DevPlane(mask, **ROWS[(k + k // 4 + 1) % 4])
        lay = PLAIN_LAYOUTS[k % len(PLAIN_LAYOUTS)]
        d = DevPlane(np.full((4 * sh, 4 * sw, 4), 0x5A, np.uint8), **lay)
        assert d.ptr % 16 == lay["offset"] or lay["flip"]
        rc = stitch_mask(lib, d, sw, sh, ov, ptrs, len(tiles), d_src, d_mask, mask)
        assert rc == 0, lib.ju_last_error()
        d.check(want)                                                 # (X = 0; the guard bytes around every row)
        d_src.check(src)
        d_mask.check(mask)
    assert np.array_equal(buf.cpu().numpy(), before)                  # (the tiles untouched)


@pytest.mark.parametrize("sw,sh,ov", GEOMETRIES)
def test_stitch_mask_scale_kernel_equals_the_numpy_definition(sw, sh, ov):
    lib = R.load_library(True)
    tiles = blended(sw, sh, ov)[0]
    buf, ptrs, _ = tile_buffers(tiles)
    src = source_of(sw, sh)
    seen = set()
    for k, (name, mask) in enumerate(masks_of(sw, sh, ov).items()):
        filt = F.FILTERS[k % 3]                                       # sizes x filters rotate, not the full product
        size = list(sizes(sw, sh, filt))[(k + 2 * (k // 3)) % 6]
        ow, oh = sizes(sw, sh, filt)[size]
        seen.add((filt, size))
        want = F.scale8(masked_of(sw, sh, ov, name), oh, ow, filt)    # (= TM.frame8: the mask first, then the scale)
        d_src, d_mask = DevPlane(src, **ROWS[(k + 1) % 4]), DevPlane(mask, **ROWS[(k + k // 4) % 4])
        lay = LAYOUTS[(k + 4) % len(LAYOUTS)]                         # (k = 0: the phase 1 mod 16)
        d = DevPlane(np.full((oh, ow, 4), 0x5A, np.uint8), **lay)
        rc = stitch_mask_scale(lib, d, ow, oh, filt, sw, sh, ov, ptrs, len(tiles), d_src, d_mask, mask)
        assert rc == 0, lib.ju_last_error()
        d.check(want)
    assert len(seen) == 10 and {f for f, _ in seen} == set(F.FILTERS) and {s for _, s in seen} == set(sizes(sw, sh, 0))


def test_the_definition_is_the_blend_the_mask_and_then_the_scale():
    sw, sh, ov = 49, 31, 4
    tiles, src, mask = blended(sw, sh, ov)[0], source_of(sw, sh), masks_of(sw, sh, ov)["rectangle"]
    ow, oh = sizes(sw, sh, F.CATMULL_ROM)["odd"]
    assert np.array_equal(TM.frame8(tiles, src, mask, W, H, ov, oh, ow, F.CATMULL_ROM),
                          F.scale8(masked_of(sw, sh, ov, "rectangle"), oh, ow, F.CATMULL_ROM))


# ---- 2. a white mask, and no mask: the unmasked kernels' bytes -----------------------------------------------------------------
@pytest.mark.parametrize("sw,sh,ov", [GEOMETRIES[0], GEOMETRIES[5], GEOMETRIES[4]])
def test_a_white_mask_and_no_mask_give_the_unmasked_hooks_bytes(sw, sh, ov):
    lib = R.load_library(True)
    tiles = blended(sw, sh, ov)[0]
    buf, ptrs, _ = tile_buffers(tiles)
    src, white = source_of(sw, sh), masks_of(sw, sh, ov)["white"]
    d_src, d_mask = DevPlane(src), DevPlane(white)
    ow, oh = sizes(sw, sh, F.MITCHELL)["odd"]
    for lay in (PLAIN_LAYOUTS[1], PLAIN_LAYOUTS[-1]):
        ref = DevPlane(np.full((4 * sh, 4 * sw, 4), 0x5A, np.uint8), **lay)
        assert lib.ju_debug_tile_stitch(ref.ptr, ref.stride, sw, sh, W, H, ov, ptrs, len(tiles)) == 0, lib.ju_last_error()
        ref8 = DevPlane(np.full((oh, ow, 4), 0x5A, np.uint8), **lay)
        assert lib.ju_debug_tile_stitch_scale(ref8.ptr, ref8.stride, ow, oh, F.MITCHELL, sw, sh, W, H, ov, ptrs, len(tiles)) == 0
        for mask in (white, None):
            d = DevPlane(np.full((4 * sh, 4 * sw, 4), 0x5A, np.uint8), **lay)
            assert stitch_mask(lib, d, sw, sh, ov, ptrs, len(tiles), d_src, d_mask, mask) == 0, lib.ju_last_error()
            assert np.array_equal(d.buf.cpu().numpy(), ref.buf.cpu().numpy())
            d = DevPlane(np.full((oh, ow, 4), 0x5A, np.uint8), **lay)
            assert stitch_mask_scale(lib, d, ow, oh, F.MITCHELL, sw, sh, ov, ptrs, len(tiles), d_src, d_mask, mask) == 0
            assert np.array_equal(d.buf.cpu().numpy(), ref8.buf.cpu().numpy())


# ---- 3. the hooks' refusals -----------------------------------------------------------------------------------------------------
def test_the_hooks_refuse_before_a_launch():
    """(the words: tests/test_tiled_mask_cpu.py, without a device; here: nothing is written)"""
    lib = R.load_library(True)
    buf, ptrs, slot = tile_buffers([np.zeros((4 * H, 4 * W, 4), np.uint8)] * 9)
    src, mask = source_of(100, 70), masks_of(100, 70, 4)["grey-7x5"]
    d_src, d_mask = DevPlane(src), DevPlane(mask)
    blank_plain, blank_scaled = np.full((280, 400, 4), 0x5A, np.uint8), np.full((210, 300, 4), 0x5A, np.uint8)
    d, d8 = DevPlane(blank_plain), DevPlane(blank_scaled)

    def plain(dst=d.ptr, stride=d.stride, n=9, ov=4, s=d_src.ptr, ss=d_src.stride, m=d_mask.ptr, ms=d_mask.stride, mw=7, mh=5):
        return lib.ju_debug_tile_stitch_mask(dst, stride, 100, 70, W, H, ov, ptrs, n, s, ss, m, ms, mw, mh)

    def scaled(dst=d8.ptr, stride=d8.stride, n=9, ov=4, s=d_src.ptr, ss=d_src.stride, m=d_mask.ptr, ms=d_mask.stride, mw=7, mh=5, ow=300):
        return lib.ju_debug_tile_stitch_mask_scale(dst, stride, ow, 210, 0, 100, 70, W, H, ov, ptrs, n, s, ss, m, ms, mw, mh)

    for call in (plain, scaled):
        for kw, word in [(dict(dst=None), "null"), (dict(n=4), "9 tiles"), (dict(ov=8), "overlap"), (dict(s=None), "null source"),
                         (dict(s=d_src.ptr + 2), "multiples of 4"), (dict(ms=30), "multiples of 4"), (dict(ss=396), "smaller than a row"),
                         (dict(ms=24), "smaller than a row"), (dict(mw=0), "1 .. 16384"), (dict(mh=16385), "1 .. 16384")]:
            assert call(**kw) == JU_ERR_INVALID_ARGUMENT, (call.__name__, kw)
            assert word in lib.ju_last_error().decode(), (word, lib.ju_last_error())
    assert plain(dst=d.ptr + 2) == JU_ERR_INVALID_ARGUMENT and "multiples of 4" in lib.ju_last_error().decode()
    assert scaled(ow=24) == JU_ERR_INVALID_ARGUMENT and "the blended frame 400x280" in lib.ju_last_error().decode()
    d.check(blank_plain)
    d8.check(blank_scaled)
    assert plain() == 0 and scaled() == 0, lib.ju_last_error()        # (the same arguments, nothing wrong: they run)


# ---- 4. end to end against twins --------------------------------------------------------------------------------------------
def device_mask(mask, flip=False):
    """A mask in device memory as a JuImage (bottom-up when `flip`), and what keeps it alive."""
    plane = DevPlane(mask, pad=8, offset=4, flip=flip)
    return R.JuImage(plane.ptr, R.LOC_DEVICE, plane.stride, mask.shape[1], mask.shape[0]), plane


E2E_MASKS = ["rectangle", "grey-source", "obs", "corners"]


@pytest.mark.parametrize("deep_from_state", [0, 1])
@pytest.mark.parametrize("scaled", [False, True], ids=["blended-size", "output-size"])
@pytest.mark.parametrize("sw,sh,ov,tiles,ow,oh,filt", CASES)
@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_frames_equal_the_twins_stitched_masked_scaled_and_encoded(dtype, sw, sh, ov, tiles, ow, oh, filt, scaled, deep_from_state):
    """Four frames, a reset, three more; formats, the frame's place and the mask's place rotate.  A deep format is the
    8-bit encode of the masked frame whatever ju_tiled_set_deep_from_state says."""
    blob, clip = small_blob(), clip_of(sw, sh)
    rec8 = twins(blob, dtype, clip, W, H, ov, ("100x70" if (sw, sh, ov) == (100, 70, 4) else (sw, sh, ov), dtype))
    which = (dtype == R.DTYPE_BF16) + 2 * (tiles == 4) + scaled + deep_from_state
    name = E2E_MASKS[which % 4]
    mask = masks_of(sw, sh, ov)[name]
    size = (ow, oh) if scaled else None
    with R.TiledRuntime(blob, 0, dtype, sw, sh, ov) as tr:
        assert tr.stat("source_mask") == 0 and tr.stat("source_mask_frames") == 0
        if scaled:
            tr.set_output_size(ow, oh, filt)
        tr.set_deep_from_state(deep_from_state)                       # (accepted; no effect while a mask is set)
        keep = None
        if which % 3 == 0:
            tr.set_source_mask(mask)                                  # a host array
        elif which % 3 == 1:
            image, keep = device_mask(mask)
            tr.set_source_mask(image)
        else:
            image, keep = device_mask(mask, flip=True)
            tr.set_source_mask(image)
        assert tr.stat("source_mask") == 1 and tr.stat("deep_from_state") == deep_from_state and tr.stat("hbd_from_state") == 1
        B, Bh = 4 * sw, 4 * sh
        assert tuple(int(tr.stat("mask_box_" + k)) for k in ("x0", "y0", "x1", "y1")) == TM.box(mask, B, Bh)
        frames = 0
        for order in ((0, 1, 2, 3), (0, 1, 2)):                       # (the second run: behind a reset)
            for t in order:
                fmt = FORMATS[(frames + frames // 5) % 5]
                location = ("host", "device")[(frames + frames // 4) % 2]
                got = frame(tr, clip[t], fmt, location, flip=location == "host" and frames == 2)
                want = TM.planes_of_blended(fmt, CS, rec8[t], clip[t], mask, size, filt)
                assert same_planes(got, want), (NAMES[fmt], t, location, name)
                frames += 1
            tr.reset()
            assert tr.stat("source_mask") == 1                        # (reset keeps the mask)
        assert frames == 7 and tr.stat("frames") == 7 and tr.stat("source_mask_frames") == 7
        assert tr.stat("deep_state_frames") == 0 and tr.stat("output_scaled_frames") == (7 if scaled else 0)
        if tiles == 9:
            assert tr.stat("group_frames") == 9 * 7
        # the setters that keep the mask; then the mask removed: the unmasked bytes, from the states the masked frames left
        tr.set_scene_detect(R.SCENE_REPORT, 10000)
        tr.set_output_size(0, 0)
        assert tr.stat("source_mask") == 1 and tuple(int(tr.stat("mask_box_" + k)) for k in ("x0", "y0", "x1", "y1")) == TM.box(mask, B, Bh)
        assert np.array_equal(frame(tr, clip[0], BGRX, "device")[0], S.blend(rec8[0], clip[0], mask))
        tr.set_source_mask(None)
        assert tr.stat("source_mask") == 0 and [tr.stat("mask_box_" + k) for k in ("x0", "y0", "x1", "y1")] == [0, 0, 0, 0]
        assert np.array_equal(frame(tr, clip[1], BGRX, "host")[0], rec8[1])
        assert tr.stat("source_mask_frames") == 8 and tr.stat("frames") == 9
    del keep


# ---- 5. host, bottom-up and NV12 sources: the pass-through pixel is the staged / decoded source's --------------------------------
def test_the_pass_through_pixel_is_the_staged_or_decoded_sources():
    """Under a black mask the frame is the source of the call in 4 x 4 blocks, whatever the tiles computed."""
    blob = small_blob()
    sw, sh, ov = 96, 64, 4
    base = M.synthetic_frames(3, sh, sw, seed=9, kind="smooth")
    torch, dev = torch_dev()

    def blocks(src):
        want = np.repeat(np.repeat(src, 4, 0), 4, 1).copy()
        want[..., 3] = 0
        return want

    with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as tr:
        tr.set_source_mask(masks_of(100, 70, 4)["black"])
        assert tuple(int(tr.stat("mask_box_" + k)) for k in ("x0", "y0", "x1", "y1")) == (0, 0, 4 * sw, 4 * sh)
        # a host frame, top-down and bottom-up (the same picture stored upside down, read with a negative stride)
        assert np.array_equal(tr.run(base[0]), blocks(base[0]))
        stored = np.ascontiguousarray(base[1][::-1])
        assert np.array_equal(tr.run(stored[::-1]), blocks(base[1]))
        # a device frame read in place, bottom-up and padded
        plane = DevPlane(base[2], pad=16, offset=0, flip=True)
        d_out = torch.zeros((4 * sh, 4 * sw, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        tr.process(R.JuImage(plane.ptr, R.LOC_DEVICE, plane.stride, sw, sh), R.JuImage(d_out.data_ptr(), R.LOC_DEVICE, 4 * sw * 4, 4 * sw, 4 * sh))
        assert np.array_equal(d_out.cpu().numpy(), blocks(base[2]))
        plane.check(base[2])
        # NV12: the source is the frame as decoded at source size
        y, u, v = Y.encode(base[0], CS)
        uv = Y.to_nv12(u, v)
        decoded = Y.decode(y, u, v, CS)
        out = np.zeros((4 * sh, 4 * sw, 4), np.uint8)
        tr.process_frame(R.host_frame(NV12, [y, uv], CS), R.host_frame(BGRX, [out]))
        assert np.array_equal(out, blocks(decoded)) and not np.array_equal(decoded, base[0])
        # ... and under an output size the scale of exactly that
        tr.set_output_size(3 * sw + 1, 3 * sh - 1, F.CATMULL_ROM)
        dy, duv = torch.from_numpy(y.copy()).to(dev), torch.from_numpy(uv).to(dev)
        torch.cuda.synchronize()
        out = np.zeros((3 * sh - 1, 3 * sw + 1, 4), np.uint8)
        tr.process_frame(R.device_frame(NV12, sw, sh, [dy, duv], colorspace=CS), R.host_frame(BGRX, [out]))
        assert np.array_equal(out, F.scale8(blocks(decoded), 3 * sh - 1, 3 * sw + 1, F.CATMULL_ROM))
        assert tr.stat("source_mask_frames") == 5


# ---- 6. one tile against a plain runtime under ju_set_source_mask ---------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["blended-size", "output-size"])
def test_one_tile_is_a_plain_runtime_under_ju_set_source_mask(scaled):
    blob = small_blob()
    clip = M.synthetic_frames(5, H, W, seed=7, kind="smooth")
    masks = masks_of(48, 30, 7)
    ow, oh = (150, 94) if scaled else (4 * W, 4 * H)
    with R.Runtime(blob, 0, R.DTYPE_F16) as rt, R.TiledRuntime(blob, 0, R.DTYPE_F16, W, H, 7) as tr:
        assert tr.stat("tiles") == 1
        tr.set_deep_from_state(1)
        if scaled:
            rt.set_output_size(ow, oh, F.MITCHELL)
            tr.set_output_size(ow, oh, F.MITCHELL)
        for t, image in enumerate(clip):
            mask = masks[("rectangle", "grey-7x5", "obs", "grey-larger", "corners")[t]]
            rt.set_source_mask(mask)
            tr.set_source_mask(mask)
            fmt = FORMATS[t]
            want = blank(fmt, oh, ow)
            rt.process_frame(R.host_frame(BGRX, [image]), R.host_frame(fmt, want, CS))
            assert same_planes(frame(tr, image, fmt, ("device", "host")[t % 2]), want), (NAMES[fmt], t)
        assert tr.stat("source_mask_frames") == 5 and tr.stat("deep_state_frames") == 0


# ---- 7. no feedback -------------------------------------------------------------------------------------------------------------
def test_a_mask_leaves_no_trace_in_the_tiles():
    """An object that ran two frames under a black mask gives, from the frame the mask is removed at, the bytes of one
    that never had a mask (the twins')."""
    sw, sh, ov = 100, 70, 4
    blob, clip = small_blob(), clip_of(sw, sh)
    rec8 = twins(blob, R.DTYPE_F16, clip, W, H, ov, ("100x70", R.DTYPE_F16))
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as tr:
        tr.set_source_mask(masks_of(sw, sh, ov)["black"])
        for t in (0, 1):
            got = tr.run(clip[t])
            assert np.array_equal(got[..., :3], np.repeat(np.repeat(clip[t], 4, 0), 4, 1)[..., :3])
        tr.set_source_mask(None)
        for t in (2, 3):
            assert np.array_equal(tr.run(clip[t]), rec8[t]), t
        assert tr.stat("source_mask_frames") == 2 and tr.stat("frames") == 4


# ---- 8. a scene cut -----------------------------------------------------------------------------------------------------------
def test_scene_reset_across_a_cut_with_a_mask_equals_an_object_reset_by_hand():
    from test_gpu_tiled_scene import OV, SH, SW, THR, known
    clip, recs = known()
    blob = small_blob()
    mask = masks_of(SW, SH, OV)["grey-source"]
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as a, R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as b:
        a.set_source_mask(mask)
        a.set_scene_detect(R.SCENE_RESET, THR)                        # (keeps the mask)
        b.set_source_mask(mask)
        for t, image in enumerate(clip[:6]):                          # across the cut at frame 4
            if recs[t]["cut"]:
                b.reset()
            if t == 3:
                for tr in (a, b):
                    tr.set_output_size(300, 210, F.MITCHELL)          # (keeps the mask too)
            fmt = (BGRX, BGRX64)[t % 2]
            assert same_planes(frame(a, image, fmt, "device"), frame(b, image, fmt, "device")), t
        assert [r["cut"] for r in a.scene_info()] == [r["cut"] for r in recs[:6]] and a.stat("scene_cuts") == 1
        assert a.stat("source_mask_frames") == 6 and a.stat("source_mask") == 1


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_setting_the_stats_and_the_frame_count_alone():
    sw, sh, ov = 100, 70, 4
    blob, clip = small_blob(), clip_of(sw, sh)
    rec8 = twins(blob, R.DTYPE_F16, clip, W, H, ov, ("100x70", R.DTYPE_F16))
    lib = R.load_library()
    mask = masks_of(sw, sh, ov)["rectangle"]
    box = TM.box(mask, 4 * sw, 4 * sh)
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as tr:
        tr.set_source_mask(mask)
        assert np.array_equal(tr.run(clip[0]), S.blend(rec8[0], clip[0], mask))
        m = np.full((5, 7, 4), 255, np.uint8)
        for image, word in [(R.JuImage(m.ctypes.data, R.LOC_GRAPHICS_RESOURCE, 28, 7, 5), "the mask must be host or device memory"),
                            (R.JuImage(m.ctypes.data, R.LOC_CPU, 28, 0, 5), "the mask must be 1 .. 16384 pixels on each axis"),
                            (R.JuImage(m.ctypes.data, R.LOC_CPU, 28, 7, 16385), "1 .. 16384"),
                            (R.JuImage(None, R.LOC_CPU, 28, 7, 5), "NULL mask image"),
                            (R.JuImage(m.ctypes.data, R.LOC_CPU, 24, 7, 5), "|stride| smaller than a row"),
                            (R.JuImage(m.ctypes.data, R.LOC_CPU, -27, 7, 5), "|stride| smaller than a row")]:
            assert lib.ju_tiled_set_source_mask(tr._h, C.byref(image)) == JU_ERR_INVALID_ARGUMENT, word
            text = lib.ju_last_error().decode()
            assert "ju_tiled_set_source_mask: " in text and word in text, (word, text)
            assert tr.stat("source_mask") == 1
            assert tuple(int(tr.stat("mask_box_" + k)) for k in ("x0", "y0", "x1", "y1")) == box
        with pytest.raises(ValueError, match="BGRX mask"):
            tr.set_source_mask(np.zeros((5, 7, 3), np.uint8))
        # a refused frame: the mask's counter and the tiles' states stay
        out = np.zeros((281, 400, 4), np.uint8)
        with pytest.raises(R.JoshUpscaleError, match="400x280"):
            tr.run(clip[1], out)
        with pytest.raises(R.JoshUpscaleError, match="unknown stat"):
            tr.stat("mask_box")
        assert tr.stat("frames") == 1 and tr.stat("source_mask_frames") == 1
        assert np.array_equal(tr.run(clip[1]), S.blend(rec8[1], clip[1], mask))


# ---- 10. the box's stats ----------------------------------------------------------------------------------------------------------
def test_the_box_stats_equal_the_restatement():
    blob = small_blob()
    for sw, sh, ov in (GEOMETRIES[3], GEOMETRIES[5]):
        B, Bh = 4 * sw, 4 * sh
        with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as tr:
            for k, (name, mask) in enumerate(masks_of(sw, sh, ov).items()):
                keep = None
                if k % 2:
                    image, keep = device_mask(mask, flip=k % 4 == 3)
                    tr.set_source_mask(image)
                else:
                    tr.set_source_mask(mask[::-1][::-1] if k % 4 else np.ascontiguousarray(mask[::-1])[::-1])
                got = tuple(int(tr.stat("mask_box_" + key)) for key in ("x0", "y0", "x1", "y1"))
                assert got == TM.box(mask, B, Bh), (name, got)
                assert tr.stat("source_mask") == 1
                del keep
            # a white mask: set, counted, and the launches of an object without one
            tr.set_source_mask(masks_of(sw, sh, ov)["white"])
            src = source_of(sw, sh)
            with R.TiledRuntime(blob, 0, R.DTYPE_F16, sw, sh, ov) as plain:
                assert np.array_equal(tr.run(src), plain.run(src))
            assert tr.stat("source_mask_frames") == 1 and tr.stat("source_mask") == 1
