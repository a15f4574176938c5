"""Tiled upscaling on the GPU (csrc/tile_kernels.hip, tiled.cpp; docs/tiled.md) -- needs an MI355X.

The two kernels alone against the numpy definition (tests/tiled_reference.py), byte for byte, through their hooks; a
ju_tiled against TWINS -- one plain runtime per tile, built from the same bytes, fed the reference's split through
ju_process, their outputs stitched by the reference -- byte for byte, with no tolerance: the group passes that advance the
tiles are byte-equal to ju_process.  Then the one-tile case, reset, host frames, NV12 in and out, a full-size model and
the refused calls."""

import ctypes as C

import numpy as np
import pytest

import tiled_reference as T
import yuv_reference as Y
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_yuv import DevPlane, torch_dev

pytestmark = pytest.mark.gpu

JU_ERR_INVALID_ARGUMENT = 1
W, H = 48, 30                                  # helpers.small_config()
SOURCES = [(48, 30), (49, 31), (80, 30), (48, 50), (100, 70)]      # (width, height); the last: 3 x 3 tiles
OVERLAPS = [0, 4, 7]
# BGRX rows: pad in bytes behind each row, first row `offset` bytes off a 64-byte boundary
LAYOUTS = {"dense": dict(pad=0, offset=0, flip=False), "padded": dict(pad=48, offset=0, flip=False),
           "bottom-up": dict(pad=16, offset=0, flip=True), "off-16": dict(pad=4, offset=4, flip=False),
           "off-16-bottom-up": dict(pad=8, offset=12, flip=True)}


def tile_buffers(tiles):
    """The tiles as one device tensor, each at a 256-byte boundary; (tensor, pointer array, slot bytes)."""
    torch, dev = torch_dev()
    slot = -(-tiles[0].size // 256) * 256
    host = np.full((len(tiles), slot), 0xA5, np.uint8)
    for k, t in enumerate(tiles):
        host[k, :t.size] = t.reshape(-1)
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 256 == 0
    ptrs = (C.c_void_p * len(tiles))(*[buf.data_ptr() + k * slot for k in range(len(tiles))])
    return buf, ptrs, slot


def hook(name, frame, sw, sh, ov, ptrs, n):
    lib = R.load_library(True)
    rc = getattr(lib, name)(frame.ptr, frame.stride, sw, sh, W, H, ov, ptrs, n)
    assert rc == 0, lib.ju_last_error()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_split_kernel_equals_the_numpy_definition(layout):
    rng = np.random.default_rng(11)
    for sw, sh in SOURCES:
        src = rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8)          # (X random: written as 0)
        d_src = DevPlane(src, **LAYOUTS[layout])
        for ov in OVERLAPS:
            want = T.split(src, W, H, ov)
            buf, ptrs, slot = tile_buffers([np.full((H, W, 4), 0x5A, np.uint8)] * len(want))
            hook("ju_debug_tile_split", d_src, sw, sh, ov, ptrs, len(want))
            got = buf.cpu().numpy()
            for k, tile in enumerate(want):
                assert np.array_equal(got[k, :tile.size].reshape(tile.shape), tile), (sw, sh, ov, k)
                assert (got[k, tile.size:] == 0xA5).all(), (sw, sh, ov, k)   # (nothing behind a tile)
            d_src.check(src)                                               # (the source untouched)


_STITCH = {}


def stitch_case(sw, sh, ov):
    """(random tile outputs, numpy result) of one geometry, computed once for all layouts."""
    if (sw, sh, ov) not in _STITCH:
        rng = np.random.default_rng(sw * 1000 + sh * 10 + ov)
        n = len(T.origins(sw, W, ov)) * len(T.origins(sh, H, ov))
        tiles = [rng.integers(0, 256, (4 * H, 4 * W, 4), dtype=np.uint8) for _ in range(n)]   # (X random: written as 0)
        _STITCH[(sw, sh, ov)] = (tiles, T.stitch(tiles, sw, sh, W, H, ov))
    return _STITCH[(sw, sh, ov)]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_stitch_kernel_equals_the_numpy_definition(layout):
    for sw, sh in SOURCES:
        for ov in OVERLAPS:
            tiles, want = stitch_case(sw, sh, ov)
            buf, ptrs, _ = tile_buffers(tiles)
            d_dst = DevPlane(np.full((4 * sh, 4 * sw, 4), 0x5A, np.uint8), **LAYOUTS[layout])
            hook("ju_debug_tile_stitch", d_dst, sw, sh, ov, ptrs, len(tiles))
            d_dst.check(want)                                   # (and the guard bytes around every row)
            if len(tiles) == 1:
                assert np.array_equal(want[..., :3], tiles[0][..., :3])


def test_kernel_hooks_refuse_before_a_launch():
    lib = R.load_library(True)
    buf, ptrs, slot = tile_buffers([np.zeros((4 * H, 4 * W, 4), np.uint8)] * 9)
    d = DevPlane(np.zeros((280, 400, 4), np.uint8))
    for args, word in [((d.ptr, d.stride, 100, 70, W, H, 8, ptrs, 9), "overlap"),
                       ((d.ptr, d.stride, 100, 70, W, H, 4, ptrs, 4), "9 tiles"),
                       ((d.ptr + 2, d.stride, 100, 70, W, H, 4, ptrs, 9), "multiples of 4"),
                       ((d.ptr, 1596, 100, 70, W, H, 4, ptrs, 9), "smaller than a row"),
                       ((None, d.stride, 100, 70, W, H, 4, ptrs, 9), "null"),
                       ((d.ptr, d.stride, 47, 70, W, H, 4, ptrs, 9), "source size")]:
        assert lib.ju_debug_tile_stitch(*args) == JU_ERR_INVALID_ARGUMENT
        assert word in lib.ju_last_error().decode(), (word, lib.ju_last_error())
    odd = (C.c_void_p * 9)(*[buf.data_ptr() + k * slot + (8 if k == 5 else 0) for k in range(9)])
    assert lib.ju_debug_tile_stitch(d.ptr, d.stride, 100, 70, W, H, 4, odd, 9) == JU_ERR_INVALID_ARGUMENT
    assert "tile 5" in lib.ju_last_error().decode()
    d.check(np.zeros((280, 400, 4), np.uint8))


# ---- end to end -------------------------------------------------------------------------------------------------------
_TWINS = {}


def twins(blob, dtype, clip, w, h, ov, key):
    """What the definition gives for `clip`: one plain runtime per tile, fed the reference's split through ju_process,
    their outputs stitched by the reference.  Computed once per key and left unchanged."""
    if key not in _TWINS:
        sh, sw = clip.shape[1:3]
        n = len(T.origins(sw, w, ov)) * len(T.origins(sh, h, ov))
        rts = [R.Runtime(blob, 0, dtype) for _ in range(n)]
        try:
            outs = []
            for frame in clip:
                tiles = T.split(frame, w, h, ov)
                outs.append(T.stitch([rt.process_image(t) for rt, t in zip(rts, tiles)], sw, sh, w, h, ov))
            assert all(rt.stat("group_frames") == 0 for rt in rts)
        finally:
            for rt in rts:
                rt.close()
        for o in outs:
            o.setflags(write=False)
        _TWINS[key] = outs
    return _TWINS[key]


def small_blob():
    cfg = small_config()
    return M.serialize(cfg, M.make_seeded_weights(cfg))


def clip_100x70():
    return M.synthetic_frames(4, 70, 100, seed=5, kind="smooth")


def device_run(tr, frame):
    """One frame through ju_tiled_process on device images; the output as numpy."""
    torch, dev = torch_dev()
    d_in = torch.from_numpy(np.ascontiguousarray(frame)).to(dev)
    d_out = torch.zeros((tr.out_height, tr.out_width, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    tr.process(R.JuImage(d_in.data_ptr(), R.LOC_DEVICE, tr.src_width * 4, tr.src_width, tr.src_height),
               R.JuImage(d_out.data_ptr(), R.LOC_DEVICE, tr.out_width * 4, tr.out_width, tr.out_height))
    return d_out.cpu().numpy()


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16])
def test_tiled_frames_equal_the_stitched_twins(dtype):
    """100 x 70 at overlap 4: 9 tiles, so every frame is two group passes (5 + 4 tiles)."""
    blob, clip = small_blob(), clip_100x70()
    want = twins(blob, dtype, clip, W, H, 4, ("100x70", dtype))
    with R.TiledRuntime(blob, 0, dtype, 100, 70, 4) as tr:
        info = tr.info()
        assert (info["tiles_x"], info["tiles_y"], info["overlap"]) == (3, 3, 4)
        assert (info["src_width"], info["src_height"], info["out_width"], info["out_height"]) == (100, 70, 400, 280)
        assert (info["tile_width"], info["tile_height"]) == (W, H)
        xs, ys = T.origins(100, W, 4), T.origins(70, H, 4)
        assert [tr.tile(k) for k in range(9)] == [(x, y) for y in ys for x in xs]
        for t, frame in enumerate(clip):
            got = device_run(tr, frame)
            assert np.array_equal(got, want[t]), (t, np.abs(got.astype(int) - want[t].astype(int)).max())
        assert tr.stat("tiles") == 9 and tr.stat("frames") == 4
        assert tr.stat("group_frames") == 9 * 4, "the tiles did not run as group passes"


def test_a_source_of_the_models_size_is_ju_process():
    blob = small_blob()
    clip = M.synthetic_frames(4, H, W, seed=7, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_F16) as rt, R.TiledRuntime(blob, 0, R.DTYPE_F16, W, H, 7) as tr:
        assert tr.stat("tiles") == 1 and tr.tile(0) == (0, 0)
        for t, frame in enumerate(clip):
            assert np.array_equal(device_run(tr, frame), rt.process_image(frame)), t
        assert tr.stat("group_frames") == 0                       # one tile: no pass to share


def test_reset_gives_the_bytes_of_a_fresh_object():
    blob, clip = small_blob(), clip_100x70()
    want = twins(blob, R.DTYPE_F16, clip, W, H, 4, ("100x70", R.DTYPE_F16))
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 100, 70, 4) as tr:
        for frame in clip[2:]:
            device_run(tr, frame)
        tr.reset()
        for t in range(2):
            assert np.array_equal(device_run(tr, clip[t]), want[t]), t


@pytest.mark.parametrize("flip", [False, True])
def test_host_frames_give_the_bytes_of_the_device_route(flip):
    blob, clip = small_blob(), clip_100x70()
    want = twins(blob, R.DTYPE_F16, clip, W, H, 4, ("100x70", R.DTYPE_F16))
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 100, 70, 4) as tr:
        for t, frame in enumerate(clip):
            if flip:                                             # bottom-up in and out, padded rows
                src = np.zeros((70, 416), np.uint8)[::-1]
                src[:, :400] = frame.reshape(70, 400)
                dst = np.full((280, 1616), 0xEE, np.uint8)[::-1]
                tr.process(R.JuImage(src.ctypes.data, R.LOC_CPU, src.strides[0], 100, 70),
                           R.JuImage(dst.ctypes.data, R.LOC_CPU, dst.strides[0], 400, 280))
                assert (dst[:, 1600:] == 0xEE).all()
                got = dst[:, :1600].reshape(280, 400, 4)
            else:
                got = tr.run(frame)
            assert np.array_equal(got, want[t]), t


def test_a_device_source_off_the_kernels_alignment_gives_the_aligned_bytes():
    """80 x 30 (two tiles): a device BGRX source 1 byte off the split kernel's 4-byte alignment is not read in place but
    copied, device to device, into the staging frame first -- the bytes of the aligned call."""
    torch, dev = torch_dev()
    clip = M.synthetic_frames(3, 30, 80, seed=9, kind="smooth")
    with R.TiledRuntime(small_blob(), 0, R.DTYPE_F16, 80, 30, 4) as tr:
        assert tr.stat("tiles") == 2
        want = [device_run(tr, frame) for frame in clip]
        tr.reset()
        for t, frame in enumerate(clip):
            raw = torch.full((frame.size + 64,), 0xEE, dtype=torch.uint8, device=dev)
            raw[1:1 + frame.size] = torch.from_numpy(np.ascontiguousarray(frame).reshape(-1)).to(dev)
            d_out = torch.zeros((120, 320, 4), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            assert (raw.data_ptr() + 1) % 4 == 1
            tr.process(R.JuImage(raw.data_ptr() + 1, R.LOC_DEVICE, 320, 80, 30), R.JuImage(d_out.data_ptr(), R.LOC_DEVICE, 1280, 320, 120))
            assert np.array_equal(d_out.cpu().numpy(), want[t]), t


def test_nv12_in_and_out():
    """96 x 64 NV12 (3 x 3 tiles): the reference's decode, the tiled route on the decoded frames, the reference's encode."""
    cs = R.CS_BT709_LIMITED
    blob = small_blob()
    base = M.synthetic_frames(3, 64, 96, seed=9, kind="smooth")
    yuv = [Y.encode(f, cs) for f in base]                        # (any NV12 frames: these are smooth ones)
    decoded = np.stack([Y.decode(y, u, v, cs) for y, u, v in yuv])
    want = twins(blob, R.DTYPE_F16, decoded, W, H, 4, ("96x64-nv12", R.DTYPE_F16))
    torch, dev = torch_dev()
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 96, 64, 4) as tr:
        assert tr.stat("tiles") == 9
        for t, (y, u, v) in enumerate(yuv):
            wy, wu, wv = Y.encode(want[t], cs)
            uv = Y.to_nv12(u, v)
            if t % 2 == 0:                                        # host planes
                oy, ouv = np.empty((256, 384), np.uint8), np.empty((128, 384), np.uint8)
                tr.process_frame(R.host_frame(R.FMT_NV12, [y, uv], cs), R.host_frame(R.FMT_NV12, [oy, ouv], cs))
            else:                                                 # device planes
                dy, duv = torch.from_numpy(y.copy()).to(dev), torch.from_numpy(uv).to(dev)
                doy = torch.zeros((256, 384), dtype=torch.uint8, device=dev)
                douv = torch.zeros((128, 384), dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                tr.process_frame(R.device_frame(R.FMT_NV12, 96, 64, [dy, duv], colorspace=cs),
                                 R.device_frame(R.FMT_NV12, 384, 256, [doy, douv], colorspace=cs))
                oy, ouv = doy.cpu().numpy(), douv.cpu().numpy()
            assert np.array_equal(oy, wy) and np.array_equal(ouv, Y.to_nv12(wu, wv)), t


def test_a_full_size_model():
    """psp-fast fp16, 500 x 280 at overlap 16: 2 x 2 tiles of 480 x 270, two frames, against twins."""
    cfg = M.PRESETS["psp-fast"]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    clip = M.synthetic_frames(2, 280, 500, seed=2, kind="smooth")
    want = twins(blob, R.DTYPE_F16, clip, 480, 270, 16, ("500x280", R.DTYPE_F16))
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 500, 280, 16) as tr:
        assert [tr.tile(k) for k in range(4)] == [(0, 0), (20, 0), (0, 10), (20, 10)]
        for t, frame in enumerate(clip):
            assert np.array_equal(device_run(tr, frame), want[t]), t
        assert tr.stat("group_frames") == 4 * 2


def test_refused_calls_leave_the_state_alone():
    blob, clip = small_blob(), clip_100x70()
    want = twins(blob, R.DTYPE_F16, clip, W, H, 4, ("100x70", R.DTYPE_F16))
    lib = R.load_library()
    torch, dev = torch_dev()

    def refused(rc, word):
        assert rc == JU_ERR_INVALID_ARGUMENT, rc
        message = lib.ju_last_error().decode()
        assert word in message, (word, message)

    # creation: sizes and overlap outside the limits, NULL pointers -- before any runtime is made
    h = C.c_void_p()
    for (sw, sh, ov), word in [((100, 70, 8), "overlap 8"), ((100, 70, -1), "overlap -1"), ((47, 70, 4), "source size 47x70"),
                               ((100, 241, 4), "source size 100x241"), ((384, 240, 7), "10x11 tiles")]:
        refused(lib.ju_tiled_create_from_memory(0, blob, len(blob), R.DTYPE_F16, sw, sh, ov, C.byref(h)), word)
        assert not h.value
    refused(lib.ju_tiled_create_from_memory(0, blob, len(blob), R.DTYPE_F16, 100, 70, 4, None), "NULL")
    refused(lib.ju_tiled_create_from_memory(0, None, 0, R.DTYPE_F16, 100, 70, 4, C.byref(h)), "NULL")
    refused(lib.ju_tiled_create(0, None, 100, 70, 4, C.byref(h)), "NULL")
    refused(lib.ju_tiled_process(None, None, None), "NULL")
    refused(lib.ju_tiled_reset(None), "NULL")

    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 100, 70, 4) as tr:
        assert np.array_equal(device_run(tr, clip[0]), want[0])
        d_in = torch.from_numpy(clip[1]).to(dev)
        d_out = torch.zeros((280 * 400 * 4 + 64,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        good_in = R.JuImage(d_in.data_ptr(), R.LOC_DEVICE, 400, 100, 70)
        good_out = R.JuImage(d_out.data_ptr(), R.LOC_DEVICE, 1600, 400, 280)

        def img(base, **kw):
            i = R.JuImage(base.ptr, base.location, base.stride, base.width, base.height)
            for k, v in kw.items():
                setattr(i, k, v)
            return i
        cases = [(None, good_out, "NULL"), (good_in, None, "NULL"),
                 (img(good_in, ptr=None), good_out, "NULL input image"), (good_in, img(good_out, ptr=None), "NULL output image"),
                 (img(good_in, width=99), good_out, "input image must be exactly 100x70"),
                 (img(good_in, width=48, height=30), good_out, "input image must be exactly 100x70"),
                 (good_in, img(good_out, height=279), "output image must be exactly 400x280"),
                 (good_in, img(good_out, width=192, height=120), "output image must be exactly 400x280"),
                 (img(good_in, stride=396), good_out, "smaller than a row"), (good_in, img(good_out, stride=-1596), "smaller than a row"),
                 (img(good_in, location=R.LOC_GRAPHICS_RESOURCE), good_out, "graphics resources"),
                 (good_in, img(good_out, location=R.LOC_GRAPHICS_RESOURCE), "graphics resources"),
                 (img(good_in, location=7), good_out, "unknown location"),
                 (img(good_out, width=100, height=70, stride=400), good_out, "overlaps the input")]
        for inp, out, word in cases:
            refused(lib.ju_tiled_process(tr._h, C.byref(inp) if inp is not None else None,
                                         C.byref(out) if out is not None else None), word)
        # frames: what ju_process_frame refuses for a frame of that size
        dy = torch.zeros((280 * 400 * 2,), dtype=torch.uint8, device=dev)
        nv12_out = R.device_frame(R.FMT_NV12, 400, 280, [dy.data_ptr(), dy.data_ptr() + 400 * 280], colorspace=0)
        bgrx_in = R.device_frame(R.FMT_BGRX, 100, 70, [d_in.data_ptr()])

        def frame(base, **kw):
            f = R.JuFrame()
            C.memmove(C.byref(f), C.byref(base), C.sizeof(f))
            for k, v in kw.items():
                setattr(f, k, v)
            return f
        nv12_in = R.device_frame(R.FMT_NV12, 100, 70, [dy.data_ptr(), dy.data_ptr() + 7000], colorspace=0)
        null_plane = frame(nv12_out)
        null_plane.planes[1] = None
        narrow = frame(nv12_out)
        narrow.strides[0] = 399
        for inp, out, word in [(bgrx_in, frame(nv12_out, colorspace=9), "colour space"), (bgrx_in, frame(nv12_out, format=99), "unknown format"),
                               (bgrx_in, frame(nv12_out, width=398), "output frame must be exactly 400x280"),
                               (frame(nv12_in, width=98), nv12_out, "input frame must be exactly 100x70"),
                               (bgrx_in, null_plane, "plane 1 is NULL"), (bgrx_in, narrow, "smaller than a row"),
                               (bgrx_in, frame(nv12_out, location=R.LOC_GRAPHICS_RESOURCE), "no graphics resources"),
                               (None, nv12_out, "NULL")]:
            refused(lib.ju_tiled_process_frame(tr._h, C.byref(inp) if inp is not None else None, C.byref(out)), word)
        refused(lib.ju_tiled_get_info(tr._h, None), "NULL")
        refused(lib.ju_tiled_get_tile(tr._h, 9, None, None), "index 9")
        v = C.c_double()
        refused(lib.ju_tiled_get_stat(tr._h, b"nope", C.byref(v)), "unknown stat nope")
        refused(lib.ju_tiled_get_stat(tr._h, None, C.byref(v)), "null")
        assert tr.stat("frames") == 1 and tr.stat("group_frames") == 9
        # the state is untouched: the clip goes on as the twins'
        for t in (1, 2, 3):
            assert np.array_equal(device_run(tr, clip[t]), want[t]), t

    # an odd source size and a 4:2:0 frame
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 49, 31, 4) as tr:
        odd_in = R.device_frame(R.FMT_NV12, 49, 31, [dy.data_ptr(), dy.data_ptr() + 4096], strides=[64, 64], colorspace=0)
        out = R.device_frame(R.FMT_BGRX, 196, 124, [d_out.data_ptr()])
        refused(lib.ju_tiled_process_frame(tr._h, C.byref(odd_in), C.byref(out)), "NV12 needs an even width and height")
        assert tr.stat("frames") == 0
