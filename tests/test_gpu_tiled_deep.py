"""A tiled frame's deep outputs on the GPU (csrc/tile_kernels.hip tile_stitch_state_kernel, tiled.cpp stitchOutDeep;
docs/tiled.md "Deep outputs") -- needs an MI355X.

The kernel alone against the numpy definition (tests/tiled_deep_reference.py), word for word, through its hook; its
refusals; a ju_tiled with ju_tiled_set_deep_from_state against TWINS -- one plain runtime per tile, fed the reference's
split through ju_process_frame with a BGRX64 output, whose words are the 16-bit samples P of that tile's state, blended
by stitch16 and encoded by output_reference.encode16 -- byte for byte, with no tolerance; the one-tile case; where the
setting must change nothing; the setter's values."""

import ctypes as C

import numpy as np
import pytest

import output_reference as O
import tiled_deep_reference as D
import tiled_reference as T
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_output import blank, byte_rows, out_frame, result, same_planes
from test_gpu_tiled import tile_buffers, twins
from test_gpu_yuv import DevPlane

pytestmark = pytest.mark.gpu

JU_ERR_INVALID_ARGUMENT = 1
CS = R.CS_BT709_LIMITED
W, H = 48, 30                                  # helpers.small_config()
SOURCES = [(48, 30), (49, 31), (80, 30), (48, 50), (100, 70)]
OVERLAPS = [0, 4, 7]
BGRX, NV12, P010, I410, BGRX64, RGBPH = R.FMT_BGRX, R.FMT_NV12, R.FMT_P010, R.FMT_I410, R.FMT_BGRX64, R.FMT_RGBPH
DEEP = (P010, I410, BGRX64, RGBPH)
NAMES = {BGRX: "bgrx", **O.NAMES}


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------
def states_of(sw, sh, ov):
    """Finite f16 states of one geometry: random in -0.6 .. 0.6 (both clamps are reached), the exact values that straddle
    them seeded into every tile, the fourth value of every pixel random."""
    rng = np.random.default_rng(sw * 1000 + sh * 10 + ov)
    n = len(T.origins(sw, W, ov)) * len(T.origins(sh, H, ov))
    half = np.float16(0.5)
    exact = np.array([half, -half, 0.0, -0.0, 0.49998, np.nextafter(half, np.float16(0)), np.nextafter(-half, np.float16(0)),
                      np.nextafter(half, np.float16(1)), np.nextafter(-half, np.float16(-1)), 2.0 ** -24, -2.0 ** -24,
                      1.0, -1.0], np.float16)
    assert np.isfinite(exact).all() and exact[9] > 0 > exact[10] and np.signbit(exact[3])
    tiles = []
    for _ in range(n):
        s = rng.uniform(-0.6, 0.6, (4 * H, 4 * W, 4)).astype(np.float16)
        s[..., 3] = rng.uniform(-4.0, 4.0, (4 * H, 4 * W)).astype(np.float16)       # (ignored)
        where = rng.choice(4 * H * 4 * W * 3, 40 * exact.size, replace=False)       # (B, G, R of random pixels)
        s.reshape(-1, 4)[where // 3, where % 3] = np.tile(exact, 40)
        assert np.isfinite(s).all()
        tiles.append(s)
    return tiles


@pytest.mark.parametrize("sw,sh", SOURCES)
def test_stitch_state_kernel_equals_the_numpy_definition(sw, sh):
    lib = R.load_library(True)
    for ov in OVERLAPS:
        states = states_of(sw, sh, ov)
        p = [D.p_from_state(s) for s in states]
        assert min(int(q.min()) for q in p) == 0 and max(int(q.max()) for q in p) == 65535       # both clamps
        want = D.stitch16(p, sw, sh, W, H, ov)
        if len(states) == 1:
            assert np.array_equal(want[..., :3], p[0])
        buf, ptrs, _ = tile_buffers([s.view(np.uint8) for s in states])
        before = buf.cpu().numpy()
        d_dst = DevPlane(np.full((4 * sh, 4 * sw * 8), 0x5A, np.uint8))
        assert d_dst.ptr % 16 == 0
        rc = lib.ju_debug_tile_stitch_state(d_dst.ptr, sw, sh, W, H, ov, ptrs, len(states))
        assert rc == 0, lib.ju_last_error()
        assert (want[..., 3] == 0).all()
        d_dst.check(byte_rows(want))                                  # (X words 0; the guard bytes around the frame)
        assert np.array_equal(buf.cpu().numpy(), before)              # (the states untouched)


# ---- 2. the hook's refusals ----------------------------------------------------------------------------------------------
def test_the_hook_refuses_before_a_launch():
    lib = R.load_library(True)
    buf, ptrs, slot = tile_buffers([np.zeros((4 * H, 4 * W, 8), np.uint8)] * 9)
    blank16 = np.full((280, 400 * 8), 0x5A, np.uint8)
    d = DevPlane(blank16)
    for args, word in [((None, 100, 70, W, H, 4, ptrs, 9), "null"),
                       ((d.ptr, 100, 70, W, H, 4, None, 9), "null"),
                       ((d.ptr + 8, 100, 70, W, H, 4, ptrs, 9), "16-byte aligned"),
                       ((d.ptr, 100, 70, W, H, 4, ptrs, 4), "9 tiles"),
                       ((d.ptr, 100, 70, W, H, 4, ptrs, 10), "9 tiles"),
                       ((d.ptr, 100, 70, W, H, 8, ptrs, 9), "overlap"),
                       ((d.ptr, 100, 70, W, H, -1, ptrs, 9), "overlap"),
                       ((d.ptr, 47, 70, W, H, 4, ptrs, 9), "source size"),
                       ((d.ptr, 100, 241, W, H, 4, ptrs, 9), "source size")]:
        assert lib.ju_debug_tile_stitch_state(*args) == JU_ERR_INVALID_ARGUMENT, word
        assert word in lib.ju_last_error().decode(), (word, lib.ju_last_error())
    odd = (C.c_void_p * 9)(*[buf.data_ptr() + k * slot + (8 if k == 5 else 0) for k in range(9)])
    assert lib.ju_debug_tile_stitch_state(d.ptr, 100, 70, W, H, 4, odd, 9) == JU_ERR_INVALID_ARGUMENT
    assert "tile 5" in lib.ju_last_error().decode()
    d.check(blank16)


# ---- 3. end to end against twins -----------------------------------------------------------------------------------------
_TWINS16 = {}


def small_blob(**kw):
    cfg = small_config(**kw)
    return M.serialize(cfg, M.make_seeded_weights(cfg))


def twins16(blob, dtype, clip, ov, key):
    """Per frame of `clip` the 16-bit samples of every tile's state: one plain runtime per tile, fed the reference's split
    through ju_process_frame with a BGRX64 output (W16 = P).  Computed once per key and left unchanged."""
    if key not in _TWINS16:
        sh, sw = clip.shape[1:3]
        n = len(T.origins(sw, W, ov)) * len(T.origins(sh, H, ov))
        rts = [R.Runtime(blob, 0, dtype) for _ in range(n)]
        try:
            assert all(rt.stat("hbd_from_state") == 1 for rt in rts)
            record = []
            for frame in clip:
                ps = []
                for rt, t in zip(rts, T.split(frame, W, H, ov)):
                    p = blank(BGRX64, 4 * H, 4 * W)
                    rt.process_frame(R.host_frame(BGRX, [t]), R.host_frame(BGRX64, p))
                    p[0].setflags(write=False)
                    ps.append(p[0])
                record.append(ps)
        finally:
            for rt in rts:
                rt.close()
        _TWINS16[key] = record
    return _TWINS16[key]


def clip_of(sw, sh, n=4):
    return M.synthetic_frames(n, sh, sw, seed=5, kind="smooth")


def run(tr, frame, fmt, location, flip=False):
    """One frame through ju_tiled_process_frame: a host BGRX frame in, `fmt` out on the host or the device."""
    oh, ow = tr.out_height, tr.out_width
    planes = blank(fmt, oh, ow)
    keep = []
    tr.process_frame(R.host_frame(BGRX, [frame]),
                     out_frame(fmt, [p[::-1] for p in planes] if flip else planes, ow, oh, location, keep, CS))
    got = result(planes, location, keep)
    return [p[::-1] for p in got] if flip else got


@pytest.mark.parametrize("sw,sh,ov,tiles", [(100, 70, 4, 9), (49, 31, 7, 4)])
@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16])
def test_deep_frames_equal_the_blend_of_the_twins_states(dtype, sw, sh, ov, tiles):
    """100 x 70 at overlap 4: nine tiles, two group passes per frame.  Four frames read both halves of every tile's state
    ping-pong; the formats and the frame's place rotate, and a reset lies in the middle."""
    blob, clip = small_blob(), clip_of(sw, sh)
    rec = twins16(blob, dtype, clip, ov, (sw, sh, ov, dtype))
    with R.TiledRuntime(blob, 0, dtype, sw, sh, ov) as tr:
        assert tr.stat("tiles") == tiles and tr.stat("deep_from_state") == 0 and tr.stat("hbd_from_state") == 1
        tr.set_deep_from_state(1)
        assert tr.stat("deep_from_state") == 1
        frames = 0
        for order in ((0, 1, 2, 3), (0, 1, 2)):                       # (the second run: behind a reset)
            for t in order:
                fmt = DEEP[(frames + frames // 4) % 4]
                location = ("host", "device")[frames % 2]
                got = run(tr, clip[t], fmt, location, flip=location == "host" and t == 2)
                want = D.planes(fmt, CS, rec[t], sw, sh, W, H, ov)
                assert same_planes(got, want), (NAMES[fmt], t, location)
                frames += 1
            tr.reset()
            assert tr.stat("deep_from_state") == 1                    # (reset keeps the setting)
        assert tr.stat("frames") == 7 and tr.stat("deep_state_frames") == 7
        if tiles == 9:
            assert tr.stat("group_frames") == 9 * 7
    # the low bits are in use: not the 257 u8 of the 8-bit route
    p = D.stitch16(rec[1], sw, sh, W, H, ov)
    assert len(np.unique(p[..., :3] & 0xFF)) > 200


# ---- 4. one tile -----------------------------------------------------------------------------------------------------------
def test_one_tiles_deep_frames_are_ju_process_frames():
    blob = small_blob()
    clip = M.synthetic_frames(4, H, W, seed=7, kind="smooth")
    with R.Runtime(blob, 0, R.DTYPE_F16) as rt, R.TiledRuntime(blob, 0, R.DTYPE_F16, W, H, 7) as tr:
        tr.set_deep_from_state(1)
        assert tr.stat("tiles") == 1
        for t, frame in enumerate(clip):
            fmt = DEEP[t]
            want = blank(fmt, 4 * H, 4 * W)
            rt.process_frame(R.host_frame(BGRX, [frame]), R.host_frame(fmt, want, CS))
            assert same_planes(run(tr, frame, fmt, ("device", "host")[t % 2]), want), (NAMES[fmt], t)
        assert tr.stat("deep_state_frames") == 4


# ---- 5. the setting is inert where it should be ---------------------------------------------------------------------------
def test_off_is_the_8_bit_route_and_on_leaves_8_bit_formats_and_the_states_alone():
    blob, clip = small_blob(), clip_of(100, 70)
    want8 = twins(blob, R.DTYPE_F16, clip, W, H, 4, ("100x70", R.DTYPE_F16))      # (the stitched 8-bit frames)
    rec = twins16(blob, R.DTYPE_F16, clip, 4, (100, 70, 4, R.DTYPE_F16))
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 100, 70, 4) as on, R.TiledRuntime(blob, 0, R.DTYPE_F16, 100, 70, 4) as off:
        on.set_deep_from_state(1)
        off.set_deep_from_state(1)
        off.set_deep_from_state(0)
        for t, fmt in enumerate((P010, NV12, BGRX64, BGRX)):              # deep and 8-bit outputs alternate
            a, b = run(on, clip[t], fmt, "device"), run(off, clip[t], fmt, "device")
            if fmt == BGRX:
                assert np.array_equal(b[0], want8[t]) and np.array_equal(a[0], want8[t]), t
            elif fmt == NV12:
                assert same_planes(b, O.encode8(fmt, CS, want8[t])) and same_planes(a, b), t
            else:
                assert same_planes(b, O.encode8(fmt, CS, want8[t])), (NAMES[fmt], t)      # off: today's bytes
                assert same_planes(a, D.planes(fmt, CS, rec[t], 100, 70, W, H, 4)), (NAMES[fmt], t)
                assert not same_planes(a, b), (NAMES[fmt], t)
        assert off.stat("deep_state_frames") == 0 and on.stat("deep_state_frames") == 2
        assert off.stat("deep_from_state") == 0 and off.stat("frames") == 4


@pytest.mark.parametrize("kw", [dict(normalize_brightness=True), dict(output="pre_warp")], ids=["brightness", "pre_warp"])
def test_models_whose_state_is_not_their_frame_keep_the_8_bit_route(kw):
    blob, clip = small_blob(**kw), clip_of(49, 31, 3)
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 49, 31, 7) as on, R.TiledRuntime(blob, 0, R.DTYPE_F16, 49, 31, 7) as off:
        on.set_deep_from_state(1)                                       # (accepted)
        assert on.stat("deep_from_state") == 1 and on.stat("hbd_from_state") == 0 and off.stat("hbd_from_state") == 0
        for t, fmt in enumerate((P010, BGRX64, RGBPH)):
            a, b = run(on, clip[t], fmt, ("host", "device")[t % 2]), run(off, clip[t], fmt, "host")
            assert same_planes(a, b), (NAMES[fmt], t)
        assert on.stat("deep_state_frames") == 0 and on.stat("frames") == 3


def test_a_flow_free_model_takes_the_16_bit_path():
    cfg = small_config()
    cfg, wts = M.remove_flow(cfg, M.make_seeded_weights(cfg))
    blob = M.serialize(cfg, wts)
    clip = clip_of(49, 31, 3)
    rec = twins16(blob, R.DTYPE_F16, clip, 7, ("flow-free", 49, 31, 7))
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, 49, 31, 7) as tr:
        tr.set_deep_from_state(1)
        assert tr.stat("hbd_from_state") == 1
        for t, fmt in enumerate((P010, BGRX64, I410)):
            got = run(tr, clip[t], fmt, ("device", "host")[t % 2])
            assert same_planes(got, D.planes(fmt, CS, rec[t], 49, 31, W, H, 7)), (NAMES[fmt], t)
        assert tr.stat("deep_state_frames") == 3


# ---- 6. the setter's values ------------------------------------------------------------------------------------------------
def test_the_setter_takes_0_and_1_only():
    lib = R.load_library()
    with R.TiledRuntime(small_blob(), 0, R.DTYPE_F16, 49, 31, 4) as tr:
        for start in (0, 1):
            tr.set_deep_from_state(start)
            for bad in (2, -1):
                assert lib.ju_tiled_set_deep_from_state(tr._h, bad) == JU_ERR_INVALID_ARGUMENT
                assert "neither 0 nor 1" in lib.ju_last_error().decode()
                assert tr.stat("deep_from_state") == start
        assert lib.ju_tiled_set_deep_from_state(None, 1) == JU_ERR_INVALID_ARGUMENT
        assert "NULL" in lib.ju_last_error().decode()
