"""The scene detector of a tiled stream on the GPU (csrc/tile_kernels.hip tile_split_scene_kernel, csrc/scene_kernels.hip
scene_clear_tiles_kernel, tiled.cpp; docs/tiled.md "Scene cuts") -- needs an MI355X.

The two kernels alone through their hooks against the definitions (tests/tiled_reference.py split, tests/scene_reference.py
through tests/tiled_scene_reference.py), bit for bit; JU_SCENE_RESET against TWINS -- one plain runtime per tile, fed the
reference's split, ju_reset on all of them before exactly the frames the definition flags, stitched by the reference --
and against a second tiled object reset by hand, byte for byte; JU_SCENE_REPORT against an object with the detector off;
host and NV12 frames; the one-tile case against a plain runtime under ju_set_scene_detect; deep outputs; the lifecycle."""

import ctypes as C

import numpy as np
import pytest

import tiled_reference as T
import tiled_scene_reference as TS
import yuv_reference as Y
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_scene import STATE_BYTES, Guarded, state_words
from test_gpu_tiled import LAYOUTS, device_run, small_blob, tile_buffers
from test_gpu_tiled_deep import run as deep_run
from test_gpu_yuv import DevPlane, torch_dev

pytestmark = pytest.mark.gpu

JU_ERR_INVALID_ARGUMENT = 1
W, H = 48, 30                                    # helpers.small_config()
SW, SH, OV, THR = 100, 70, 4, 18500              # the known clip at 100 x 70: cuts at 4, 7, 10, 12 (test_tiled_scene_cpu.py)
CUTS = [4, 7, 10, 12]
# (source width, source height, overlap): one tile; a width that is no multiple of four, origins 0 and 1; two tiles;
# 3 x 3 tiles; three tiles over one pixel on both axes
GEOMETRIES = [(48, 30, 7), (49, 31, 0), (80, 30, 4), (100, 70, 4), (90, 54, 7)]


# ---- 1. tile_split_scene_kernel alone ---------------------------------------------------------------------------------------
def split_scene(d_src, sw, sh, ov, ptrs, n, d_prev, state, has_prev, thr, reset_mode, w=W, h=H):
    lib = R.load_library(True)
    rec = R.JuSceneInfo()
    rc = lib.ju_debug_tile_split_scene(d_src.ptr, d_src.stride, sw, sh, w, h, ov, ptrs, n, d_prev.ptr, state.data_ptr(),
                                       C.byref(rec), has_prev, thr, reset_mode)
    assert rc == 0, lib.ju_last_error()
    return {"step": rec.step, "sad": rec.sad, "score": rec.score, "cut": int(rec.cut)}


def fresh_state(s_before=0):
    torch, dev = torch_dev()
    words = np.zeros(STATE_BYTES // 8, np.uint64)
    words[2] = s_before                                           # the S the step compares with
    return torch.from_numpy(words.view(np.uint8).copy()).to(dev)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_fused_kernel_equals_the_definitions(layout):
    for sw, sh, ov in GEOMETRIES:
        rng = np.random.default_rng(sw * 100 + sh + ov)
        src = rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8)            # (X random: ignored, written as 0)
        old = rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8)
        d_src = DevPlane(src, **LAYOUTS[layout])
        want_tiles = T.split(src, W, H, ov)
        s_full = TS.S.sad(src, old)
        assert TS.owned_sad(src, old, W, H, ov) == s_full
        n = 3 * sw * sh
        # (has_prev, S before, threshold, reset mode): no predecessor; one; two: no cut at the largest threshold, a cut in
        # report mode, D = 0, a cut that raises the flag
        for has_prev, s_before, thr, reset_mode in [(0, 0, 1, 1), (1, 0, 1, 1), (3, 0, 255000, 1), (3, 0, 1, 0),
                                                    (3, s_full, 1, 1), (3, s_full // 2, 40000, 1)]:
            case = (sw, sh, ov, has_prev, s_before, thr, reset_mode)
            buf, ptrs, _ = tile_buffers([np.full((H, W, 4), 0x5A, np.uint8)] * len(want_tiles))
            d_prev = DevPlane(old)                                 # (the kept frame: dense, with guards around it)
            state = fresh_state(s_before)
            rec = split_scene(d_src, sw, sh, ov, ptrs, len(want_tiles), d_prev, state, has_prev, thr, reset_mode)
            got = buf.cpu().numpy()
            for k, tile in enumerate(want_tiles):
                assert np.array_equal(got[k, :tile.size].reshape(tile.shape), tile), (case, k)
                assert (got[k, tile.size:] == 0xA5).all(), (case, k)   # (nothing behind a tile)
            d_src.check(src)                                       # the source and its guard bytes untouched
            d_prev.check(TS.masked(src))                           # the kept frame is the masked source, nothing around it
            seen = {0: 0, 1: 1, 3: 2}[has_prev]
            want_s = s_full if seen >= 1 else 0
            want_d, want_cut = TS.S.decide(want_s, s_before, seen, n, thr)
            assert rec == {"step": 0, "sad": want_s, "score": want_d, "cut": want_cut}, case
            q, w = state_words(state)
            assert q[0] == 0 and w[2] == 0, case                   # accumulator and ticket re-armed
            assert w[3] == (1 if want_cut and reset_mode else 0), case
            assert q[2] == want_s and q[3] == 1 and q[4] == want_cut, case
        # the cases above met both decisions
        assert TS.S.decide(s_full, 0, 2, n, 255000)[1] == 0 and TS.S.decide(s_full, 0, 2, n, 1)[1] == 1
        assert TS.S.decide(s_full, s_full // 2, 2, n, 40000)[1] == 1


def test_fused_kernel_sums_in_64_bits():
    """3840 x 2160 white against a black kept frame, 480 x 270 tiles: S = 3 3840 2160 255 > 2^32, exact.  At overlap 16 that
    source has 9 x 9 = 81 tiles, more than the 64 a frame may have, and the hook refuses it as ju_debug_tile_split does
    (asserted below); the same source and the same sum run at overlap 0, its only admitted layout: 8 x 8 tiles."""
    torch, dev = torch_dev()
    lib = R.load_library(True)
    sw, sh = 3840, 2160
    assert "tiles are more than 64" in T.problem(sw, sh, 480, 270, 16) and T.problem(sw, sh, 480, 270, 0) == ""
    white = np.full((sh, sw, 4), 255, np.uint8)
    d_src = DevPlane(white)
    prev = torch.zeros((sh, sw, 4), dtype=torch.uint8, device=dev)
    tiles = torch.zeros((64, 270 * 480 * 4), dtype=torch.uint8, device=dev)
    ptrs = (C.c_void_p * 64)(*[tiles.data_ptr() + k * tiles.shape[1] for k in range(64)])
    state = fresh_state()
    rec = R.JuSceneInfo()
    torch.cuda.synchronize()
    args = [d_src.ptr, d_src.stride, sw, sh, 480, 270, 16, ptrs, 64, prev.data_ptr(), state.data_ptr(), C.byref(rec), 3,
            TS.S.THRESHOLD_MAX, 0]
    assert lib.ju_debug_tile_split_scene(*args) == JU_ERR_INVALID_ARGUMENT and "9x9 tiles" in lib.ju_last_error().decode()
    args[6] = 0
    assert lib.ju_debug_tile_split_scene(*args) == 0, lib.ju_last_error()
    want = 3 * sw * sh * 255
    assert want > 2 ** 32
    assert (rec.step, rec.sad, rec.score, rec.cut) == (0, want, want, 1)
    q, w = state_words(state)
    assert q[0] == 0 and w[2] == 0 and w[3] == 0 and q[2] == want   # (a cut in report mode: no reset flag)
    masked = torch.tensor([255, 255, 255, 0], dtype=torch.uint8, device=dev)
    assert bool((prev == masked).all()) and bool((tiles.view(64, 270, 480, 4) == masked).all())


def test_fused_kernel_hook_refuses_before_a_launch():
    lib = R.load_library(True)
    torch, dev = torch_dev()
    buf, ptrs, slot = tile_buffers([np.zeros((H, W, 4), np.uint8)] * 9)
    d = DevPlane(np.zeros((70, 100, 4), np.uint8))
    prev = DevPlane(np.full((70, 100, 4), 7, np.uint8))
    state = fresh_state()
    rec = R.JuSceneInfo()

    base = dict(src=d.ptr, stride=d.stride, sw=100, ov=4, tiles=ptrs, count=9, p=prev.ptr, st=state.data_ptr(), r=C.byref(rec),
                has_prev=3, thr=THR)

    def call(**kw):
        a = {**base, **kw}
        return lib.ju_debug_tile_split_scene(a["src"], a["stride"], a["sw"], 70, W, H, a["ov"], a["tiles"], a["count"], a["p"],
                                             a["st"], a["r"], a["has_prev"], a["thr"], 1)
    odd = (C.c_void_p * 9)(*[buf.data_ptr() + k * slot + (8 if k == 5 else 0) for k in range(9)])
    for kw, word in [(dict(ov=8), "overlap"), (dict(count=4), "9 tiles"), (dict(src=d.ptr + 2), "multiples of 4"),
                     (dict(stride=396), "smaller than a row"), (dict(sw=47), "source size"), (dict(src=None), "null"),
                     (dict(p=None), "null"), (dict(st=None), "null"), (dict(r=None), "null"), (dict(p=prev.ptr + 2), "aligned"),
                     (dict(st=state.data_ptr() + 4), "aligned"), (dict(has_prev=2), "has_prev"),
                     (dict(thr=0), "threshold_milli"), (dict(thr=255001), "threshold_milli"), (dict(tiles=odd), "tile 5")]:
        assert call(**kw) == JU_ERR_INVALID_ARGUMENT, kw
        assert word in lib.ju_last_error().decode(), (word, lib.ju_last_error())
    prev.check(np.full((70, 100, 4), 7, np.uint8))
    assert not state.cpu().numpy().any() and not buf.cpu().numpy()[:, :H * W * 4].any()


# ---- 2. scene_clear_tiles_kernel alone -----------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, 1])
def test_clear_tiles_kernel_obeys_the_flag_and_the_bounds(flag):
    """Nine tiles under one flag, buffers 0, 4 and 9 bytes off a 64-byte boundary: sizes below one vector, no multiple of
    16, and more than one workgroup's chunk (16384 bytes)."""
    torch, dev = torch_dev()
    lib = R.load_library(True)
    word = torch.tensor([flag], dtype=torch.int32, device=dev)
    sizes = [16, 4080, 100016, 1, 33, 16384, 16400, 7, 50000]
    a = [Guarded(sizes[k], (0, 4, 9)[k % 3], k) for k in range(9)]
    b = [Guarded(sizes[(k + 4) % 9], (9, 0, 4)[k % 3], 20 + k) for k in range(9)]
    torch.cuda.synchronize()
    arr = lambda vals, ty: (ty * 9)(*vals)
    rc = lib.ju_debug_scene_clear_tiles(9, word.data_ptr(), arr([g.ptr for g in a], C.c_void_p), arr([g.size for g in a], C.c_size_t),
                                        arr([g.ptr for g in b], C.c_void_p), arr([g.size for g in b], C.c_size_t))
    assert rc == 0, lib.ju_last_error()
    for g in a + b:
        g.check(bool(flag))                                       # exactly the named bytes, or nothing
    assert int(word.cpu()[0]) == flag
    assert lib.ju_debug_scene_clear_tiles(65, word.data_ptr(), None, None, None, None) == JU_ERR_INVALID_ARGUMENT
    assert lib.ju_debug_scene_clear_tiles(9, None, None, None, None, None) == JU_ERR_INVALID_ARGUMENT


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
_CACHE = {}


def known(sh=SH, sw=SW, thr=THR):
    """(the 13-frame clip at the source size, the definition's records): computed once."""
    if (sh, sw, thr) not in _CACHE:
        clip = TS.known_clip(M.synthetic_frames, sh, sw)
        clip.setflags(write=False)
        _CACHE[(sh, sw, thr)] = (clip, TS.run(clip, thr))
    return _CACHE[(sh, sw, thr)]


def reset_twins(dtype, clip=None, key="known"):
    """The definition's frames: one plain runtime per tile, fed T.split through ju_process, ju_reset on ALL of them before
    the frames the definition flags at THR, stitched by T.stitch.  Computed once per dtype and left unchanged."""
    if (key, dtype) not in _CACHE:
        if clip is None:
            clip = known()[0]
        recs = TS.run(clip, THR)
        rts = [R.Runtime(small_blob(), 0, dtype) for _ in range(len(T.split(clip[0], W, H, OV)))]
        try:
            outs = []
            for t, frame in enumerate(clip):
                if recs[t]["cut"]:
                    for rt in rts:
                        rt.reset()
                outs.append(T.stitch([rt.process_image(tile) for rt, tile in zip(rts, T.split(frame, W, H, OV))], SW, SH, W, H, OV))
                outs[-1].setflags(write=False)
        finally:
            for rt in rts:
                rt.close()
        _CACHE[(key, dtype)] = outs
    return _CACHE[(key, dtype)]


@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_reset_mode_equals_the_twins_reset_at_the_flagged_frames(dtype):
    """Nine tiles: every frame is two group passes back to back (5 + 4 tiles); cuts on even and odd frames."""
    clip, recs = known()
    assert TS.cuts(recs) == CUTS
    want = reset_twins(dtype)
    blob = small_blob()
    with R.TiledRuntime(blob, 0, dtype, SW, SH, OV) as a, R.TiledRuntime(blob, 0, dtype, SW, SH, OV) as b:
        a.set_scene_detect(R.SCENE_RESET, THR)
        assert a.get_scene_detect() == (R.SCENE_RESET, THR) and b.get_scene_detect() == (R.SCENE_OFF, 0)
        assert a.stat("scene_mode") == 2 and a.scene_info() == []
        for t, frame in enumerate(clip):
            got = device_run(a, frame)
            assert np.array_equal(got, want[t]), (t, np.abs(got.astype(int) - want[t].astype(int)).max())
            assert a.scene_info(1) == [recs[t]], t
            if recs[t]["cut"]:                                    # the remedy by hand on the second object
                b.reset()
            assert np.array_equal(device_run(b, frame), want[t]), t
        assert a.scene_info() == recs
        assert a.stat("group_frames") == 9 * 13 and b.stat("group_frames") == 9 * 13
        assert a.stat("scene_cuts") == 4 and a.stat("scene_frames") == 13 and a.stat("frames") == 13
        assert b.stat("scene_cuts") == 0 and b.stat("scene_frames") == 0 and b.stat("scene_mode") == 0 and b.scene_info() == []


def test_report_mode_changes_no_byte():
    clip, recs = known()
    blob = small_blob()
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as a, R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as b:
        a.set_scene_detect(R.SCENE_REPORT, THR)
        differs = False
        for t, frame in enumerate(clip):
            got = device_run(a, frame)
            assert np.array_equal(got, device_run(b, frame)), t
            differs = differs or not np.array_equal(got, reset_twins(R.DTYPE_F16)[t])
        assert differs                                            # (a reset at the cuts would have shown)
        assert a.scene_info() == recs and a.stat("scene_cuts") == 4 and a.stat("scene_mode") == 1


@pytest.mark.parametrize("route", ["host", "host-bottom-up", "nv12"])
def test_other_frame_routes_see_the_same_detector_frame(route):
    """RESET mode, so a detector that saw another frame would also show in the bytes."""
    clip, recs = known()
    blob = small_blob()
    torch, dev = torch_dev()
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as tr:
        tr.set_scene_detect(R.SCENE_RESET, THR)
        if route == "nv12":
            cs = R.CS_BT709_LIMITED
            yuv = [Y.encode(f, cs) for f in clip]
            decoded = np.stack([Y.decode(y, u, v, cs) for y, u, v in yuv])
            want_recs = TS.run(decoded, THR)
            assert sum(r["cut"] for r in want_recs) >= 2
            want = reset_twins(R.DTYPE_F16, decoded, "nv12")
            for t, (y, u, v) in enumerate(yuv):
                uv = Y.to_nv12(u, v)
                out = np.empty((4 * SH, 4 * SW, 4), np.uint8)
                if t % 2 == 0:                                    # host planes
                    tr.process_frame(R.host_frame(R.FMT_NV12, [y, uv], cs), R.host_frame(R.FMT_BGRX, [out]))
                else:                                             # device planes
                    dy, duv = torch.from_numpy(y.copy()).to(dev), torch.from_numpy(uv).to(dev)
                    torch.cuda.synchronize()
                    tr.process_frame(R.device_frame(R.FMT_NV12, SW, SH, [dy, duv], colorspace=cs), R.host_frame(R.FMT_BGRX, [out]))
                assert np.array_equal(out, want[t]), t
            assert tr.scene_info() == want_recs
            return
        want = reset_twins(R.DTYPE_F16)
        for t, frame in enumerate(clip):
            if route == "host":
                got = tr.run(frame)
            else:                                                 # bottom-up in and out, padded rows
                src = np.zeros((SH, 4 * SW + 16), np.uint8)[::-1]
                src[:, :4 * SW] = frame.reshape(SH, 4 * SW)
                src[:, 4 * SW:] = 0xEE                            # (padding the detector must not count)
                dst = np.full((4 * SH, 16 * SW + 16), 0xEE, np.uint8)[::-1]
                tr.process(R.JuImage(src.ctypes.data, R.LOC_CPU, src.strides[0], SW, SH),
                           R.JuImage(dst.ctypes.data, R.LOC_CPU, dst.strides[0], 4 * SW, 4 * SH))
                got = dst[:, :16 * SW].reshape(4 * SH, 4 * SW, 4)
            assert np.array_equal(got, want[t]), t
        assert tr.scene_info() == recs


def test_one_tile_is_a_plain_runtime_under_ju_set_scene_detect():
    clip = TS.known_clip(M.synthetic_frames, H, W)
    thr = TS.S.KNOWN_THRESHOLD
    recs = TS.run(clip, thr)
    assert TS.cuts(recs) == TS.S.KNOWN_CUTS
    blob = small_blob()
    with R.Runtime(blob, 0, R.DTYPE_F16) as rt, R.TiledRuntime(blob, 0, R.DTYPE_F16, W, H, 7) as tr:
        rt.set_scene_detect(R.SCENE_RESET, thr)
        tr.set_scene_detect(R.SCENE_RESET, thr)
        assert tr.stat("tiles") == 1
        for t, frame in enumerate(clip):
            assert np.array_equal(device_run(tr, frame), rt.process_image(frame)), t
            assert tr.scene_info(1) == rt.scene_info(1) == [recs[t]], t
        assert tr.scene_info() == rt.scene_info() == recs
        assert tr.stat("scene_cuts") == rt.stat("scene_cuts") == 4


def test_deep_outputs_across_a_cut_equal_an_object_reset_by_hand():
    clip, recs = known()
    blob = small_blob()
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as a, R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as b:
        a.set_scene_detect(R.SCENE_RESET, THR)
        for tr in (a, b):
            tr.set_deep_from_state(1)
            assert tr.stat("hbd_from_state") == 1
        for t, frame in enumerate(clip[:6]):                       # across the cut at frame 4
            if recs[t]["cut"]:
                b.reset()
            got, want = deep_run(a, frame, R.FMT_BGRX64, "device"), deep_run(b, frame, R.FMT_BGRX64, "device")
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), t
        assert TS.cuts(a.scene_info()) == [4] and a.stat("deep_state_frames") == 6


def test_lifecycle():
    clip, recs = known()
    blob = small_blob()
    lib = R.load_library()
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as tr:
        # the refusals are scene_reference.problem's, and leave the setting alone
        tr.set_scene_detect(R.SCENE_REPORT, 500)
        for mode, thr in [(3, 1000), (-1, 1000), (1, 0), (2, 255001), (1, 2 ** 32 - 1)]:
            assert TS.problem(mode, thr)
            assert lib.ju_tiled_set_scene_detect(tr._h, mode, thr) == JU_ERR_INVALID_ARGUMENT
            assert TS.problem(mode, thr) in lib.ju_last_error().decode(), lib.ju_last_error()
            assert tr.get_scene_detect() == (R.SCENE_REPORT, 500)
        assert TS.problem(0, 0) == "" and lib.ju_tiled_set_scene_detect(None, 1, 1000) == JU_ERR_INVALID_ARGUMENT
        assert lib.ju_tiled_get_scene_info(tr._h, None, 4, None) == JU_ERR_INVALID_ARGUMENT
        tr.set_scene_detect(R.SCENE_OFF, 0)
        assert tr.get_scene_detect() == (R.SCENE_OFF, 0) and tr.scene_info() == []

        det = TS.Detector(THR)
        tr.set_scene_detect(R.SCENE_REPORT, THR)
        want = [det.feed(f) for f in clip[:3]]
        for f in clip[:3]:
            device_run(tr, f)
        assert tr.scene_info() == want
        # the same mode with another threshold is no start: the predecessors stay
        tr.set_scene_detect(R.SCENE_REPORT, 1)
        det.threshold = 1
        device_run(tr, clip[3])
        want.append(det.feed(clip[3]))
        assert tr.scene_info() == want and want[3]["cut"] == 1 and want[3]["step"] == 3
        # ju_tiled_reset is a start, keeps mode and threshold, and `step` continues
        tr.reset()
        det.restart()
        assert tr.get_scene_detect() == (R.SCENE_REPORT, 1)
        for f in clip[4:7]:
            device_run(tr, f)
            want.append(det.feed(f))
        assert tr.scene_info() == want and [r["step"] for r in want[4:]] == [4, 5, 6] and want[4]["sad"] == 0 and want[5]["score"] == 0
        # a refused frame advances nothing
        torch, dev = torch_dev()
        d_in = torch.zeros((SH, SW, 4), dtype=torch.uint8, device=dev)
        d_out = torch.zeros((4 * SH, 4 * SW, 4), dtype=torch.uint8, device=dev)
        bad = R.JuImage(d_in.data_ptr(), R.LOC_DEVICE, SW * 4, SW - 1, SH)
        good_out = R.JuImage(d_out.data_ptr(), R.LOC_DEVICE, SW * 16, 4 * SW, 4 * SH)
        assert lib.ju_tiled_process(tr._h, C.byref(bad), C.byref(good_out)) == JU_ERR_INVALID_ARGUMENT
        assert tr.scene_info() == want and tr.stat("scene_frames") == 7 and tr.stat("frames") == 7
        device_run(tr, clip[7])
        want.append(det.feed(clip[7]))
        assert tr.scene_info(1) == [want[-1]] and want[-1]["step"] == 7
        cuts_so_far = sum(r["cut"] for r in want)
        assert tr.stat("scene_cuts") == cuts_so_far
        # off then on again is a start: step 0, no predecessor, an empty ring; the counters are cumulative
        tr.set_scene_detect(R.SCENE_OFF, 0)
        assert tr.scene_info() == [] and tr.stat("scene_frames") == 8 and tr.stat("scene_mode") == 0
        tr.set_scene_detect(R.SCENE_REPORT, THR)
        det = TS.Detector(THR)
        ring = []
        for k in range(70):                                       # the ring keeps the last 64 of 70 decisions
            f = clip[k % 13]
            device_run(tr, f)
            ring.append(det.feed(f))
        assert ring[0] == {"step": 0, "sad": 0, "score": 0, "cut": 0}
        assert tr.scene_info() == ring[-64:] and tr.scene_info(3) == ring[-3:] and tr.scene_info(0) == []
        assert tr.stat("scene_frames") == 78 and tr.stat("scene_cuts") == cuts_so_far + sum(r["cut"] for r in ring)


def test_a_flow_free_model_takes_reset_as_report():
    cfg = small_config()
    cfg, wts = M.remove_flow(cfg, M.make_seeded_weights(cfg))
    blob = M.serialize(cfg, wts)
    clip, recs = known()
    with R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as a, R.TiledRuntime(blob, 0, R.DTYPE_F16, SW, SH, OV) as b:
        a.set_scene_detect(R.SCENE_RESET, THR)
        for t, frame in enumerate(clip[:6]):
            assert np.array_equal(device_run(a, frame), device_run(b, frame)), t
        assert a.scene_info() == recs[:6] and a.get_scene_detect() == (R.SCENE_RESET, THR) and a.stat("scene_cuts") == 1
