"""The scene detector inside look-ahead passes (ju_set_scene_lookahead; csrc/scene_kernels.hip scene_pass_kernel, the
cut-aware first flow block, engine_passes.cpp "The scene detector inside a pass"; docs/scene_detect.md "Passes").

The contract is equality with the same frames sent one by one through ju_process / ju_process_frame with the same
detector setting -- the path tests/test_gpu_scene.py holds to ju_reset-equivalence -- in every output byte, the state,
the frame history and every ju_scene_info record; and the records equal the Python definition (tests/scene_reference.py).
All comparisons are byte or integer equality."""

import ctypes as C

import numpy as np
import pytest

import scene_reference as S
from flowfree_common import flow_free
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_scene import H, LAYOUTS, STATE_BYTES, THR, W, device_clip, known, state_words
from test_gpu_yuv import DevPlane, torch_dev
from test_gpu_yuv10 import NV12, P010, blank_planes, decoded, source

pytestmark = pytest.mark.gpu

CS = R.CS_BT709_LIMITED
PASS_BYTES = 136                          # ScenePassState: acc[8] u64, ticket u32, reserved u32, resetAt[8] u32, cutAt[8] i32
LAYOUT_NAMES = ["dense", "padded", "bottom-up", "word-offset"]
LOW = 50                                  # a threshold at which the known clip's small motion cuts too (0.05 of a code value)
_CACHE = {}


# ---- 1. scene_pass_kernel alone --------------------------------------------------------------------------------------------
def debug_pass(frames, hw, prev, state, pass_state, has_prev, first_step, thr=THR, reset_mode=1):
    lib = R.load_library(True)
    n = len(frames)
    ptrs = (C.c_void_p * n)(*[f.ptr for f in frames])
    strides = (C.c_ssize_t * n)(*[f.stride for f in frames])
    recs = (R.JuSceneInfo * n)()
    reset_at, cut_at = (C.c_uint32 * n)(), (C.c_int32 * n)()
    rc = lib.ju_debug_scene_pass(n, ptrs, strides, hw[1], hw[0], prev.ptr, state.data_ptr(), pass_state.data_ptr(), has_prev,
                                 first_step, thr, reset_mode, recs, reset_at, cut_at)
    assert rc == 0, lib.ju_last_error()
    return ([{"step": r.step, "sad": r.sad, "score": r.score, "cut": int(r.cut)} for r in recs], list(reset_at), list(cut_at))


def arrays_of(recs, reset_mode):
    """resetAt[] and cutAt[] as the issue defines them, from the definition's records."""
    reset_at = [int(bool(r["cut"] and reset_mode)) for r in recs]
    cut_at, latest = [], -1
    for i, flag in enumerate(reset_at):
        latest = i if flag else latest
        cut_at.append(latest)
    return reset_at, cut_at


def pass_words(pass_state):
    raw = pass_state.cpu().numpy()
    return raw[:64].view(np.uint64), raw[64:68].view(np.uint32)[0]


def launch_and_check(det, clip, lo, n, prev, state, pass_state, reset_mode, shift):
    """Frames clip[lo : lo + n] as ONE launch, each in another layout, against the definition `det` continues."""
    torch, dev = torch_dev()
    has_prev = 0 if det.seen == 0 else (1 if det.seen == 1 else 3)
    first_step = det.step
    frames = [DevPlane(clip[lo + i], **LAYOUTS[LAYOUT_NAMES[(i + shift) % 4]]) for i in range(n)]
    torch.cuda.synchronize()
    got, reset_at, cut_at = debug_pass(frames, (H, W), prev, state, pass_state, has_prev, first_step, reset_mode=reset_mode)
    want = [det.feed(clip[lo + i]) for i in range(n)]
    assert got == want, (lo, n, has_prev, got, want)
    assert (reset_at, cut_at) == arrays_of(want, reset_mode), (lo, n, has_prev, reset_at, cut_at)
    for i, f in enumerate(frames):
        f.check(clip[lo + i])                                     # the frames and their guard bytes untouched
    prev.check(clip[lo + n - 1])                                  # the kept frame is the last item, X included
    acc, ticket = pass_words(pass_state)
    assert not acc.any() and ticket == 0                          # re-armed
    q, w = state_words(state)
    assert q[0] == 0 and w[2] == 0 and q[2] == want[-1]["sad"]    # (SceneState's own accumulator untouched; S carried on)
    return want


@pytest.mark.parametrize("has_prev", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_pass_kernel_equals_the_definition(n, has_prev):
    torch, dev = torch_dev()
    _, clip, recs = known()
    lo = {0: 0, 1: 1, 3: 3}[has_prev]                             # the launch starts at frame `lo` of the known clip
    det = S.Detector(THR)
    for f in clip[:lo]:
        det.feed(f)
    garbage = np.random.default_rng(n).integers(0, 256, (H, W, 4), dtype=np.uint8)
    prev = DevPlane(clip[lo - 1] if lo else garbage)              # (no predecessor: what the kept frame holds must not count)
    state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=dev)
    q = np.zeros(STATE_BYTES // 8, np.uint64)
    q[2], q[3], q[4] = det.s_before, lo, 0                        # S before, frames, cuts: as lo per-frame steps left them
    state.copy_(torch.from_numpy(q.view(np.uint8)))
    pass_state = torch.zeros(PASS_BYTES, dtype=torch.uint8, device=dev)
    first = launch_and_check(det, clip, lo, n, prev, state, pass_state, 1, n)
    assert first == recs[lo:lo + n]
    # a second launch on the same memory goes on where the first stopped: S before, predecessors, step
    second = launch_and_check(det, clip, lo + n, 2, prev, state, pass_state, 1, n + 1)
    assert second == recs[lo + n:lo + n + 2]
    q, _ = state_words(state)
    assert q[3] == lo + n + 2 and q[4] == sum(r["cut"] for r in first + second)
    if has_prev == 3 and n == 8:                                  # frames 3 .. 10: cuts at 4, 7 and 10
        assert arrays_of(first, 1)[1] == [-1, 1, 1, 1, 4, 4, 4, 7]


def test_pass_kernel_in_report_mode_raises_no_flag():
    torch, dev = torch_dev()
    _, clip, recs = known()
    det = S.Detector(THR)
    prev = DevPlane(clip[0])
    state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=dev)
    pass_state = torch.zeros(PASS_BYTES, dtype=torch.uint8, device=dev)
    want = launch_and_check(det, clip, 0, 8, prev, state, pass_state, 0, 0)
    assert [r["cut"] for r in want] == [0, 0, 0, 0, 1, 0, 0, 1] and state_words(state)[1][3] == 0


def test_pass_kernel_sums_in_64_bits():
    torch, dev = torch_dev()
    hw = (2400, 2400)
    black, white = np.zeros(hw + (4,), np.uint8), np.full(hw + (4,), 255, np.uint8)
    white[..., 3] = 0
    frames, prev = [DevPlane(black), DevPlane(white)], DevPlane(black)
    state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=dev)
    pass_state = torch.zeros(PASS_BYTES, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    got, reset_at, cut_at = debug_pass(frames, hw, prev, state, pass_state, 3, 5, thr=S.THRESHOLD_MAX)
    want = 3 * 2400 * 2400 * 255
    assert want > 2 ** 32
    assert got == [{"step": 5, "sad": 0, "score": 0, "cut": 0}, {"step": 6, "sad": want, "score": want, "cut": 1}]
    assert reset_at == [0, 1] and cut_at == [-1, 1]
    prev.check(white)
    acc, ticket = pass_words(pass_state)
    assert not acc.any() and ticket == 0


# ---- 2. end to end: the twin runs frame by frame -----------------------------------------------------------------------------
def frames_in_passes(count, cap):
    """How many of `count` consecutive eligible frames go in passes of at most `cap`: a trailing single frame does not."""
    return count - (1 if count % cap == 1 else 0)


def bound(rt, d_in, d_out):
    n = d_in.shape[0]
    return ([rt.device_image(d_in[t].data_ptr(), W, H) for t in range(n)],
            [rt.device_image(d_out[t].data_ptr(), 4 * W, 4 * H) for t in range(n)])


def snapshot(rt):
    return rt.read_tensor("state").copy(), rt.read_tensor("flow_in").copy()


def same_as(rt, snap):
    return np.array_equal(rt.read_tensor("state"), snap[0]) and np.array_equal(rt.read_tensor("flow_in"), snap[1])


def twin_runs(dtype, mode):
    """The frame-by-frame detecting twin on the known clip, computed once per dtype and mode: run 0 from a fresh runtime,
    run 1 after ju_reset, run 2 straight on without one.  Per run: the 13 output frames, (state, history) and the records."""
    key = ("twin", dtype, mode)
    if key not in _CACHE:
        blob, clip, _ = known()
        runs = []
        with R.Runtime(blob, 0, dtype) as b:
            b.set_scene_detect(mode, THR)
            d_in, d_out = device_clip(clip, 4 * H, 4 * W)
            ins, outs = bound(b, d_in, d_out)
            for run in range(3):
                if run == 1:
                    b.reset()
                for t in range(13):
                    b.process(ins[t], outs[t])
                runs.append((d_out.cpu().numpy().copy(), snapshot(b), b.scene_info(13)))
            assert b.stat("lookahead_frames") == 0 and b.stat("scene_detector_runs") == 39
        _CACHE[key] = runs
    return _CACHE[key]


def definition_runs():
    """The definition's records of the three runs of twin_runs."""
    if "definition" not in _CACHE:
        _, clip, _ = known()
        det = S.Detector(THR)
        runs = []
        for run in range(3):
            if run == 1:
                det.restart()
            runs.append([det.feed(f) for f in clip])
        _CACHE["definition"] = runs
    return _CACHE["definition"]


@pytest.mark.parametrize("cap", [8, 4, 3, 2])
@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_reset_mode_in_passes_equals_the_frame_by_frame_detector(dtype, cap):
    """Cuts as the first item of a pass (cap 4: frame 4; cap 2: frames 4 and 10), a middle item, the last item (cap 8 and
    cap 4: frame 7) and a trailing single frame (frame 12 under caps 4, 3, 2: the per-frame detector, after passes); history
    slots that are part frames and part zeros (items 5 and 6 under cap 8)."""
    blob, clip, recs = known()
    twin, want = twin_runs(dtype, R.SCENE_RESET), definition_runs()
    assert want[0] == recs and [r["step"] for r in want[1]] == list(range(13, 26))
    in_passes = frames_in_passes(13, cap)
    with R.Runtime(blob, 0, dtype) as a:
        a.set_scene_detect(R.SCENE_RESET, THR)
        a.set_scene_lookahead(1)
        a.set_lookahead(cap)
        assert a.stat("scene_lookahead") == 1 and a.stat("scene_pass_frames") == 0
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        ins, outs = bound(a, d_in, d_out)
        for run in range(3):
            # run 0: every tuple's first sighting (eager); run 1, after ju_reset on the same buffers: captured and replayed
            # with other predecessor bits and another first step; run 2, straight on: replays only
            if run == 1:
                a.reset()
                assert a.stat("scene_lookahead") == 1
            d_out.zero_()
            captures = a.stat("graph_captures")
            a.process_batch(ins, outs)
            got = d_out.cpu().numpy()
            for t in range(13):
                assert np.array_equal(got[t], twin[run][0][t]), (run, t)
            assert same_as(a, twin[run][1]), run
            assert a.scene_info(13) == twin[run][2] == want[run], run
            assert a.stat("lookahead_frames") == a.stat("scene_pass_frames") == (run + 1) * in_passes
            if run == 2:
                assert a.stat("graph_captures") == captures
        assert a.stat("scene_cuts") == sum(r["cut"] for run in want for r in run) and a.stat("scene_frames") == 39
        assert a.stat("scene_detector_runs") == 39 and a.stat("fallbacks") == 0
        assert np.array_equal(d_in.cpu().numpy(), clip)            # (the caller's frames: read in place)
    assert sum(r["cut"] for r in want[0]) == 4 and S.cuts(want[0]) == [4, 7, 10, 12]


def test_report_mode_in_passes_changes_no_byte():
    blob, clip, recs = known()
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as plain:
        a.set_scene_detect(R.SCENE_REPORT, THR)
        a.set_scene_lookahead(1)
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        _, p_out = device_clip(clip, 4 * H, 4 * W)
        ins, outs = bound(a, d_in, d_out)
        p_ins, p_outs = bound(plain, d_in, p_out)
        for run in range(2):
            a.process_batch(ins, outs)
            plain.process_batch(p_ins, p_outs)
            assert np.array_equal(d_out.cpu().numpy(), p_out.cpu().numpy()), run
            assert same_as(a, snapshot(plain)), run
        assert a.scene_info(26) == S.run(list(clip) + list(clip), THR)
        assert a.stat("lookahead_frames") == a.stat("scene_pass_frames") == 26 == plain.stat("lookahead_frames")
        assert plain.stat("scene_pass_frames") == 0


def test_process_frames_with_host_yuv_frames():
    """Host NV12 in, host P010 out: the detector goes behind the pass's decode launch and sees the decoded frames."""
    blob, clip, _ = known()
    planes = [source(f, NV12, CS) for f in clip]
    recs = S.run([decoded(NV12, CS, p) for p in planes], THR)
    assert S.cuts(recs) == [4, 7, 10, 12]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        for rt in (a, b):
            rt.set_scene_detect(R.SCENE_RESET, THR)
        a.set_scene_lookahead(1)
        got = [blank_planes(P010, 4 * H, 4 * W) for _ in range(13)]
        want = [blank_planes(P010, 4 * H, 4 * W) for _ in range(13)]
        a.process_frames([R.host_frame(NV12, planes[t], CS) for t in range(13)],
                         [R.host_frame(R.FMT_P010, got[t], CS) for t in range(13)])
        for t in range(13):
            b.process_frame(R.host_frame(NV12, planes[t], CS), R.host_frame(R.FMT_P010, want[t], CS))
        for t in range(13):
            for g, e in zip(got[t], want[t]):
                assert np.array_equal(g, e), t
        assert same_as(a, snapshot(b))
        assert a.scene_info() == b.scene_info() == recs
        assert a.stat("lookahead_yuv_frames") == a.stat("scene_pass_frames") == a.stat("lookahead_frames") == 13
        assert b.stat("lookahead_frames") == 0


def test_a_pass_that_is_run_again_keeps_its_decisions():
    blob, clip, recs = known()
    twin = twin_runs(R.DTYPE_F16, R.SCENE_RESET)
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        a.set_scene_detect(R.SCENE_RESET, THR)
        a.set_scene_lookahead(1)
        a.set_lookahead(4)
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        ins, outs = bound(a, d_in, d_out)
        assert lib.ju_debug_set(b"pass_rerun", 1) == 0
        try:
            a.process_batch(ins, outs)
        finally:
            lib.ju_debug_set(b"pass_rerun", 0)
        got = d_out.cpu().numpy()
        for t in range(13):
            assert np.array_equal(got[t], twin[0][0][t]), t
        assert same_as(a, twin[0][1]) and a.scene_info() == recs
        # every frame met the detector once -- twelve of them inside a pass -- and ran a second time without it
        assert a.stat("scene_detector_runs") == 13 and a.stat("scene_frames") == 13 and a.stat("scene_cuts") == 4
        assert a.stat("scene_pass_frames") == 12 and a.stat("lookahead_frames") == 0


def test_prepare_batch_captures_and_the_passes_only_replay():
    blob, clip, recs = known()
    twin = twin_runs(R.DTYPE_F16, R.SCENE_RESET)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        a.set_scene_detect(R.SCENE_RESET, THR)
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        ins, outs = bound(a, d_in, d_out)
        assert a.prepare_batch(ins[:8], outs[:8]) == 0             # the setting is off: nothing to capture
        a.set_scene_lookahead(1)
        assert a.prepare_batch(ins[:8], outs[:8]) == 2 and a.prepare_batch(ins[8:], outs[8:]) == 2
        assert a.stat("prepared_captures") == 4 and a.stat("eager_runs") == 0
        a.process_batch(ins, outs)
        assert a.stat("graph_replays") == 2 and a.stat("eager_runs") == 0 and a.stat("graph_captures") == 0
        got = d_out.cpu().numpy()
        for t in range(13):
            assert np.array_equal(got[t], twin[0][0][t]), t
        assert same_as(a, twin[0][1]) and a.scene_info() == recs and a.stat("scene_pass_frames") == 13


def test_no_graph_serves_another_detector_configuration():
    """One tuple of four device buffers, registered, refilled between calls: REPORT, then RESET (a change of the mode: the
    detector starts over), then another threshold under the same mode (its memory stays), then REPORT again."""
    torch, dev = torch_dev()
    blob, clip, _ = known()
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_scene_lookahead(1)
        a.set_lookahead(4)
        d_in, d_out = device_clip(clip[:4], 4 * H, 4 * W)
        _, b_out = device_clip(clip[:4], 4 * H, 4 * W)
        ins, outs = bound(a, d_in, d_out)
        b_ins, b_outs = bound(b, d_in, b_out)
        det = None
        # (mode, threshold, the clip's frames fed four by four, graphs ju_prepare_batch has to capture: a change of the
        # mode dropped those of the tuple, the same mode again kept them)
        steps = [(R.SCENE_REPORT, THR, [0, 4], 2), (R.SCENE_RESET, THR, [0, 4, 8], 2), (R.SCENE_RESET, LOW, [0, 4], 0),
                 (R.SCENE_REPORT, LOW, [8, 4], 2)]
        mode_before = R.SCENE_OFF
        for mode, thr, chunks, fresh in steps:
            for rt in (a, b):
                rt.set_scene_detect(mode, thr)
            if mode != mode_before:
                det = S.Detector(thr)
            det.threshold = thr
            mode_before = mode
            assert a.stat("scene_lookahead") == 1
            assert a.prepare_batch(ins, outs) == fresh
            fed = []
            for lo in chunks:
                d_in.copy_(torch.from_numpy(np.ascontiguousarray(clip[lo:lo + 4])).to(dev))
                torch.cuda.synchronize()
                want = [det.feed(f) for f in clip[lo:lo + 4]]
                fed += want
                captures = a.stat("graph_captures")
                a.process_batch(ins, outs)
                for t in range(4):
                    b.process(b_ins[t], b_outs[t])
                assert np.array_equal(d_out.cpu().numpy(), b_out.cpu().numpy()), (mode, thr, lo)
                assert same_as(a, snapshot(b)), (mode, thr, lo)
                assert a.scene_info(4) == b.scene_info(4) == want, (mode, thr, lo)
                assert a.stat("graph_captures") == captures
            if (mode, thr) == (R.SCENE_RESET, THR):
                assert S.cuts(a.scene_info()) == [4, 7, 10]
            if (mode, thr) == (R.SCENE_RESET, LOW):                # the lower threshold counts: a cut the other one does not see
                assert any(r["cut"] and 1000 * r["score"] < THR * 3 * H * W for r in fed)
        assert a.stat("scene_pass_frames") == a.stat("lookahead_frames") == 36 and b.stat("lookahead_frames") == 0


def test_the_setting_its_refusals_and_its_default():
    blob, clip, recs = known()
    twin = twin_runs(R.DTYPE_F16, R.SCENE_RESET)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        assert a.stat("scene_lookahead") == 0 and a.stat("scene_pass_frames") == 0
        for bad in (2, -1, 7):
            with pytest.raises(R.JoshUpscaleError) as e:
                a.set_scene_lookahead(bad)
            assert e.value.code == 1 and e.value.message == \
                "std::invalid_argument: ju_set_scene_lookahead: on must be 0 or 1, got %d" % bad
        assert a.stat("scene_lookahead") == 0
        a.set_scene_lookahead(1)
        a.set_scene_detect(R.SCENE_RESET, THR)                     # ju_set_scene_detect and ju_reset keep the setting
        a.reset()
        assert a.stat("scene_lookahead") == 1
        a.set_scene_lookahead(0)
        # off: today's behaviour -- no pass is formed, nothing is captured for one
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        ins, outs = bound(a, d_in, d_out)
        assert a.prepare_batch(ins[:4], outs[:4]) == 0
        a.process_batch(ins, outs)
        assert a.stat("lookahead_frames") == 0 and a.stat("scene_pass_frames") == 0 and a.stat("scene_detector_runs") == 13
        got = d_out.cpu().numpy()
        for t in range(13):
            assert np.array_equal(got[t], twin[0][0][t]), t
        assert same_as(a, twin[0][1]) and a.scene_info() == recs
    with R.Runtime(blob, 0, R.DTYPE_F16, hooks=False) as p:       # the product library has the setter and the stat keys
        p.set_scene_lookahead(1)
        assert p.stat("scene_lookahead") == 1 and p.stat("scene_pass_frames") == 0


def test_mode_off_with_the_setting_on_is_a_plain_pass():
    blob, clip, _ = known()
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as plain:
        a.set_scene_lookahead(1)
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        _, p_out = device_clip(clip, 4 * H, 4 * W)
        ins, outs = bound(a, d_in, d_out)
        p_ins, p_outs = bound(plain, d_in, p_out)
        a.process_batch(ins, outs)
        plain.process_batch(p_ins, p_outs)
        assert np.array_equal(d_out.cpu().numpy(), p_out.cpu().numpy()) and same_as(a, snapshot(plain))
        assert a.stat("lookahead_frames") == 13 and a.stat("scene_pass_frames") == 0
        assert a.stat("scene_detector_runs") == 0 and a.stat("scene_frames") == 0 and a.scene_info() == []


def test_a_flow_free_model_in_passes_reports_and_changes_no_byte():
    _, clip, recs = known()
    cfg, wts = flow_free(small_config())
    blob = M.serialize(cfg, wts)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as plain:
        assert not a.recurrent
        a.set_scene_detect(R.SCENE_RESET, THR)
        a.set_scene_lookahead(1)
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        _, p_out = device_clip(clip, 4 * H, 4 * W)
        ins, outs = bound(a, d_in, d_out)
        p_ins, p_outs = bound(plain, d_in, p_out)
        a.process_batch(ins, outs)
        plain.process_batch(p_ins, p_outs)
        assert np.array_equal(d_out.cpu().numpy(), p_out.cpu().numpy())
        assert a.scene_info() == recs and a.stat("scene_cuts") == 4
        assert a.stat("scene_pass_frames") == a.stat("lookahead_frames") == 13
