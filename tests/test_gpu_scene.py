"""The scene detector on the GPU (csrc/scene_kernels.hip, engine_frames.cpp "Scene detector"; docs/scene_detect.md): the two
kernels alone against the Python definition (tests/scene_reference.py), bit for bit; JU_SCENE_RESET against a twin that
is ju_reset by hand before exactly the frames the definition flags, byte for byte in every output, the state and the
frame history; JU_SCENE_REPORT against an untouched twin; every entry point; the lifecycle; a flow-free model; the
re-run of a step."""

import ctypes as C

import numpy as np
import pytest

import scene_reference as S
import source_reference as SRC
from flowfree_common import flow_free
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_source import same_state
from test_gpu_yuv import GUARD, DevPlane, torch_dev
from test_gpu_yuv10 import NV12, P010, blank_planes, decoded, source

pytestmark = pytest.mark.gpu

CS = R.CS_BT709_LIMITED
THR = S.KNOWN_THRESHOLD
H, W = 30, 48
LAYOUTS = {"dense": dict(pad=0, offset=0, flip=False), "padded": dict(pad=128, offset=0, flip=False),
           "bottom-up": dict(pad=64, offset=0, flip=True), "word-offset": dict(pad=4, offset=4, flip=False)}
STATE_BYTES = 40                         # SceneState: acc u64, ticket u32, reset flag u32, S before u64, frames u64, cuts u64

_CACHE = {}


def known():
    """(blob of the small model, the 13-frame clip, the definition's records at THR): computed once."""
    if "known" not in _CACHE:
        cfg = small_config()
        clip = S.known_clip(M.synthetic_frames, H, W)
        _CACHE["known"] = (M.serialize(cfg, M.make_seeded_weights(cfg)), clip, S.run(clip, THR))
    return _CACHE["known"]


def drive_twin(b, recs, t):
    """The manual remedy: ju_reset in front of exactly the frames the definition flags."""
    if recs[t]["cut"]:
        b.reset()


# ---- 1. scene_sad_kernel alone ---------------------------------------------------------------------------------------------
def debug_sad(frame, hw, prev, state, has_prev, thr=THR, reset_mode=0):
    lib = R.load_library(True)
    rec = R.JuSceneInfo()
    rc = lib.ju_debug_scene(0, frame.ptr, frame.stride, hw[1], hw[0], prev.ptr, state.data_ptr(), has_prev, thr, reset_mode,
                            C.byref(rec), None, 0, None, 0)
    assert rc == 0, lib.ju_last_error()
    return {"step": rec.step, "sad": rec.sad, "score": rec.score, "cut": int(rec.cut)}


def state_words(state):
    return state.cpu().numpy().view(np.uint64), state.cpu().numpy().view(np.uint32)


def sad_pair(hw, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, hw + (4,), dtype=np.uint8), rng.integers(0, 256, hw + (4,), dtype=np.uint8))   # (X random)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_sad_kernel_equals_the_definition(layout):
    torch, dev = torch_dev()
    for hw in [(2, 2), (7, 301), (30, 48), (270, 480)]:
        old, cur = sad_pair(hw, hw[0] * 1000 + hw[1])
        want = S.sad(cur, old)
        n = 3 * hw[0] * hw[1]
        d_cur = DevPlane(cur, **LAYOUTS[layout])
        sums = []
        state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=dev)
        for run in range(2):                                      # the same input twice: accumulator and ticket re-armed
            d_prev = DevPlane(old)                                # (the kept frame: dense, with guards around it)
            rec = debug_sad(d_cur, hw, d_prev, state, 3, thr=1, reset_mode=1)
            sums.append(rec["sad"])
            d_prev.check(cur)                                     # the kept frame is c_t byte for byte, X included
            d_cur.check(cur)                                      # the source and its guard bytes untouched
            q, w = state_words(state)
            assert q[0] == 0 and w[2] == 0                        # accumulator, ticket
            assert q[2] == want and q[3] == run + 1               # S for the next step, frames
            # first run: S before is 0, D = S, a cut; second: S before = S, D = 0, none -- the flag follows
            assert rec["score"] == (want if run == 0 else 0) and rec["cut"] == (1 if run == 0 else 0) == w[3], (hw, run, rec)
            assert S.decide(want, 0 if run == 0 else want, 2, n, 1) == (rec["score"], rec["cut"])
        assert sums == [want, want], (hw, sums)


def test_sad_kernel_without_predecessors():
    torch, dev = torch_dev()
    hw = (30, 48)
    old, cur = sad_pair(hw, 5)
    for has_prev, want_sad in ((0, 0), (1, S.sad(cur, old))):
        d_cur, d_prev = DevPlane(cur), DevPlane(old)
        state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=dev)
        rec = debug_sad(d_cur, hw, d_prev, state, has_prev, thr=1, reset_mode=1)
        assert rec == {"step": 0, "sad": want_sad, "score": 0, "cut": 0}
        d_prev.check(cur)
        q, w = state_words(state)
        assert q[2] == want_sad and w[3] == 0 and q[4] == 0


def test_sad_kernel_sums_in_64_bits():
    torch, dev = torch_dev()
    hw = (2400, 2400)
    black, white = np.zeros(hw + (4,), np.uint8), np.full(hw + (4,), 255, np.uint8)
    white[..., 3] = 0
    d_cur, d_prev = DevPlane(white), DevPlane(black)
    state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=dev)
    rec = debug_sad(d_cur, hw, d_prev, state, 3, thr=S.THRESHOLD_MAX)
    want = 3 * 2400 * 2400 * 255
    assert want > 2 ** 32 and rec == {"step": 0, "sad": want, "score": want, "cut": 1}
    assert state_words(state)[1][3] == 0                          # (a cut in report mode: no reset flag)
    d_prev.check(white)


# ---- 2. scene_clear_kernel alone -------------------------------------------------------------------------------------------
class Guarded:
    """`size` pattern bytes inside a device buffer of guard bytes, `offset` bytes past a 64-byte guard."""

    def __init__(self, size, offset, seed):
        torch, dev = torch_dev()
        self.size, self.lead = size, 64 + offset
        self.host = np.full(self.lead + size + 64, GUARD, np.uint8)
        self.body(self.host)[...] = np.random.default_rng(seed).integers(1, 256, size, dtype=np.uint8)   # (never 0)
        self.buf = torch.from_numpy(self.host.copy()).to(dev)

    def body(self, a):
        return a[self.lead:self.lead + self.size]

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lead

    def check(self, cleared):
        exp = self.host.copy()
        if cleared:
            self.body(exp)[...] = 0
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (bad[:8], got[bad[:8]], exp[bad[:8]])


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("offset", [0, 4, 9])
def test_clear_kernel_obeys_the_flag_and_the_bounds(flag, offset):
    torch, dev = torch_dev()
    lib = R.load_library(True)
    word = torch.tensor([flag], dtype=torch.int32, device=dev)
    sizes = [16, 4080, 1000016]
    for k, size in enumerate(sizes):
        a, b = Guarded(size, offset, k), Guarded(sizes[(k + 1) % 3], offset, 7 + k)
        torch.cuda.synchronize()
        rc = lib.ju_debug_scene(1, None, 0, 0, 0, None, word.data_ptr(), 0, 0, 0, None, a.ptr, a.size, b.ptr, b.size)
        assert rc == 0, lib.ju_last_error()
        a.check(bool(flag))
        b.check(bool(flag))
    assert int(word.cpu()[0]) == flag


# ---- 3, 4. the modes end to end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_reset_mode_equals_a_reset_by_hand_at_the_flagged_frames(dtype):
    blob, clip, recs = known()
    assert S.cuts(recs) == [4, 7, 10, 12]                         # even and odd frames: both binding-set parities
    with R.Runtime(blob, 0, dtype) as a, R.Runtime(blob, 0, dtype) as b:
        a.set_scene_detect(R.SCENE_RESET, THR)
        assert a.get_scene_detect() == (R.SCENE_RESET, THR) and b.get_scene_detect() == (R.SCENE_OFF, 0)
        assert a.stat("scene_mode") == 2 and a.scene_info() == []
        for t, f in enumerate(clip):
            drive_twin(b, recs, t)
            assert np.array_equal(a.process_image(f), b.process_image(f)), t
            assert same_state(a, b), t
            assert a.scene_info(1) == [recs[t]], t
        assert a.scene_info() == recs
        assert a.stat("scene_cuts") == 4 and a.stat("scene_frames") == 13 and a.stat("scene_detector_runs") == 13
        assert b.stat("scene_cuts") == 0 and b.stat("scene_frames") == 0 and b.stat("scene_mode") == 0


def test_report_mode_changes_no_byte():
    blob, clip, recs = known()
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_scene_detect(R.SCENE_REPORT, THR)
        for t, f in enumerate(clip):
            assert np.array_equal(a.process_image(f), b.process_image(f)), t
            assert same_state(a, b), t
        assert a.scene_info() == recs and a.stat("scene_cuts") == 4
        # the same mode again: the threshold alone changes, the detector's memory stays
        a.set_scene_detect(R.SCENE_REPORT, 1)
        a.process_image(clip[0])
        b.process_image(clip[0])
        want = S.Detector(1, step=13)
        want.prev, want.s_before, want.seen = clip[12], recs[12]["sad"], 13
        assert a.scene_info(1) == [want.feed(clip[0])] and a.scene_info(1)[0]["step"] == 13
        assert same_state(a, b)


# ---- 5. every entry point ----------------------------------------------------------------------------------------------------
def device_clip(clip, oh, ow):
    torch, dev = torch_dev()
    d_in = torch.from_numpy(np.ascontiguousarray(clip)).to(dev)
    d_out = torch.zeros((len(clip), oh, ow, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return d_in, d_out


def twin_outputs(b, clip, recs):
    outs = []
    for t, f in enumerate(clip):
        drive_twin(b, recs, t)
        outs.append(b.process_image(f).copy())
    return outs


def test_process_on_device_frames_keeps_the_direct_path():
    blob, clip, recs = known()
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_scene_detect(R.SCENE_RESET, THR)
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        ins = [a.device_image(d_in[t].data_ptr(), W, H) for t in range(13)]
        out = a.device_image(d_out[0].data_ptr(), 4 * W, 4 * H)
        assert a.prepare_frames(ins[0], out) == 2                 # (ju_prepare_frames works as before)
        before = a.stat("graph_replays")
        for t in range(13):
            drive_twin(b, recs, t)
            a.process(ins[t], out)
            assert np.array_equal(d_out[0].cpu().numpy(), b.process_image(clip[t])), t
            assert same_state(a, b), t
        assert a.stat("direct_graphs") >= 2 and a.stat("graph_replays") > before
        assert a.scene_info() == recs and np.array_equal(d_in.cpu().numpy(), clip)   # (the caller's frames: read in place)
        # a second pass over the same buffers: every tuple is captured by now, every frame replays a direct graph
        a.reset()
        b.reset()
        before = a.stat("graph_replays")
        eager = a.stat("eager_runs")
        det = S.Detector(THR, step=13)
        for t in range(13):
            rec = det.feed(clip[t])
            if rec["cut"]:
                b.reset()
            a.process(ins[t], out)
            assert np.array_equal(d_out[0].cpu().numpy(), b.process_image(clip[t])), t
            assert a.scene_info(1) == [rec]
        assert a.stat("graph_replays") == before + 13 and a.stat("eager_runs") == eager and same_state(a, b)


def test_process_frame_sees_the_decoded_frame():
    blob, clip, _ = known()
    planes = [source(f, NV12, CS) for f in clip]
    seen = [decoded(NV12, CS, p) for p in planes]
    recs = S.run(seen, THR)
    assert S.cuts(recs) == [4, 7, 10, 12]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_scene_detect(R.SCENE_RESET, THR)
        for t in range(13):
            drive_twin(b, recs, t)
            got, want = blank_planes(P010, 4 * H, 4 * W), blank_planes(P010, 4 * H, 4 * W)
            a.process_frame(R.host_frame(NV12, planes[t], CS), R.host_frame(R.FMT_P010, got, CS))
            b.process_frame(R.host_frame(NV12, planes[t], CS), R.host_frame(R.FMT_P010, want, CS))
            for g, e in zip(got, want):
                assert np.array_equal(g, e), t
            assert same_state(a, b), t
        assert a.scene_info() == recs


def test_enqueue_and_batch_and_group_run_the_detector_frame_by_frame():
    blob, clip, recs = known()
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b, \
            R.Runtime(blob, 0, R.DTYPE_F16) as plain, R.Runtime(blob, 0, R.DTYPE_F16) as plain_twin:
        a.set_scene_detect(R.SCENE_RESET, THR)
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        ins = [a.device_image(d_in[t].data_ptr(), W, H) for t in range(13)]
        outs = [a.device_image(d_out[t].data_ptr(), 4 * W, 4 * H) for t in range(13)]
        # ju_enqueue x 13, then ONE ju_get_scene_info
        for t in range(13):
            a.enqueue(ins[t], outs[t])
        assert a.scene_info() == recs                             # (it waits for the stream)
        want = twin_outputs(b, clip, recs)
        got = d_out.cpu().numpy()
        for t in range(13):
            assert np.array_equal(got[t], want[t]), t
        assert same_state(a, b)
        # ju_process_batch of 13 frames: no pass is formed, nothing is captured for one
        a.reset()
        b.reset()
        d_out.zero_()
        assert a.prepare_batch(ins[:4], outs[:4]) == 0
        a.process_batch(ins, outs)
        assert a.stat("lookahead_frames") == 0
        want = twin_outputs(b, clip, recs)
        got = d_out.cpu().numpy()
        for t in range(13):
            assert np.array_equal(got[t], want[t]), t
        assert same_state(a, b)
        assert a.scene_info(13) == [dict(r, step=13 + r["step"]) for r in recs]
        # ju_process_group of the detecting runtime with a plain one: member by member, both get their bytes
        a.reset()
        b.reset()
        p_out = d_out[0].clone()
        for t in range(13):
            drive_twin(b, recs, t)
            R.process_group([a, plain], [ins[t], ins[t]], [outs[t], plain.device_image(p_out.data_ptr(), 4 * W, 4 * H)])
            assert np.array_equal(d_out[t].cpu().numpy(), b.process_image(clip[t])), t
            assert np.array_equal(p_out.cpu().numpy(), plain_twin.process_image(clip[t])), t
        assert same_state(a, b) and same_state(plain, plain_twin)
        assert a.stat("group_frames") == 0 and a.stat("scene_cuts") == 12 and a.stat("scene_frames") == 39
        assert plain.stat("scene_frames") == 0


def test_with_a_source_size_the_detector_sees_the_scaled_frame():
    blob, _, _ = known()
    sh, sw = 48, 72
    clip = S.known_clip(M.synthetic_frames, sh, sw)
    seen = [SRC.scale(f, H, W) for f in clip]
    recs = S.run(seen, THR)
    assert S.cuts(recs) == [4, 7, 10, 12]
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_source_size(sw, sh)
        a.set_scene_detect(R.SCENE_RESET, THR)
        for t in range(13):
            drive_twin(b, recs, t)
            assert np.array_equal(a.process_image(clip[t]), b.process_image(seen[t])), t
            assert same_state(a, b), t
        assert a.scene_info() == recs


# ---- 6. lifecycle --------------------------------------------------------------------------------------------------------------
def test_lifecycle_reset_refusals_off_and_on_again():
    blob, clip, _ = known()
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_scene_detect(R.SCENE_RESET, THR)
        # ju_reset in front of frame 4: the setting stays, the next two frames never cut, `step` goes on
        det = S.Detector(THR)
        want = []
        for t in range(13):
            if t == 4:
                a.reset()
                b.reset()
                det.restart()
                assert a.get_scene_detect() == (R.SCENE_RESET, THR)
            rec = det.feed(clip[t])
            want.append(rec)
            if rec["cut"]:
                b.reset()
            assert np.array_equal(a.process_image(clip[t]), b.process_image(clip[t])), t
        assert a.scene_info() == want and [r["cut"] for r in want[4:6]] == [0, 0] and S.cuts(want) == [7, 10, 12]
        assert same_state(a, b)
        # refused calls: an unknown mode, thresholds out of range (Python and C, one message), a frame of the wrong size
        for mode, thr in ((3, THR), (1, 0), (2, 255001)):
            with pytest.raises(R.JoshUpscaleError) as e:
                a.set_scene_detect(mode, thr)
            assert e.value.code == 1 and e.value.message == "std::invalid_argument: ju_set_scene_detect: " + S.problem(mode, thr)
        assert a.get_scene_detect() == (R.SCENE_RESET, THR)
        out = np.zeros((4 * H, 4 * W, 4), np.uint8)
        good = R.host_image(clip[0])
        d_good, d_big = device_clip(clip[:1], 4 * H + 1, 4 * W)
        refused = [
            # a bad input
            lambda: a.process(R.host_image(np.zeros((H + 1, W, 4), np.uint8)), R.host_image(out)),
            lambda: a.process_frame(R.host_frame(R.FMT_BGRX, [np.zeros((H, W + 2, 4), np.uint8)]), R.host_frame(R.FMT_BGRX, [out])),
            # a good input with a bad output, host and device: the wrong size, a stride shorter than a row
            lambda: a.process(good, R.host_image(np.zeros((4 * H + 1, 4 * W, 4), np.uint8))),
            lambda: a.process(good, R.JuImage(out.ctypes.data, R.LOC_CPU, 4 * W * 4 - 4, 4 * W, 4 * H)),
            lambda: a.process(a.device_image(d_good[0].data_ptr(), W, H), a.device_image(d_big[0].data_ptr(), 4 * W, 4 * H + 1)),
            lambda: a.process(good, a.device_image(d_big[0].data_ptr(), 4 * W, 4 * H, stride=8)),
        ]
        for k, call in enumerate(refused):
            with pytest.raises(R.JoshUpscaleError):
                call()
            assert a.stat("scene_detector_runs") == 13 and a.scene_info() == want, k
        assert same_state(a, b)                                   # (no step happened, nothing was cleared)
        # a device pair captured while the detector was on ...
        d_in, d_out = device_clip(clip[:4], 4 * H, 4 * W)
        ins = [a.device_image(d_in[t].data_ptr(), W, H) for t in range(4)]
        outs = [a.device_image(d_out[t].data_ptr(), 4 * W, 4 * H) for t in range(4)]
        a.prepare_frames(ins[0], outs[0])
        rec = det.feed(clip[0])                                   # (scene 1 behind the flash: a cut)
        assert rec["cut"] == 1
        b.reset()
        a.process(ins[0], outs[0])
        assert np.array_equal(d_out[0].cpu().numpy(), b.process_image(clip[0])) and a.scene_info(1) == [rec]
        # ... off: its graphs still serve, look-ahead passes are back, the counters stay
        a.set_scene_detect(R.SCENE_OFF)
        assert a.get_scene_detect() == (R.SCENE_OFF, 0) and a.scene_info() == [] and a.stat("scene_mode") == 0
        assert a.stat("scene_frames") == 14 and a.stat("scene_cuts") == 4
        a.process(ins[0], outs[0])
        assert np.array_equal(d_out[0].cpu().numpy(), b.process_image(clip[0]))
        a.process_batch(ins, outs)
        assert a.stat("lookahead_frames") == 4 and a.stat("scene_detector_runs") == 14
        got = d_out.cpu().numpy()
        for t in range(4):
            assert np.array_equal(got[t], b.process_image(clip[t])), t
        assert same_state(a, b)
        # on again: step 0, no predecessor
        a.set_scene_detect(R.SCENE_REPORT, THR)
        assert a.scene_info() == []
        a.process_image(clip[12])
        b.process_image(clip[12])
        assert a.scene_info() == [{"step": 0, "sad": 0, "score": 0, "cut": 0}] and same_state(a, b)


def test_the_ring_keeps_the_last_64_decisions():
    blob, clip, _ = known()
    frames = [clip[t % 13] for t in range(70)]
    want = S.run(frames, THR)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        a.set_scene_detect(R.SCENE_REPORT, THR)
        d_in, d_out = device_clip(clip, 4 * H, 4 * W)
        out = a.device_image(d_out[0].data_ptr(), 4 * W, 4 * H)
        for t in range(70):
            a.enqueue(a.device_image(d_in[t % 13].data_ptr(), W, H), out)
        assert a.scene_info() == want[6:] and a.scene_info(3) == want[67:] and a.scene_info(0) == []
        assert a.scene_info(1000) == want[6:]
        assert a.stat("scene_frames") == 70 and a.stat("scene_cuts") == len(S.cuts(want))


# ---- 7. a flow-free model -------------------------------------------------------------------------------------------------------
def test_a_flow_free_model_reports_and_changes_no_byte():
    _, clip, recs = known()
    cfg, wts = flow_free(small_config())
    blob = M.serialize(cfg, wts)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        assert not a.recurrent
        a.set_scene_detect(R.SCENE_RESET, THR)
        assert a.get_scene_detect() == (R.SCENE_RESET, THR)
        for t, f in enumerate(clip):
            assert np.array_equal(a.process_image(f), b.process_image(f)), t
        assert a.scene_info() == recs and a.stat("scene_cuts") == 4


# ---- 8. the re-run of a step ----------------------------------------------------------------------------------------------------
def test_a_step_that_is_run_again_meets_the_detector_once():
    blob, clip, recs = known()
    lib = R.load_library(True)
    with R.Runtime(blob, 0, R.DTYPE_F16) as a, R.Runtime(blob, 0, R.DTYPE_F16) as b:
        a.set_scene_detect(R.SCENE_RESET, THR)
        outs = twin_outputs(b, clip, recs)
        assert lib.ju_debug_set(b"step_rerun", 1) == 0
        try:
            for t, f in enumerate(clip):
                assert np.array_equal(a.process_image(f), outs[t]), t
                assert a.scene_info(1) == [recs[t]], t            # the first run's decision stands, S_t with it
        finally:
            lib.ju_debug_set(b"step_rerun", 0)
        assert same_state(a, b)
        assert a.stat("graph_replays") + a.stat("eager_runs") == 26      # every step was submitted twice ...
        assert a.stat("scene_detector_runs") == 13 and a.stat("scene_frames") == 13   # ... and met the detector once
        assert a.scene_info() == recs
    with R.Runtime(blob, 0, R.DTYPE_F16, hooks=False) as p:       # the product library does not answer the test counter
        with pytest.raises(R.JoshUpscaleError):
            p.stat("scene_detector_runs")
        assert p.stat("scene_frames") == 0
