"""The scene detector inside group passes (ju_set_scene_group; csrc/scene_kernels.hip scene_group_kernel and
scene_clear_items_kernel, engine_passes.cpp "Group passes"; docs/scene_detect.md "Group passes"): the two kernels alone
against the Python definition (tests/scene_reference.py), and ju_process_group of detecting members against twins driven
frame by frame by ju_process with the same detector setting -- every comparison byte or integer equality."""

import ctypes as C

import numpy as np
import pytest

import scene_reference as S
from flowfree_common import flow_free
from helpers import M, small_config
from joshupscale_amd import runtime as R
from test_gpu_scene import LAYOUTS, STATE_BYTES, Guarded, known, state_words
from test_gpu_yuv import DevPlane, torch_dev
from test_group_frames_cpu import ROTATED_CUTS, rotated

pytestmark = pytest.mark.gpu

THR = S.KNOWN_THRESHOLD
H, W = 30, 48
MEMBERS, TICKS = 8, 13
_CACHE = {}


# ---- 1. scene_group_kernel alone -------------------------------------------------------------------------------------------
def debug_group(frames, hw, prevs, states, has_prev, steps, thrs, modes):
    """One launch over len(frames) items (None: an absent item); -> (records, reset flags)."""
    n = len(frames)
    lib = R.load_library(True)
    recs, flags = (R.JuSceneInfo * n)(), (C.c_uint32 * n)()
    rc = lib.ju_debug_scene_group(
        n, (C.c_void_p * n)(*[f.ptr if f is not None else None for f in frames]),
        (C.c_ssize_t * n)(*[f.stride if f is not None else 0 for f in frames]), hw[1], hw[0],
        (C.c_void_p * n)(*[p.ptr for p in prevs]), (C.c_void_p * n)(*[s.data_ptr() for s in states]),
        (C.c_int * n)(*has_prev), (C.c_uint64 * n)(*steps), (C.c_uint32 * n)(*thrs), (C.c_int * n)(*modes), recs, flags)
    assert rc == 0, lib.ju_last_error()
    return [{"step": r.step, "sad": r.sad, "score": r.score, "cut": int(r.cut)} for r in recs], list(flags)


def make_state(s_before):
    torch, dev = torch_dev()
    words = np.zeros(STATE_BYTES // 8, np.uint64)
    words[2] = s_before
    return torch.from_numpy(words.view(np.uint8).copy()).to(dev)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_group_kernel_equals_the_definition_per_item(n):
    torch, dev = torch_dev()
    names = sorted(LAYOUTS)
    absent = 1 if n >= 3 else -1
    for hw in [(2, 2), (7, 301), (30, 48)]:
        pixel_bytes = 3 * hw[0] * hw[1]
        rng = np.random.default_rng(1000 * n + hw[1])
        old = [rng.integers(0, 256, hw + (4,), dtype=np.uint8) for _ in range(n)]      # (garbage where has_prev is 0)
        cur = [rng.integers(0, 256, hw + (4,), dtype=np.uint8) for _ in range(n)]
        nxt = [rng.integers(0, 256, hw + (4,), dtype=np.uint8) if i % 2 else np.full(hw + (4,), 255, np.uint8) for i in range(n)]
        has_prev = [(3, 0, 1, 3)[i % 4] for i in range(n)]
        thrs = [(THR, 50)[(i // 2) % 2] for i in range(n)]
        modes = [(S.RESET, S.REPORT, S.RESET)[i % 3] for i in range(n)]
        steps = [0, 5, 63, 64, 1000, 2 ** 40, 7, 127][:n]
        # S before, where two frames went before: 0 (D = S), S itself (D = 0), S - N / 10 (a cut at 50, none at 22000)
        sums = [S.sad(cur[i], old[i]) for i in range(n)]
        s_before = [(0, sums[i], max(sums[i] - pixel_bytes // 10, 0))[(i // 4 + i) % 3] if has_prev[i] == 3 else 0 for i in range(n)]
        dets = []
        for i in range(n):
            det = S.Detector(thrs[i], step=steps[i])
            det.seen = {0: 0, 1: 1, 3: 2}[has_prev[i]]
            det.prev, det.s_before = old[i], s_before[i]
            dets.append(det)
        states = [make_state(s) for s in s_before]
        prevs = [DevPlane(o) for o in old]
        before = [s.cpu().numpy().copy() for s in states]
        torch.cuda.synchronize()
        total_cuts = [0] * n
        for run, frames_now in enumerate((cur, nxt)):             # the second launch continues each item's sequence
            planes = [None if i == absent else DevPlane(frames_now[i], **LAYOUTS[names[(i + run) % 4]]) for i in range(n)]
            hp = has_prev if run == 0 else [1 if h == 0 else 3 for h in has_prev]
            torch.cuda.synchronize()
            recs, flags = debug_group(planes, hw, prevs, states, hp, [s + run for s in steps], thrs, modes)
            for i in range(n):
                q, w = state_words(states[i])
                if i == absent:
                    assert recs[i] == {"step": 0, "sad": 0, "score": 0, "cut": 0} and flags[i] == 0
                    prevs[i].check(old[i])                        # an absent item's memory: untouched
                    assert np.array_equal(states[i].cpu().numpy(), before[i])
                    continue
                want = dets[i].feed(frames_now[i])
                total_cuts[i] += want["cut"]
                assert recs[i] == want, (hw, run, i, recs[i], want)
                assert flags[i] == (1 if want["cut"] and modes[i] == S.RESET else 0) == w[3], (hw, run, i)
                prevs[i].check(frames_now[i])                     # the kept frame is the item byte for byte, X included
                planes[i].check(frames_now[i])                    # the frame and its guard bytes untouched
                assert q[0] == 0 and w[2] == 0, (hw, run, i)      # every accumulator and every ticket word
                assert q[2] == want["sad"] and q[3] == run + 1 and q[4] == total_cuts[i], (hw, run, i)


def test_group_kernel_sums_in_64_bits():
    torch, dev = torch_dev()
    hw = (2400, 2400)
    black, white = np.zeros(hw + (4,), np.uint8), np.full(hw + (4,), 255, np.uint8)
    frames = [DevPlane(white), DevPlane(black)]
    prevs = [DevPlane(black), DevPlane(black)]
    states = [make_state(0), make_state(0)]
    torch.cuda.synchronize()
    recs, flags = debug_group(frames, hw, prevs, states, [3, 3], [0, 0], [S.THRESHOLD_MAX] * 2, [S.RESET] * 2)
    want = 3 * 2400 * 2400 * 255
    assert want > 2 ** 32
    assert recs[0] == {"step": 0, "sad": want, "score": want, "cut": 1} and flags[0] == 1
    assert recs[1] == {"step": 0, "sad": 0, "score": 0, "cut": 0} and flags[1] == 0
    prevs[0].check(white)
    prevs[1].check(black)
    for s in states:
        q, w = state_words(s)
        assert q[0] == 0 and w[2] == 0


# ---- 2. scene_clear_items_kernel alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [(1, 0, 1, 1, 0, 0, 1, 0), (0,) * 8, (1,) * 8], ids=["mixed", "none", "all"])
def test_clear_items_kernel_obeys_each_flag_and_the_bounds(flags):
    torch, dev = torch_dev()
    lib = R.load_library(True)
    sizes = [17, 4081, 1000017, 250, 65521, 31, 100003, 4097]     # none a multiple of 16
    offsets = [0, 1, 4, 15]
    a = [Guarded(sizes[i], offsets[i % 4], i) for i in range(8)]
    b = [Guarded(sizes[(i + 3) % 8], offsets[(i + 1) % 4], 20 + i) for i in range(8)]
    words = torch.tensor(flags, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = lib.ju_debug_scene_clear_items(
        8, (C.c_void_p * 8)(*[words.data_ptr() + 4 * i for i in range(8)]),
        (C.c_void_p * 8)(*[x.ptr for x in a]), (C.c_size_t * 8)(*[x.size for x in a]),
        (C.c_void_p * 8)(*[x.ptr for x in b]), (C.c_size_t * 8)(*[x.size for x in b]))
    assert rc == 0, lib.ju_last_error()
    for i in range(8):
        a[i].check(bool(flags[i]))                                # flagged pairs all zero, the others untouched, guards intact
        b[i].check(bool(flags[i]))
    assert tuple(words.cpu().tolist()) == flags


# ---- 3. end to end, JU_SCENE_RESET -------------------------------------------------------------------------------------------
def twins(dtype, mode=R.SCENE_RESET, thr=THR):
    """Per member k, the rotated clip three times through ju_process on a runtime with the same detector setting (a
    ju_reset in front of the second round): outputs[round][k][t], (state, flow_in)[round][k], scene_info(13)[round][k]."""
    key = ("twins", dtype, mode, thr)
    if key not in _CACHE:
        blob, clip, _ = known()
        outs, tensors, infos = ([[None] * MEMBERS for _ in range(3)] for _ in range(3))
        for k in range(MEMBERS):
            rot = rotated(clip, k)
            with R.Runtime(blob, 0, dtype) as b:
                if mode != R.SCENE_OFF:
                    b.set_scene_detect(mode, thr)
                for r in range(3):
                    if r == 1:
                        b.reset()
                    outs[r][k] = [b.process_image(f).copy() for f in rot]
                    tensors[r][k] = (b.read_tensor("state").copy(), b.read_tensor("flow_in").copy())
                    infos[r][k] = b.scene_info(TICKS)
        _CACHE[key] = (outs, tensors, infos)
    return _CACHE[key]


def device_streams(clip, members):
    """Member k's rotated clip and one output frame per member, on the device."""
    torch, dev = torch_dev()
    d_in = torch.from_numpy(np.stack([np.stack(rotated(clip, k)) for k in range(members)])).to(dev)
    d_out = torch.zeros((members, 4 * H, 4 * W, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return d_in, d_out


def tick(rts, d_in, d_out, t, ks=None):
    ks = list(range(len(rts))) if ks is None else ks
    R.process_group(rts, [rt.device_image(d_in[k][t].data_ptr(), W, H) for rt, k in zip(rts, ks)],
                    [rt.device_image(d_out[k].data_ptr(), 4 * W, 4 * H) for rt, k in zip(rts, ks)])
    return d_out.cpu().numpy()


def same_tensors(rt, pair):
    return np.array_equal(rt.read_tensor("state"), pair[0]) and np.array_equal(rt.read_tensor("flow_in"), pair[1])


@pytest.mark.parametrize("cap", [8, 3])
@pytest.mark.parametrize("dtype", [R.DTYPE_F16, R.DTYPE_BF16], ids=["fp16", "bf16"])
def test_reset_mode_in_group_passes_equals_the_per_frame_twins(dtype, cap):
    blob, clip, _ = known()
    outs, tensors, infos = twins(dtype)
    rts = [R.Runtime(blob, 0, dtype) for _ in range(MEMBERS)]
    try:
        rts[0].set_lookahead(cap)                                 # (3: passes of 3 + 3 + 2)
        for rt in rts:
            rt.set_scene_detect(R.SCENE_RESET, THR)
            rt.set_scene_group(1)
            assert rt.stat("scene_group") == 1
        d_in, d_out = device_streams(clip, MEMBERS)
        dets = [S.Detector(THR) for _ in range(MEMBERS)]
        for r in range(3):                                        # round 2 after ju_reset of every member, round 3 straight on
            if r == 1:
                for rt, det in zip(rts, dets):
                    rt.reset()
                    det.restart()
            want = [[dets[k].feed(f) for f in rotated(clip, k)] for k in range(MEMBERS)]
            if r == 0:
                assert {k: S.cuts(want[k]) for k in range(MEMBERS)} == ROTATED_CUTS
            for t in range(TICKS):
                got = tick(rts, d_in, d_out, t)
                for k in range(MEMBERS):
                    assert np.array_equal(got[k], outs[r][k][t]), (r, t, k)
            for k, rt in enumerate(rts):
                assert same_tensors(rt, tensors[r][k]), (r, k)
                assert rt.scene_info(TICKS) == infos[r][k] == want[k], (r, k)
                assert want[k][0]["step"] == 13 * r
                n = 13 * (r + 1)
                assert rt.stat("group_frames") == rt.stat("scene_group_frames") == n, (r, k)
                assert rt.stat("scene_detector_runs") == n and rt.stat("scene_frames") == n and rt.stat("fallbacks") == 0
        assert np.array_equal(d_in.cpu().numpy(), np.stack([np.stack(rotated(clip, k)) for k in range(MEMBERS)]))
    finally:
        for rt in rts:
            rt.close()


# ---- 4. mixed members in one call -------------------------------------------------------------------------------------------
def test_members_with_and_without_a_detector_share_a_pass():
    blob, clip, _ = known()
    dtype = R.DTYPE_F16
    plain = twins(dtype, R.SCENE_OFF, 0)[0][0]                    # the undetecting twins' outputs, round 1
    reset_outs, reset_tensors, reset_infos = twins(dtype)
    kinds = [(R.SCENE_OFF, 0, 0), (R.SCENE_REPORT, 50, 1), (R.SCENE_RESET, THR, 1), (R.SCENE_RESET, THR, 0)]
    rts = [R.Runtime(blob, 0, dtype) for _ in kinds]
    try:
        for rt, (mode, thr, on) in zip(rts, kinds):
            if mode != R.SCENE_OFF:
                rt.set_scene_detect(mode, thr)
            rt.set_scene_group(on)
        d_in, d_out = device_streams(clip, 4)
        for t in range(TICKS):
            got = tick(rts, d_in, d_out, t)
            assert np.array_equal(got[0], plain[0][t]) and np.array_equal(got[1], plain[1][t]), t   # REPORT changes no byte
            assert np.array_equal(got[2], reset_outs[0][2][t]) and np.array_equal(got[3], reset_outs[0][3][t]), t
        assert rts[0].scene_info() == []
        assert rts[1].scene_info() == S.run(rotated(clip, 1), 50)
        for k in (2, 3):
            assert rts[k].scene_info() == reset_infos[0][k] == S.run(rotated(clip, k), THR)
            assert same_tensors(rts[k], reset_tensors[0][k])
        assert [rt.stat("group_frames") for rt in rts] == [13, 13, 13, 0]   # the setting left at 0: alone, as before
        assert [rt.stat("scene_group_frames") for rt in rts] == [0, 13, 13, 0]
        assert [rt.stat("scene_detector_runs") for rt in rts] == [0, 13, 13, 13]
    finally:
        for rt in rts:
            rt.close()


# ---- 5. a group pass that is run again ---------------------------------------------------------------------------------------
def test_a_group_pass_that_is_run_again_meets_the_detector_once():
    blob, clip, _ = known()
    dtype = R.DTYPE_F16
    outs, tensors, infos = twins(dtype)
    lib = R.load_library(True)
    rts = [R.Runtime(blob, 0, dtype) for _ in range(MEMBERS)]
    try:
        for rt in rts:
            rt.set_scene_detect(R.SCENE_RESET, THR)
            rt.set_scene_group(1)
        d_in, d_out = device_streams(clip, MEMBERS)
        assert lib.ju_debug_set(b"group_rerun", 1) == 0
        try:
            for t in range(TICKS):
                got = tick(rts, d_in, d_out, t)
                for k in range(MEMBERS):
                    assert np.array_equal(got[k], outs[0][k][t]), (t, k)
        finally:
            lib.ju_debug_set(b"group_rerun", 0)
        for k, rt in enumerate(rts):
            assert same_tensors(rt, tensors[0][k]), k
            recs = rt.scene_info()
            assert recs == infos[0][k] and [r["step"] for r in recs] == list(range(TICKS)), k   # no record twice
            assert rt.stat("scene_detector_runs") == 13 and rt.stat("scene_frames") == 13, k
            assert rt.stat("scene_group_frames") == 13 and rt.stat("group_frames") == 0 and rt.stat("fallbacks") == 0
    finally:
        for rt in rts:
            rt.close()


# ---- 6. the setting ------------------------------------------------------------------------------------------------------------
def test_the_setting_its_default_its_refusals_and_what_keeps_it():
    blob, _, _ = known()
    with R.Runtime(blob, 0, R.DTYPE_F16) as a:
        assert a.stat("scene_group") == 0 and a.stat("scene_group_frames") == 0
        for bad in (2, -1):
            with pytest.raises(R.JoshUpscaleError) as err:
                a.set_scene_group(bad)
            assert f"ju_set_scene_group: on must be 0 or 1, got {bad}" in str(err.value)
            assert a.stat("scene_group") == 0
        a.set_scene_group(1)
        assert a.stat("scene_group") == 1
        a.reset()
        a.set_scene_detect(R.SCENE_RESET, THR)
        a.set_scene_detect(R.SCENE_OFF, 0)
        a.set_scene_detect(R.SCENE_REPORT, 50)
        a.reset()
        assert a.stat("scene_group") == 1
        a.set_scene_group(0)
        assert a.stat("scene_group") == 0


def test_a_flow_free_model_in_reset_mode_reports_and_changes_no_byte():
    _, clip, _ = known()
    cfg, wts = flow_free(small_config())
    blob = M.serialize(cfg, wts)
    rts = [R.Runtime(blob, 0, R.DTYPE_F16) for _ in range(2)]
    try:
        with R.Runtime(blob, 0, R.DTYPE_F16) as twin:
            want = [[twin.process_image(f).copy() for f in rotated(clip, k)] for k in range(2)]
        for rt in rts:
            assert not rt.recurrent
            rt.set_scene_detect(R.SCENE_RESET, THR)
            rt.set_scene_group(1)
        d_in, d_out = device_streams(clip, 2)
        for t in range(TICKS):
            got = tick(rts, d_in, d_out, t)
            for k in range(2):
                assert np.array_equal(got[k], want[k][t]), (t, k)
        for k, rt in enumerate(rts):
            assert rt.scene_info() == S.run(rotated(clip, k), THR) and rt.stat("scene_cuts") == len(ROTATED_CUTS[k])
            assert rt.stat("group_frames") == rt.stat("scene_group_frames") == 13
    finally:
        for rt in rts:
            rt.close()
